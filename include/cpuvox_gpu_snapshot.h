/* cpuvox_gpu_snapshot.h -- snapshots of rectangles of the uploaded world that stay on the device: six entry points of libcpuvox_gpu.so (the
 * product library exports them like those of include/cpuvox_gpu.h; they are declared here, in a header of their own that includes it, so that
 * the list of include/cpuvox_gpu.h stays what its hosts were built against).  Error codes, cvx_context and cvx_last_error are
 * include/cpuvox_gpu.h's. */
#ifndef CPUVOX_GPU_SNAPSHOT_H
#define CPUVOX_GPU_SNAPSHOT_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*  * A snapshot keeps the columns of a rectangle, at LOD 0 and the coarse levels over it, in device memory of its own: what a host needs to
 * take a change back (an undo stack), to relight a world it has edited (cvx_world_light is one-shot: the unlit rectangle is kept here instead
 * of going to the host with cvx_world_read_region and back with cvx_world_edit), to stamp a dynamic object for a frame and take it out again,
 * and to ask which columns a call really changed.  Nothing but totals crosses to the host.
 *
 * cvx_world_snapshot: captures the rectangle [x0, x0 + sizeX) x [z0, z0 + sizeZ) of LOD-0 columns and the levels 0 .. levelCount (0 .. 5).
 *   Rectangle: rounded outward to multiples of 2^levelCount and clipped to the world, as the brush rounds its footprint; it must meet the
 *     world (sizeX, sizeZ >= 1, x0 < dimX, z0 < dimZ, x0 + sizeX > 0, z0 + sizeZ > 0).  cvx_snapshot_info_get reports what is held.
 *   Contents: for every level k <= levelCount the columns of (rectangle >> k) exactly as level k holds them at the time of the call -- a coarse
 *     level that an earlier edit with a smaller levelCount left stale is captured stale.  Each level is one sub-world blob in the reference's
 *     layout and the builder's encoding, byte for byte what cvx_world_read_region(k, rectangle >> k) returns, in device memory that the
 *     snapshot owns (info.deviceBytes: 12 bytes per column and 4 per element, all levels together).
 *   Ordering: behind everything enqueued on the context's stream before it; levels uploaded but not yet placed are placed first; returns when
 *     the snapshot is complete.  The world is not changed and cvx_world_edit_stats is as before.  outDeviceMs may be NULL.
 *   A snapshot is independent of the arena: later edits, cvx_world_compact, a new layout of the arena and a re-upload of the world leave it
 *     valid.  It belongs to ONE context and must be destroyed (cvx_snapshot_destroy, NULL allowed) before that context is; until then it may
 *     be restored and compared any number of times.
 *   CVX_ERR_INVALID_ARGUMENT: NULL ctx / out; levelCount outside 0 .. 5; a rectangle that does not meet the world; a world narrower than
 *     2^levelCount.  CVX_ERR_NOT_READY: a level has not been uploaded.  CVX_ERR_CAPACITY: a rectangle of 2^31 / 12 columns or more, a level
 *     of 2^31 elements or more, out of device memory.  *out is NULL on failure.
 *
 * cvx_world_snapshot_restore: puts every held level back over its rectangle.
 *   Afterwards cvx_world_read_region(k, rectangle >> k) returns, for every k <= levelCount, byte for byte what it returned when the snapshot
 *     was taken; every column outside the rectangle and every level above levelCount is untouched.  No level is rebuilt from another: the
 *     coarse columns are the held ones.
 *   Ordering, atomicity and several GPUs are cvx_world_edit's: a draw enqueued before the restore renders the old world, a failure leaves the
 *     world as it was, every rank restores its own snapshot.  Columns go to their old places when they fit and to the tails otherwise; a
 *     restore may lay the arena out again or grow it, as any edit may.  A snapshot can be restored any number of times and in any order with
 *     others; where two overlap the later restore wins.
 *   CVX_ERR_INVALID_ARGUMENT: NULL ctx / snap; a snapshot of another context; a world whose dimX / dimY / dimZ are no longer the snapshot's
 *     (an upload of a different world).  CVX_ERR_NOT_READY, CVX_ERR_CAPACITY: as cvx_world_edit.
 *
 * cvx_world_snapshot_diff / _device: compares LOD 0 of the world as it is now with the snapshot's LOD 0.  Integers and bytes only.
 *   Voxel (x, y, z) of the rectangle DIFFERS iff it is solid in one and air in the other, or solid in both with different colour words; under
 *     CVX_SNAPSHOT_IGNORE_COLOUR only solidity counts.  A column is CHANGED iff one of its voxels differs; its entry holds the lowest differing
 *     y as yMin and the highest + 1 as yMax.  How a column is encoded never counts.
 *   The changed columns are listed in the rectangle's column order, x ascending, then z; the list is a function of the two worlds alone.
 *     `changes` receives the first min(changeCapacity, changedColumns) entries; a smaller capacity is not an error (cvx_world_pieces'
 *     convention), and `changes` may be NULL iff changeCapacity is 0.  cvx_world_snapshot_diff_device leaves the list in device memory (a torch
 *     tensor's data_ptr()); both return the summary (may be NULL) on the host: the totals and the tight bounding box of the differing voxels.
 *   Ordering as the capture's; the world is not changed, cvx_world_edit_stats is as before, the scratch (12 bytes per column of the
 *     rectangle and 40 per 256 of them) is freed before the call returns.
 *   CVX_ERR_INVALID_ARGUMENT: as restore, and unknown flag bits, a negative changeCapacity, NULL `changes` with a capacity above 0.
 *   CVX_ERR_NOT_READY: LOD 0 has not been uploaded.  CVX_ERR_CAPACITY: out of device memory. */
typedef struct cvx_snapshot cvx_snapshot;           /* opaque; owns device memory; belongs to ONE context */

typedef struct cvx_snapshot_info {                  /* 48 bytes */
    int32_t x0, z0, sizeX, sizeZ;                   /* the rectangle actually held, LOD-0 columns (rounded, clipped) */
    int32_t levelCount;                             /* levels 0 .. levelCount are held */
    int32_t dimX, dimY, dimZ;                       /* the world it was taken from */
    int64_t deviceBytes;                            /* what the snapshot holds on the device */
    int64_t elements;                               /* blob elements, all levels together */
} cvx_snapshot_info;

typedef struct cvx_snapshot_change {                /* 16 bytes */
    int32_t x, z;                                   /* LOD-0 column */
    int32_t yMin, yMax;                             /* its differing voxels lie in [yMin, yMax), both ends tight */
} cvx_snapshot_change;

typedef struct cvx_snapshot_diff_summary {          /* 48 bytes */
    int64_t changedColumns, changedVoxels;
    int32_t min[3], max[3];                         /* bounding box of the differing voxels, incl / excl; all 0 when nothing differs */
    int32_t pad_[2];
} cvx_snapshot_diff_summary;

enum { CVX_SNAPSHOT_IGNORE_COLOUR = 1 };            /* diff flags */

int  cvx_world_snapshot(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, int levelCount, cvx_snapshot **out, float *outDeviceMs);
int  cvx_snapshot_info_get(const cvx_snapshot *snap, cvx_snapshot_info *out);
int  cvx_world_snapshot_restore(cvx_context *ctx, const cvx_snapshot *snap, float *outDeviceMs);
int  cvx_world_snapshot_diff(cvx_context *ctx, const cvx_snapshot *snap, int flags, cvx_snapshot_change *changes, int64_t changeCapacity,
                             cvx_snapshot_diff_summary *summary, float *outDeviceMs);
int  cvx_world_snapshot_diff_device(cvx_context *ctx, const cvx_snapshot *snap, int flags, cvx_snapshot_change *changesDevice, int64_t changeCapacity,
                                    cvx_snapshot_diff_summary *summary, float *outDeviceMs);
void cvx_snapshot_destroy(cvx_snapshot *snap);

#ifdef __cplusplus
}
#endif
#endif
