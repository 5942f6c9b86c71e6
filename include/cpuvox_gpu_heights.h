/* cpuvox_gpu_heights.h -- terrain as height maps out of and into the uploaded world: four entry points of libcpuvox_gpu.so (the product library
 * exports them like those of include/cpuvox_gpu.h; they are declared here, in a header of their own that includes it, so that the list of
 * include/cpuvox_gpu.h stays what its hosts were built against).  Error codes, cvx_context, the op constants and cvx_last_error are
 * include/cpuvox_gpu.h's. */
#ifndef CPUVOX_GPU_HEIGHTS_H
#define CPUVOX_GPU_HEIGHTS_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*  * cvx_world_read_heights / cvx_world_write_heights: the ground as every voxlap-lineage engine starts from it, one height and one colour per
 * column -- spawn heights, minimaps, blob shadows, the camera's floor on the way out; raise, lower, smooth and flatten tools, generated or
 * imported terrain on the way in, without a dense (X, Z, Y) array in between.  No RLE columns are encoded or decoded on the host.
 *   Arrays and box.  Coordinates are LOD-0 voxels of the stored tile (a repeating world does not wrap them), every |coordinate| <= 2^30.  All
 *     arrays are (X, Z), z fastest: X = boxMax.x - boxMin.x, Z = boxMax.z - boxMin.z, the footprint of a dense box, X * Z < 2^31; column (x, z)
 *     is element (x - boxMin.x) * Z + (z - boxMin.z).  [boxMin.y, boxMax.y) is the window [y0, y1).  The box may stick out of the world on any
 *     side.
 *   Read.  For column (x, z), with the window clipped to [0, dimY): heights = 1 + the y of the highest solid voxel in the window, y0 (unclipped)
 *     when there is none or the column lies outside the world; argb = that voxel's colour word, 0 when there is none; bottoms = the lowest
 *     b >= max(y0, 0) with [b, heights) all solid -- the thickness of the top layer, so that a second call with y1 = bottoms peels the next
 *     one -- and y0 when there is none.  Any of the three may be NULL, not all.  Ordering, streams and outDeviceMs as cvx_world_read_voxels /
 *     cvx_world_read_voxels_device.
 *   Write.  DEFINED as cvx_world_write_voxels with the same box, op (CVX_BRUSH_FILL, CARVE, PAINT, CVX_COPY_REPLACE) and levelCount and a solid
 *     mask and colour array that are never materialised.  With H = clamp(heights[x, z], y0, y1): set(x, y, z) iff b(x, z) <= y < H(x, z), where
 *     thickness 0: b = y0 (solid down to the window's bottom); thickness t = 1 .. 32767: b = max(y0, min(H, N) - t), a crust, N the smallest H
 *     of the four edge neighbours in the arrays.  A neighbour outside the footprint counts as the column's own H; under CVX_HEIGHTS_WALLED it
 *     counts as y0, so that the rim becomes a wall down to the window's bottom.  t = 1 is the thinnest crust without holes between face
 *     neighbours, t = 2 the procedural world's rule.  A set voxel's colour is argb[x, z] for y == H - 1 and sideArgb[x, z] below it (argb[x, z]
 *     too when sideArgb is NULL); argb may be NULL only for a CARVE.  Entries over columns outside the world are still neighbours; their
 *     voxels are dropped, as in the dense write.  So REPLACE is "the window of these columns becomes this terrain" (raising and lowering are
 *     the same call), FILL adds terrain under what is there, CARVE with thickness 0 cuts a terrain-shaped volume out.  Tiles written one by one
 *     overlap by a column and use FILL, or pass WALLED: REPLACE on a tile's rim column only knows the neighbours inside the tile.
 *     Rectangle, LOD rebuild, ordering, atomicity, outDeviceMs, CVX_ERR_CAPACITY (a column with a run or a colour index above 32767 or more
 *     than 65535 runs -- thickness 0 over a window taller than 32767, say --, the arena limits) and CVX_ERR_NOT_READY are
 *     cvx_world_write_voxels'; every error leaves the world as it was.  A box wholly outside the world: CVX_OK, nothing is written,
 *     *outDeviceMs = 0.  cvx_world_write_heights_device reads its device arrays on the context's stream: the caller makes sure they are
 *     complete when it calls and leaves them alone until it returns.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued: NULL box pointers, an empty axis, a coordinate beyond 2^30,
 * X * Z >= 2^31, all three outputs NULL on a read, heights NULL on a write, argb NULL unless the op is CARVE, thickness outside 0 .. 32767,
 * unknown flag bits, a bad op, levelCount outside 0 .. 5.  Device memory while a call runs: the host-array calls hold their arrays (4 bytes
 * per column each); a write adds cvx_world_brush's scratch for its rectangle, 4 more bytes per column of it (the run counts) and the
 * rectangle's new columns.  With several GPUs every rank applies the same write to its own context. */
#define CVX_HEIGHTS_WALLED 1 /* flags: a neighbour outside the footprint counts as y0 */
int cvx_world_read_heights(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int32_t *heights, uint32_t *argb, int32_t *bottoms,
                           float *outDeviceMs);
int cvx_world_read_heights_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int32_t *heightsDevice, uint32_t *argbDevice,
                                  int32_t *bottomsDevice, void *hipStream);
int cvx_world_write_heights(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const int32_t *heights, const uint32_t *argb,
                            const uint32_t *sideArgb, int thickness, int flags, int op, int levelCount, float *outDeviceMs);
int cvx_world_write_heights_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const int32_t *heightsDevice,
                                   const uint32_t *argbDevice, const uint32_t *sideArgbDevice, int thickness, int flags, int op, int levelCount,
                                   float *outDeviceMs);

#ifdef __cplusplus
}
#endif
#endif
