/* cpuvox_gpu_spread.h -- travel-distance fields through the air or the solid of the uploaded world: two entry points of libcpuvox_gpu.so (the
 * product library exports them like those of include/cpuvox_gpu.h; they are declared here, in a header of their own that includes it, so that
 * the list of include/cpuvox_gpu.h stays what its hosts were built against).  Error codes, cvx_context and cvx_last_error are
 * include/cpuvox_gpu.h's. */
#ifndef CPUVOX_GPU_SPREAD_H
#define CPUVOX_GPU_SPREAD_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*  * cvx_world_spread: how far it is from the seeds to every voxel of a box without passing through walls (voxlap's setfloodfill3d, in both
 * media) -- water that fills a basin from a spring (steps sideways and down, the box's top the water level, the distance the arrival time),
 * smoke that rises through rooms, fire through connected material, flow fields of flying and swimming agents, sound occlusion (path distance
 * against cvx_world_distance's straight line), the distance of an overhang to its support through SOLID.  Everything is integers: the same
 * call gives the same bytes on every device and on the host.
 *   Box and layout: cvx_world_distance's.  Size s = boxMax - boxMin > 0 per axis, every |coordinate| <= 2^30, s.x * s.y * s.z < 2^31; the box
 *     may stick out of the world or lie wholly outside it.  Voxel (x, y, z) is element ((x - boxMin.x) * s.z + (z - boxMin.z)) * s.y +
 *     (y - boxMin.y) of `out`: (X, Z, Y), y fastest.  Coordinates are LOD-0 voxels of the stored tile (a repeating world does not wrap them).
 *   Passable(v): v lies in the box and in the world on all three axes, and LOD 0 holds solid there iff medium == CVX_SPREAD_SOLID.  Nothing
 *     outside the world is passable, above dimY included: the box's top is the water level of a flood.
 *   Step: from passable v to passable v + dir(f) for a face f with bit f of stepFaces set (bits 0..5 = -X,+X,-Y,+Y,-Z,+Z, the pick's face
 *     numbers); it costs 1.  Steps are directed: 0x3F is the symmetric 6-neighbourhood, 0x37 (no +Y) water, 0x3B (no -Y) smoke; for the
 *     distance TOWARDS the seeds swap the bits of each axis pair.
 *   Distance: D(v) = the minimum, over the seeds k that lie on a passable voxel and all step paths from seed k to v, of start_k + path length,
 *     defined only where that is <= maxSteps.  A seed on a voxel that is not passable (outside the box or the world, in the other medium) is
 *     ignored, which is no error; several seeds on one voxel give the smallest start.  out[v] = D(v) where defined, CVX_SPREAD_UNREACHED for
 *     every other passable voxel, CVX_SPREAD_BLOCKED for every box voxel that is not passable.  The field is a function of the world and the
 *     arguments only: no schedule and no seed order shows.
 *   Summary (may be NULL): passable and reached voxels, the largest distance (-1: nothing reached), seedsUsed = the entries on a passable voxel,
 *     duplicates included; launches and tileVisits (relax launches made, tiles relaxed summed over them) say what the call cost and are not
 *     part of the deterministic result.
 *   Ordering as cvx_world_distance: both calls are ordered on the context's stream behind everything enqueued before them, place unplaced
 *     levels first, return when the field and the summary are complete and free their scratch before they return.  `seeds` is a host array
 *     in both; cvx_world_spread_device leaves the field in device memory (a torch tensor's data_ptr()).  outDeviceMs may be NULL.  Neither
 *     call changes the world.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued, in this order (the message names the seed where there is
 * one): NULL params / seeds / out; an empty box, a coordinate beyond 2^30, 2^31 or more voxels; a bad medium; stepFaces zero or with bits above
 * 0x3F; maxSteps outside 1 .. CVX_SPREAD_MAX_STEPS; seedCount outside 1 .. CVX_SPREAD_MAX_SEEDS; a seed start outside 0 .. maxSteps.
 * CVX_ERR_NOT_READY: LOD 0 has not been uploaded.  CVX_ERR_CAPACITY: the scratch does not fit in device memory.
 * Device memory while a call runs: 2 bytes per box voxel (the 16-bit working distances), 8 bytes per column of the box and 64 voxels of its
 * height (one passable bit per voxel), 2 bytes per tile of CVX_SPREAD_TILE_X x _Y x _Z voxels (the active flags, double-buffered), 16 bytes
 * per seed and 40 bytes of totals, each of these rounded up to 256 bytes; the host-array call adds the field itself, 4 bytes per voxel. */
enum { CVX_SPREAD_AIR = 0, CVX_SPREAD_SOLID = 1 };
#define CVX_SPREAD_UNREACHED (-1)
#define CVX_SPREAD_BLOCKED   (-2)
#define CVX_SPREAD_MAX_SEEDS 4096
#define CVX_SPREAD_MAX_STEPS 65534
/* the tile a workgroup relaxes (informative: what tileVisits counts, and the sizes at which the kernels take another path) */
#define CVX_SPREAD_TILE_X 8
#define CVX_SPREAD_TILE_Y 64
#define CVX_SPREAD_TILE_Z 8

typedef struct cvx_spread_params {   /* 40 bytes */
    int32_t boxMin[3], boxMax[3];    /* LOD-0 voxels, inclusive / exclusive */
    int32_t medium;                  /* CVX_SPREAD_* */
    int32_t stepFaces;               /* bits 0..5 = -X,+X,-Y,+Y,-Z,+Z (the pick's face numbers): the directions a step may go */
    int32_t maxSteps;                /* 1 .. CVX_SPREAD_MAX_STEPS */
    int32_t pad_;
} cvx_spread_params;

typedef struct cvx_spread_seed {     /* 16 bytes */
    int32_t voxel[3];
    int32_t start;                   /* 0 .. maxSteps: the distance the seed itself has */
} cvx_spread_seed;

typedef struct cvx_spread_summary {  /* 40 bytes */
    int64_t passable, reached;
    int32_t largestDistance;         /* -1: nothing reached */
    int32_t seedsUsed;               /* entries that lie on a passable voxel, duplicates included */
    int32_t launches, pad_;          /* relax launches made: informative, not part of the deterministic result */
    int64_t tileVisits;              /* tiles relaxed, summed over launches: informative */
} cvx_spread_summary;

int cvx_world_spread(cvx_context *ctx, const cvx_spread_params *params, const cvx_spread_seed *seeds, int seedCount,
                     int32_t *out, cvx_spread_summary *summary, float *outDeviceMs);
int cvx_world_spread_device(cvx_context *ctx, const cvx_spread_params *params, const cvx_spread_seed *seeds, int seedCount,
                            int32_t *outDevice, cvx_spread_summary *summary, float *outDeviceMs);

#ifdef __cplusplus
}
#endif
#endif
