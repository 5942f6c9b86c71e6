/* cpuvox_gpu_models.h -- voxel models at any orientation and scale into and out of the uploaded world: five entry points of libcpuvox_gpu.so
 * (the product library exports them like those of include/cpuvox_gpu.h; they are declared here, in a header of their own that includes it, so
 * that the list of include/cpuvox_gpu.h stays what its hosts were built against).  Error codes, cvx_context, the op constants and
 * cvx_last_error are include/cpuvox_gpu.h's. */
#ifndef CPUVOX_GPU_MODELS_H
#define CPUVOX_GPU_MODELS_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*  * cvx_world_place_models: voxlap's setkv6 -- a door swung by 30 degrees, a vehicle or a character stamped for the frame, a tree library
 * scattered at random yaw and scale, debris put back tilted.  cvx_world_read_model is the way out (voxlap's meltspans): a tilted chunk of the
 * world lifted out as a model.  Everything is integer arithmetic: the same call gives the same bytes on every device and on the host.
 *   Maps.  A cvx_model_map is an affine map between voxel grids in fixed point, units of 2^-16.  The image of voxel v = (v0, v1, v2) is
 *     q_i = m[i][0] * (2 v0 + 1) + m[i][1] * (2 v1 + 1) + m[i][2] * (2 v2 + 1) + 2 t[i]   (int64),   image_i = q_i >> 17   (arithmetic: floor),
 *     the map applied to the voxel's centre, then floored.  |m| <= 2^24, |t| <= 2^46; with world dimensions and model sizes below 2^31,
 *     |q| < 2^59: nothing but int64 decides a voxel.
 *   Models.  Dense arrays in cvx_world_read_voxels' layout, (X, Z, Y), y fastest: voxel (x, y, z) is element (x * size.z + z) * size.y + y.  A
 *     voxel is SET as in cvx_world_write_voxels: solid[] != 0 when there is a mask, else argb[] != 0; argb may be NULL for a model only CARVE
 *     instances use.  size >= 1 on every axis, the product below 2^31.
 *   Place.  With R = LOD 0 before the call, for each instance in array order, every world voxel d inside [boxMin, boxMax) and inside the world
 *     is visited and s = toModel(d) taken; d is untouched when s lies outside [0, size) on any axis.  Otherwise CVX_COPY_REPLACE: R(d) = the
 *     model's voxel, air included; CVX_BRUSH_FILL: a set voxel makes R(d) solid with the model's colour; CVX_BRUSH_CARVE: a set voxel makes R(d)
 *     air; CVX_BRUSH_PAINT: a set voxel recolours R(d) if R(d) is solid.  A later instance sees what the earlier ones did.  Colour words are
 *     copied verbatim.  Sampling is nearest-voxel, with no filtering: under minification (a model drawn smaller than it is) thin features may
 *     vanish, under magnification every model voxel becomes a block.  Coordinates are LOD-0 voxels of the stored tile (a repeating world does
 *     not wrap them).
 *     The edited rectangle is the XZ bounding box of the instances' boxes clipped to the world, rounded outward to multiples of 2^levelCount
 *     and clipped to the world; LOD 1 .. levelCount (0 .. 5) are rebuilt over it; columns nothing touches are re-encoded with the builder's
 *     rule.  Every box outside the world: CVX_OK, nothing changes, *outDeviceMs = 0.  Ordering, atomicity (every error leaves the world as it
 *     was), several GPUs (every rank applies the same call to its own context), CVX_ERR_NOT_READY and CVX_ERR_CAPACITY (a column with a run or a
 *     colour index above 32767 or more than 65535 runs, the arena limits) are cvx_world_brush's.  The host call uploads the models' arrays; in
 *     cvx_world_place_models_device they are device pointers (a torch tensor's data_ptr()), read on the context's stream: the caller makes sure
 *     they are complete when it calls and leaves them alone until it returns.  The descriptor and instance arrays are host memory in both.
 *     Moving things: read the instance's box with cvx_world_read_voxels, place, render, write the box back with CVX_COPY_REPLACE.
 *   Read.  For every model voxel s the output holds the world's voxel at toWorld(s), air outside the world, in the models' layout; either
 *     array may be NULL, not both.  Ordering, streams and outDeviceMs as cvx_world_read_voxels / cvx_world_read_voxels_device.
 *   cvx_model_instance_from_matrix (pure host, no context).  forward: the row-major 3 x 4 matrix that takes model coordinates (voxel s is the
 *     cube [s, s + 1)) to world voxel coordinates.  Computed in double precision in a fixed order: the inverse by adjugate / determinant,
 *     m = llround(inverse * 65536), t = llround(inverse translation * 65536), the box as floor / ceil of the eight forward-mapped corners of
 *     [0, size), widened by one voxel and clamped to +-2^30 (conservative: a wider box gives the same world).  CVX_ERR_INVALID_ARGUMENT for a
 *     non-finite entry, |det| < 1e-12 or a result beyond the limits.  A toWorld map for cvx_world_read_model is the same rounding of `forward`
 *     itself: pass the INVERSE matrix here and take out->toModel.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued (the message names the model or the instance): NULL arrays or
 * counts outside 1 .. CVX_MODELS_MAX_MODELS / CVX_MODELS_MAX_INSTANCES, a size below 1 or a product of 2^31 or more, a model with neither
 * array, a model without argb used by an op other than CARVE, a model index out of range, a bad op, boxMin >= boxMax on an axis, a box
 * coordinate above 2^30 in magnitude, m or t beyond their limits, levelCount outside 0 .. 5; for the read also both outputs NULL.
 * Device memory while a call runs: the host call holds the models' arrays; a place adds cvx_world_brush's scratch for its rectangle, 4 more bytes
 * per column of it (the run counts), the descriptors (32 bytes a model, 128 an instance) and the rectangle's new columns. */
typedef struct cvx_model_map {      /* 64 bytes: an affine map between voxel grids, exact */
    int32_t m[3][3];                /* units of 2^-16 */
    int32_t pad_;
    int64_t t[3];                   /* units of 2^-16 */
} cvx_model_map;

typedef struct cvx_model {          /* 32 bytes */
    int32_t size[3];                /* (sx, sy, sz) >= 1, product < 2^31 */
    int32_t pad_;
    const uint32_t *argb;           /* (X, Z, Y) arrays in cvx_world_read_voxels' layout: */
    const uint8_t *solid;           /* ((x*sz + z)*sy + y) */
} cvx_model;

typedef struct cvx_model_instance { /* 96 bytes */
    cvx_model_map toModel;          /* world voxel -> model voxel */
    int32_t boxMin[3], boxMax[3];   /* the world voxels the instance may touch, [min, max) */
    int32_t model;                  /* index into the call's models */
    int32_t op;                     /* CVX_COPY_REPLACE, CVX_BRUSH_FILL, CVX_BRUSH_CARVE, CVX_BRUSH_PAINT */
} cvx_model_instance;
#define CVX_MODELS_MAX_MODELS 256
#define CVX_MODELS_MAX_INSTANCES 4096

int cvx_world_place_models(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                           int levelCount, float *outDeviceMs);
int cvx_world_place_models_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                                  int levelCount, float *outDeviceMs);
int cvx_world_read_model(cvx_context *ctx, const int32_t size[3], const cvx_model_map *toWorld, uint32_t *argb, uint8_t *solid, float *outDeviceMs);
int cvx_world_read_model_device(cvx_context *ctx, const int32_t size[3], const cvx_model_map *toWorld, uint32_t *argbDevice, uint8_t *solidDevice,
                                void *hipStream);
int cvx_model_instance_from_matrix(const double forward[12], const int32_t size[3], int model, int op, cvx_model_instance *out);

#ifdef __cplusplus
}
#endif
#endif
