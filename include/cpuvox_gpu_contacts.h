/* cpuvox_gpu_contacts.h -- where placed voxel models touch the uploaded world: three entry points of libcpuvox_gpu.so, a family of their own with
 * the prefix cvxc_ (as the host library has cvxh_): the list of every header whose entry points begin with cvx_ stays what its hosts were built
 * against.  Error codes, cvx_context, CVX_SURFACE_OUTSIDE_DEFAULT and cvx_last_error are include/cpuvox_gpu.h's; cvx_model, cvx_model_instance,
 * cvx_model_map and cvx_model_instance_from_matrix (which makes the poses) are include/cpuvox_gpu_models.h's. */
#ifndef CPUVOX_GPU_CONTACTS_H
#define CPUVOX_GPU_CONTACTS_H

#include "cpuvox_gpu_models.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvxc_world_contacts / _device: what a host that integrates rigid bodies needs every step (the loop of include/cpuvox_gpu_lift.h): where a body
 * in a given pose touches the world and which way to push it out, for up to CVX_MODELS_MAX_INSTANCES poses in one launch.  The contact set of an
 * instance is exactly the voxels a CVX_BRUSH_FILL of that instance (cvx_world_place_models) would write that are already solid, decided by the
 * same int64 map: "no overlap reported" and "the stamp overwrites nothing" are one statement.  Everything is integer arithmetic.
 *   Solid(v).  cvx_world_distance's rule: inside the stored tile what the arena holds at LOD 0; outside it v is solid iff it lies beyond the
 *     world on the side of a face f whose bit of solidOutside is set, faces 0..5 = -X, +X, -Y, +Y, -Z, +Z (CVX_SURFACE_OUTSIDE_DEFAULT: an
 *     infinite ground below y = 0).  A repeating world does not wrap coordinates.
 *   Body.  For instance k, B_k is the set of world voxels d in [boxMin, boxMax) -- the box is NOT clipped to the world -- for which
 *     s = toModel(d) lies in [0, size) and the model's voxel s is SET (solid[] != 0 with a mask, else argb[] != 0).  instance.op is not read; a
 *     model without argb is fine.
 *   Overlap.  O_k = { d in B_k : Solid(d) }.
 *   Faces.  For d in O_k, bit f of faces(d) is set iff !Solid(d + e_f), e_f the unit step through face f.
 *   Contact points.  The d in O_k with faces(d) != 0.  The full list holds the points of all instances ordered by instance ascending, then x
 *     ascending, then z ascending, then y DESCENDING (cvx_world_surface's order).  `points` (may be NULL iff pointCapacity = 0: results alone)
 *     receives the first min(pointCapacity, summary.points) entries; entries beyond are not written; a smaller capacity is no error.
 *   Per instance one cvxc_contact_result, per call one cvxc_contacts_summary (may be NULL).  All sums are integers: the result is a function of
 *     the world and the arguments, an instance's result does not depend on the other instances, and the same call twice gives the same bytes.
 * Ordering as cvx_world_surface / cvx_world_surface_device: the call is ordered on the context's stream behind everything enqueued before it,
 *   places levels that were uploaded and not placed yet, and returns when the summary is on the host, so results and points -- device arrays
 *   too -- are complete at return.  It never writes the arena.  outDeviceMs (may be NULL): device time of the call.
 * cvxc_world_contacts_device: the models' arrays, resultsDevice (instanceCount entries) and pointsDevice (pointCapacity entries) are device
 *   pointers (a torch tensor's data_ptr()) on the context's device, read and written on the context's stream; the descriptors, the instances and
 *   the summary are host memory.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued (the message names the model or the instance):
 *   cvx_world_place_models' checks of models, instances, boxes and maps (without its op and levelCount checks), solidOutside bits above 0x3F,
 *   NULL results, a negative pointCapacity, points NULL with a capacity above 0.  CVX_ERR_NOT_READY: LOD 0 not uploaded.  CVX_ERR_CAPACITY: the
 *   (instance, column of its box) pairs of all boxes sum to 2^31 - 1 or more (the launch itself has a fixed number of waves that take the pairs in
 *   turn: no smaller limit comes from it), a list is asked for and the contacts hold 2^31 or more points, or the scratch does not fit.  On an
 *   error the host arrays are untouched; what resultsDevice and pointsDevice hold is then unspecified (the points limit is known only after
 *   they were written).
 * Cost.  A wave walks its column of a box 64 voxels a step; a box of more than 256 voxels of height is first cut to the part of the column where
 *   the map can meet the model, so a call's work grows with the bodies' voxels and the boxes' footprints, not with the boxes' heights: a box
 *   far taller than its body gives the same answer (but for origin and the sums relative to it) at the same cost.
 * Device memory while a call runs: 120 bytes a result (the host call), 32 bytes a model, 96 an instance and 4 bytes a prefix entry, 32 bytes of
 *   totals; with pointCapacity > 0 also 4 bytes per pair and the scan's 8 bytes per chunk of them; the host call also holds the models' arrays
 *   and the listed points (24 bytes each). */
typedef struct cvxc_contact_result { /* 120 bytes */
    int64_t  voxels;             /* |B_k| */
    int64_t  overlap;            /* |O_k| */
    int64_t  points;             /* its entries in the full list, whatever the capacity */
    int64_t  firstPoint;         /* sum of `points` of the instances before it */
    uint64_t sum[3];             /* sum over O_k of (d - boxMin), modulo 2^64 */
    int64_t  normal[3];          /* sum over O_k, over the set bits f of faces(d), of e_f: out of the world's solid, the way to push the body */
    int32_t  origin[3];          /* the instance's boxMin */
    int32_t  min[3], max[3];     /* bounding box [min, max) of O_k; all 0 when O_k is empty */
    int32_t  pad_;               /* 0 */
} cvxc_contact_result;

typedef struct cvxc_contact_point { /* 24 bytes */
    int32_t  voxel[3];
    int32_t  instance;
    int32_t  faces;              /* bit f: the neighbour through face f is not solid */
    uint32_t argb;               /* the arena's colour word of the world voxel, 0 outside the world */
} cvxc_contact_point;

typedef struct cvxc_contacts_summary { /* 32 bytes */
    int64_t touching;            /* instances with overlap > 0 */
    int64_t overlap, points, voxels; /* totals over the instances, whatever the capacity */
} cvxc_contacts_summary;

int cvxc_world_contacts(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                        int solidOutside, cvxc_contact_result *results, cvxc_contact_point *points, int64_t pointCapacity,
                        cvxc_contacts_summary *summary, float *outDeviceMs);
int cvxc_world_contacts_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                               int solidOutside, cvxc_contact_result *resultsDevice, cvxc_contact_point *pointsDevice, int64_t pointCapacity,
                               cvxc_contacts_summary *summary, float *outDeviceMs);

/* cvxc_contact_response: a result as a push-out.  Pure host code: no context, no device.  centre (may be NULL): the centre of the overlap in
 * world coordinates, a voxel v being the cube [v, v + 1).  normal (may be NULL): the unit vector of `normal`, 0 when that is 0.  depth (may be
 * NULL): overlap / |normal|, 0 when normal is 0: a body sunk k layers into flat ground gives k.
 * Computed in double in this order, every operation rounded once (no contraction):
 *     n = (double)overlap;  centre[a] = ((double)origin[a] + (double)sum[a] / n) + 0.5;  g_a = (double)normal[a]          a = x, y, z
 *     len = sqrt((g_x * g_x + g_y * g_y) + g_z * g_z);  normal[a] = len > 0 ? g_a / len : 0;  *depth = len > 0 ? n / len : 0
 * CVX_ERR_INVALID_ARGUMENT: r NULL, or overlap <= 0. */
int cvxc_contact_response(const cvxc_contact_result *r, double centre[3], double normal[3], double *depth);

#ifdef __cplusplus
}
#endif
#endif
