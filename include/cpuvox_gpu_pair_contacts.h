/* cpuvox_gpu_pair_contacts.h -- where placed voxel models touch EACH OTHER: four entry points of libcpuvox_gpu.so, a family of their own with the
 * prefix cvxp_ (as include/cpuvox_gpu_contacts.h has cvxc_ and the host library cvxh_): the list of every header whose entry points begin with
 * cvx_ stays what its hosts were built against, and the cvxc_ family stays at three.  Error codes, cvx_context and cvx_last_error are
 * include/cpuvox_gpu.h's; cvx_model, cvx_model_instance, cvx_model_map and cvx_model_instance_from_matrix (which makes the poses) are
 * include/cpuvox_gpu_models.h's. */
#ifndef CPUVOX_GPU_PAIR_CONTACTS_H
#define CPUVOX_GPU_PAIR_CONTACTS_H

#include "cpuvox_gpu_models.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CVXP_MAX_PAIRS 65536 /* cvxp_model_contacts: pairCount */

/* cvxp_model_contacts / _device: what a host that integrates rigid bodies needs every step besides cvxc_world_contacts (the loop of
 * include/cpuvox_gpu_lift.h): where two bodies in flight, neither of them in the world, overlap, and which way to push each of them out of the
 * other, for up to CVXP_MAX_PAIRS pairs of poses in one launch.  No world is read, placed or needed.  Everything is integer arithmetic.
 *   Body.  include/cpuvox_gpu_contacts.h's: for instance k, B_k is the set of world voxels d in [boxMin, boxMax) -- the box is not clipped to
 *     anything -- for which s = toModel(d) lies in [0, size) and the model's voxel s is SET (solid[] != 0 with a mask, else argb[] != 0).
 *     instance.op is not read; a model without argb is fine.  A voxel outside k's box is never in B_k, even where the map would hit a set
 *     model voxel.
 *   Pair.  `pairs` holds pairCount entries of int32_t[2], p = (a, b), both indices into `instances`, a != b.  The same pair may appear more than
 *     once, and (b, a) is a different pair from (a, b).  X_p is the intersection of the two boxes and may be empty.  origin is the per-axis
 *     maximum of the two boxMin, whether or not X_p is empty.
 *   Overlap.  O_p = B_a intersected with B_b.
 *   Faces.  For d in O_p, bit f of facesA(d) is set iff d + e_f is not in B_a, e_f the unit step through face f, faces 0..5 = -X, +X, -Y, +Y,
 *     -Z, +Z (cvx_world_surface's numbering); facesB(d) is the same test against B_b.  pushA is the sum over O_p, over the set bits f of
 *     facesB(d), of e_f: it points out of b, the way to move a.  pushB is the same over facesA: out of a, the way to move b.
 *   Contact points.  The d in O_p with (facesA | facesB) != 0.  The full list holds the points of all pairs ordered by pair ascending in the
 *     array's order, then x ascending, then z ascending, then y DESCENDING.  `points` (may be NULL iff pointCapacity = 0: results alone) receives
 *     the first min(pointCapacity, summary.points) entries; entries beyond are not written; a smaller capacity is no error.
 *   Per pair one cvxp_pair_result, per call one cvxp_pairs_summary (may be NULL).  All sums are integers: a pair's result (but for firstPoint)
 *     is a function of its two instances and their models alone, and the same call twice gives the same bytes.
 * Ordering as cvxc_world_contacts: the call is ordered on the context's stream behind everything enqueued before it and returns when the
 *   summary is on the host, so results and points -- device arrays too -- are complete at return.  It works on a context with nothing uploaded
 *   and never returns CVX_ERR_NOT_READY.  outDeviceMs (may be NULL): device time of the call.
 * cvxp_model_contacts_device: the models' arrays, resultsDevice (pairCount entries) and pointsDevice (pointCapacity entries) are device
 *   pointers (a torch tensor's data_ptr()) on the context's device, read and written on the context's stream; the descriptors, the instances,
 *   the pairs and the summary are host memory.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued (the message names the model, the instance or the pair):
 *   cvxc_world_contacts' checks of models, instances, boxes and maps; pairs NULL; pairCount outside 1 .. CVXP_MAX_PAIRS; an index outside
 *   0 .. instanceCount - 1; a == b; NULL results; a negative pointCapacity; points NULL with a capacity above 0.  CVX_ERR_CAPACITY: the
 *   (pair, column of X_p) jobs of all pairs sum to 2^31 - 1 or more (the launch itself has a fixed number of waves that take the jobs in turn:
 *   no smaller limit comes from it), a list is asked for and the call holds 2^31 or more points, or the scratch does not fit.  On an error the
 *   host arrays are untouched; what resultsDevice and pointsDevice hold is then unspecified.
 * Cost.  A wave walks its column of X_p 64 voxels a step; an X_p of more than 256 voxels of height is first cut to the part of the column where
 *   both maps can meet their models.  Side faces are evaluated only where the two bodies overlap.
 * Device memory while a call runs: 144 bytes a result (the host call), 32 bytes a model, 96 an instance, 8 a pair and 4 bytes a prefix entry, 32
 *   bytes of totals; with pointCapacity > 0 also 4 bytes per job and the scan's 8 bytes per chunk of them; the host call also holds the models'
 *   arrays and the listed points (32 bytes each). */
typedef struct cvxp_pair_result { /* 144 bytes */
    int64_t  overlap;            /* |O_p| */
    int64_t  points;             /* its entries in the full list, whatever the capacity */
    int64_t  firstPoint;         /* sum of `points` of the pairs before it */
    uint64_t sum[3];             /* sum over O_p of (d - origin), modulo 2^64 */
    int64_t  pushA[3];           /* sum over O_p, over the set bits f of facesB(d), of e_f: out of b, the way to move a */
    int64_t  pushB[3];           /* the same over facesA(d): out of a, the way to move b */
    int32_t  origin[3];          /* the per-axis maximum of the two boxMin */
    int32_t  min[3], max[3];     /* bounding box [min, max) of O_p; all 0 when O_p is empty */
    int32_t  a, b;               /* the pair, as given */
    int32_t  pad_;               /* 0 */
} cvxp_pair_result;

typedef struct cvxp_pair_point { /* 32 bytes */
    int32_t  voxel[3];
    int32_t  pair;               /* its index in `pairs` */
    int32_t  facesA;             /* bit f: the neighbour through face f is not in B_a */
    int32_t  facesB;             /* ... not in B_b */
    uint32_t argbA, argbB;       /* each model's colour word of the voxel's image, 0 for a model without argb */
} cvxp_pair_point;

typedef struct cvxp_pairs_summary { /* 32 bytes */
    int64_t touching;            /* pairs with overlap > 0 */
    int64_t overlap, points;     /* totals over the pairs, whatever the capacity */
    int64_t jobs;                /* the (pair, column of X_p) pairs walked */
} cvxp_pairs_summary;

int cvxp_model_contacts(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                        const int32_t *pairs, int pairCount, cvxp_pair_result *results, cvxp_pair_point *points, int64_t pointCapacity,
                        cvxp_pairs_summary *summary, float *outDeviceMs);
int cvxp_model_contacts_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                               const int32_t *pairs, int pairCount, cvxp_pair_result *resultsDevice, cvxp_pair_point *pointsDevice,
                               int64_t pointCapacity, cvxp_pairs_summary *summary, float *outDeviceMs);

/* cvxp_box_pairs: the broad phase.  Pure host code: no context, no device.  Lists every (a, b), a < b, whose boxes intersect once each is
 * widened by `margin` voxels on every side, in lexicographic order.  *found receives their number; `pairs` (int32_t[2] each; may be NULL iff
 * pairCapacity = 0) receives the first min(pairCapacity, *found).  Boxes that only touch (one's boxMax equals the other's boxMin, margin 0) do
 * not intersect.  CVX_ERR_INVALID_ARGUMENT: instances NULL with a count above 0, a negative count or capacity, margin outside 0 .. 2^20,
 * found NULL, pairs NULL with a capacity above 0. */
int cvxp_box_pairs(const cvx_model_instance *instances, int instanceCount, int margin, int32_t *pairs, int64_t pairCapacity, int64_t *found);

/* cvxp_pair_response: a result as a push-out of body a (which = 0: pushA) or body b (which = 1: pushB).  Pure host code.  It is
 * cvxc_contact_response's formula, in the same fixed order of double operations, with the push in the place of `normal`: centre (may be NULL)
 * the centre of the overlap, normal (may be NULL) the unit vector of the push, 0 when that is 0, depth (may be NULL) overlap / |push|.
 * CVX_ERR_INVALID_ARGUMENT: r NULL, overlap <= 0, or any other `which`. */
int cvxp_pair_response(const cvxp_pair_result *r, int which, double centre[3], double normal[3], double *depth);

#ifdef __cplusplus
}
#endif
#endif
