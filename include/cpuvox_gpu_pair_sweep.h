/* cpuvox_gpu_pair_sweep.h -- how far a placed voxel model can move before it touches ANOTHER placed model: two entry points of
 * libcpuvox_gpu.so, a family of their own with the prefix cvxm_ (beside cvxc_, cvxp_, cvxq_, cvxv_, cvxs_ and the host library's cvxh_): the
 * list of every other header stays what its hosts were built against.  Error codes, cvx_context and cvx_last_error are include/cpuvox_gpu.h's;
 * cvx_model, cvx_model_instance and cvx_model_map are include/cpuvox_gpu_models.h's; cvxs_sweep_result, CVXS_MAX_MOTION, cvxs_sweep_offset and
 * cvxs_instance_moved are include/cpuvox_gpu_sweep.h's; cvxp_pair_result and CVXP_MAX_PAIRS are include/cpuvox_gpu_pair_contacts.h's. */
#ifndef CPUVOX_GPU_PAIR_SWEEP_H
#define CPUVOX_GPU_PAIR_SWEEP_H

#include "cpuvox_gpu_sweep.h"
#include "cpuvox_gpu_pair_contacts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvxm_pair_sweep / _device: the last question of an integrator's step (the loop of include/cpuvox_gpu_lift.h).  cvxp_model_contacts answers
 * for one pose of two bodies; lifted pieces are thin shells, so debris that moves more than a voxel a step passes through a plate between two
 * poses and that call sees nothing at either end.  For up to CVXP_MAX_PAIRS pairs with an integer motion each, one call gives per pair the first
 * step of the motion's lattice path at which the two bodies share a voxel, the last free offset and, if asked for, the cvxp_pair_result of the
 * touching pose.  No world is read, placed or needed.  Everything is integer arithmetic: the same call gives the same bytes.
 *   Body, pair, overlap.  cvxp_model_contacts' own: B_k is the set of voxels d inside instance k's own box whose image toModel(d) is a SET
 *     voxel of its model; pairs[p] = (a, b), both indices into `instances`, a != b; the same pair may appear more than once and (b, a) is a
 *     different pair from (a, b).
 *   Motion.  `motions` holds three int32 per PAIR: the motion v of a RELATIVE TO b, |v_c| <= CVXS_MAX_MOTION on every axis.  This is a
 *     definition: b is the frame, it stays where it is, and the path is the relative motion's.  A host whose two bodies both move passes
 *     v_a - v_b.  The path o_0 .. o_n, n = |vx| + |vy| + |vz|, is cvxs_sweep_offset's and the moved instance I + o cvxs_instance_moved's, word
 *     for word (include/cpuvox_gpu_sweep.h).
 *   Sweep.  hit_p is the least j in 0 .. n_p for which B_(I_a + o_j) and B_b share a voxel -- cvxp_model_contacts' overlap > 0 for that pose --,
 *     -1 when no j does.  A pair's answer depends on its two instances, their models and its motion alone.  sweeps[p] is its
 *     cvxm_pair_sweep_result: `sweep` filled as cvxs_world_sweep fills it (steps, hit, axis, sign, free, at), then the pair as given.
 *     The hit of (a, b) under v is the hit of (b, a) under -v: the path of -v is the path of v negated, step for step.
 *   contacts (may be NULL: the sweeps alone) receives per pair the bytes cvxp_model_contacts writes to results[p] for the same `pairs` with
 *     instance a of pair p alone replaced by I_a + at_p -- the pose `at` = v when there is no hit --: a and b are the pair as given, firstPoint
 *     the running sum of `points` over the call's pairs.  No point list is part of this call: a caller that wants the points calls
 *     cvxp_model_contacts on the moved instances.
 *   summary (may be NULL): the call's cvxm_pair_sweeps_summary.
 *   Jobs.  For axis c let R_c(p) be the coordinates u of a's box range [boxMin_c, boxMax_c) for which [min(u, u + v_c), max(u, u + v_c)] meets
 *     b's [boxMin_c, boxMax_c): an interval.  Pair p has |R_x| * |R_z| jobs if R_y is not empty and none otherwise; with none its hit is -1
 *     and no device work is done for it.  A wave takes one job: a column of a's box that can come over b's box during the motion.
 * Ordering is cvxp_model_contacts': the call is ordered on the context's stream behind everything enqueued before it and returns when its
 *   answers are on the host, device arrays complete too.  It works on a context with nothing uploaded and never returns CVX_ERR_NOT_READY.
 *   outDeviceMs (may be NULL): the device time of both phases.
 * cvxm_pair_sweep_device: the models' arrays and contactsDevice (pairCount entries) are device pointers on the context's device; the
 *   descriptors, the instances, the pairs, the motions, sweeps and the summary are host memory.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued: cvxp_model_contacts' own checks of models, instances and pairs
 *   (pairCount outside 1 .. CVXP_MAX_PAIRS among them), motions or sweeps NULL, a motion component beyond CVXS_MAX_MOTION, a pair for which
 *   I_a + v leaves cvx_world_place_models' limits (every I_a + o_j then stays inside them).
 * CVX_ERR_CAPACITY: the jobs are 2^31 - 1 or more, or the scratch does not fit.  On an error the host arrays are untouched.
 * Cost.  Phase 1: a wave holds 64 voxels of a's column and walks the poses at which that column lies inside b's box on x and z and its body
 *   voxels can reach b's y range, a ballot a pose, up to the first pose that touches.  Phase 2 (with contacts) is one cvxp_model_contacts
 *   launch over the touching poses.
 * Device memory while a call runs: 32 bytes a model, 96 an instance, 8 + 12 + 4 + 4 a pair for the pairs, the motions, the jobs' prefix and the
 *   first touching step; the host call also holds the models' arrays, once for both phases; phase 2 adds cvxp_model_contacts' and 96 + 4 bytes
 *   a pair.
 * Not part of this: rotation during the motion, sub-voxel motion, a point list, a swept broad phase (cvxp_box_pairs with margin = the largest
 *   motion component serves), a device-resident instance list. */
typedef struct cvxm_pair_sweep_result { /* 56 bytes */
    cvxs_sweep_result sweep;     /* of a relative to b, as cvxs_world_sweep fills it */
    int32_t a, b;                /* the pair, as given */
} cvxm_pair_sweep_result;

typedef struct cvxm_pair_sweeps_summary { /* 32 bytes */
    int64_t hits;                /* pairs with hit >= 0 */
    int64_t startsSolid;         /* pairs with hit == 0 */
    int64_t jobs;                /* the (pair, column) jobs of phase 1 */
    int64_t pad_;                /* 0 */
} cvxm_pair_sweeps_summary;

int cvxm_pair_sweep(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                    const int32_t *pairs, const int32_t *motions, int pairCount, cvxm_pair_sweep_result *sweeps, cvxp_pair_result *contacts,
                    cvxm_pair_sweeps_summary *summary, float *outDeviceMs);
int cvxm_pair_sweep_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                           const int32_t *pairs, const int32_t *motions, int pairCount, cvxm_pair_sweep_result *sweeps,
                           cvxp_pair_result *contactsDevice, cvxm_pair_sweeps_summary *summary, float *outDeviceMs);

#ifdef __cplusplus
}
#endif
#endif
