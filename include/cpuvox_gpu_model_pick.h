/* cpuvox_gpu_model_pick.h -- first-hit rays against placed voxel models: two entry points of libcpuvox_gpu.so, a family of their own with the
 * prefix cvxq_ (as include/cpuvox_gpu_contacts.h has cvxc_ and include/cpuvox_gpu_pair_contacts.h cvxp_): the list of every header whose entry
 * points begin with cvx_ stays what its hosts were built against, and the cvxc_ and cvxp_ families stay what they are.  Error codes, cvx_context,
 * cvx_pick_ray and cvx_last_error are include/cpuvox_gpu.h's; cvx_model, cvx_model_instance, cvx_model_map and cvx_model_instance_from_matrix
 * (which makes the poses) are include/cpuvox_gpu_models.h's. */
#ifndef CPUVOX_GPU_MODEL_PICK_H
#define CPUVOX_GPU_MODEL_PICK_H

#include "cpuvox_gpu_models.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CVXQ_PICK_MAX_RAYS 65536 /* cvxq_model_pick: rayCount */

/* cvxq_model_pick / _device: the third of "what touches a body in flight" besides cvxc_world_contacts (the world) and cvxp_model_contacts
 * (other bodies): per ray the first voxel of any placed instance that the ray enters, which instance it belongs to and which voxel of the
 * model it is.  A body in flight is not in the world, so cvx_world_pick cannot see it.
 *   Body.  include/cpuvox_gpu_contacts.h's: for instance k, B_k is the set of world voxels d in [boxMin, boxMax) -- the box is not clipped to
 *     any world -- for which s = toModel(d) lies in [0, size) and the model's voxel s is SET (solid[] != 0 with a mask, else argb[] != 0),
 *     decided by the same int64 map.  instance.op is not read; a model without argb is fine.  So "the ray hits voxel d of instance k" implies
 *     "a FILL of instance k would write d".
 *   No world is read or needed: the context supplies the stream, the scratch and the timing, and the call works before any cvx_world_upload.
 *     For "first of world or bodies" pass cvx_world_pick's t of the same ray as its maxT: a body is then reported only where it lies in front
 *     of the world's hit (or at the same t).
 *   Pair rule: the hit of a ray against instance k, a plain 3-D DDA in float64 over the instance's box, every operation rounded once and in a
 *     fixed order (cvxb::ModelPickSequential, cpuvox_amd/csrc/cvx_model_pick.h):
 *     1. o, d, maxT as doubles.  A component of o or d that is not finite (|v| < 1e30, cvx_world_pick's test) is a miss, and so is a NaN or
 *        negative maxT; +inf is allowed.
 *     2. clip as cvx_world_pick does, per axis with the slab [boxMin_a, boxMax_a]: inv_a = 1.0 / d_a, t0 / t1 = (plane - o_a) * inv_a swapped
 *        into order, tEnter = max(0, the t0's), the axis whose t0 > tEnter set it being the entry axis (ties: the lower axis), tExit =
 *        min(maxT, the t1's).  An axis with d_a == 0 and o_a outside [boxMin_a, boxMax_a) is a miss; !(tEnter <= tExit) is a miss.
 *     3. start: v_a = clamp(floor(o_a + tEnter * d_a), boxMin_a, boxMax_a - 1); face = the entry face 2 a + (d_a > 0 ? 0 : 1), or 6 when no
 *        axis set tEnter (the ray starts inside the box); t = tEnter.
 *     4. loop: v in B_k is the hit, with the current face and t.  Otherwise tNext_a = ((v_a + (d_a > 0 ? 1 : 0)) - o_a) * inv_a, +inf for
 *        d_a == 0; the axis with the least tNext is taken (ties: the lower axis, so a diagonal crossing takes two or three steps of length 0);
 *        tNext > tExit is a miss; v steps along that axis, and leaving the box is a miss; t = tNext, face = the one of the plane crossed.  A zero
 *        direction tests the origin's voxel alone.
 *     5. the reported t is (float)t + 0.0f: a zero is +0.
 *     Rays that graze a voxel's edge within rounding may resolve either way against a different rule, never differently between two runs of
 *     this one.
 *   Ray rule: among the instances that report a hit, the one with the least reported float t wins, equal floats go to the lower index.  The
 *     result is a function of the arguments alone: the same call twice gives the same bytes, and the order of the instances changes only
 *     `instance` and which of two exactly tied bodies wins.
 * Ordering: both calls are ordered on the context's stream behind everything enqueued before them and return when the hits are complete --
 *   hitsDevice too (the number of (ray, instance) jobs comes to the host in the middle of the call, so there is one synchronisation anyway).
 *   They never return CVX_ERR_NOT_READY.  outDeviceMs (may be NULL): device time of the call.
 * cvxq_model_pick_device: the models' arrays, raysDevice and hitsDevice (rayCount entries each) are device pointers (a torch tensor's
 *   data_ptr()) on the context's device, read and written on the context's stream; one device array of rays serves this call and
 *   cvx_world_pick_device.  The descriptors and the instances are host memory.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued (the message names the model or the instance):
 *   cvxc_world_contacts' checks of models, instances, boxes and maps; NULL rays or hits; rayCount outside 1 .. CVXQ_PICK_MAX_RAYS.
 *   CVX_ERR_CAPACITY: the scratch does not fit.  On an error the host arrays are untouched; what hitsDevice holds is then unspecified.
 * Cost.  A wave per (ray, instance) whose box the ray crosses walks 64 layers of the box along the ray's dominant axis a step; a wave stops
 *   where its ray already has a nearer hit.
 * Device memory while a call runs: 32 bytes a model, 96 an instance, 8 bytes a ray (its nearest key), 4 bytes per 64 (ray, instance) pairs and
 *   the scan's 8 bytes per chunk of them, 4 bytes per job (a pair whose box the ray crosses); the host call also holds the models' arrays, the
 *   rays (32 bytes each) and the hits (48 bytes each). */
typedef struct cvxq_model_hit { /* 48 bytes */
    int32_t  voxel[3];       /* the world voxel d that was hit; {-1,-1,-1} on a miss */
    int32_t  face;           /* 0..5 = -X,+X,-Y,+Y,-Z,+Z as cvx_world_pick; 6: the ray starts inside the voxel; -1: miss */
    uint32_t argb;           /* the model's colour word of modelVoxel; 0 when the model has no argb, and on a miss */
    float    t;              /* along the ray, in the direction's units; maxT on a miss */
    int32_t  instance;       /* index into the call's instances; -1 on a miss */
    int32_t  modelVoxel[3];  /* s = toModel(d): the voxel of the model to carve or paint; {-1,-1,-1} on a miss */
    int32_t  pad_[2];        /* 0 */
} cvxq_model_hit;

int cvxq_model_pick(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                    const cvx_pick_ray *rays, int rayCount, cvxq_model_hit *hits, float *outDeviceMs);
int cvxq_model_pick_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                           const cvx_pick_ray *raysDevice, int rayCount, cvxq_model_hit *hitsDevice, float *outDeviceMs);

#ifdef __cplusplus
}
#endif
#endif
