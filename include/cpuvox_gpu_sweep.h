/* cpuvox_gpu_sweep.h -- how far a placed voxel model can move before it touches the uploaded world: four entry points of libcpuvox_gpu.so, a
 * family of their own with the prefix cvxs_ (beside cvxc_, cvxp_, cvxq_, cvxv_ and the host library's cvxh_): the list of every header whose
 * entry points begin with cvx_ stays what its hosts were built against.  Error codes, cvx_context, CVX_SURFACE_OUTSIDE_DEFAULT and
 * cvx_last_error are include/cpuvox_gpu.h's; cvx_model, cvx_model_instance and cvx_model_map are include/cpuvox_gpu_models.h's;
 * cvxc_contact_result and cvxc_contact_point are include/cpuvox_gpu_contacts.h's. */
#ifndef CPUVOX_GPU_SWEEP_H
#define CPUVOX_GPU_SWEEP_H

#include "cpuvox_gpu_contacts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvxs_world_sweep / _device: the question an integrator has every step (the loop of include/cpuvox_gpu_lift.h): how far can this body go
 * along this step's motion before it touches anything?  cvxc_world_contacts answers for one pose; worlds and lifted pieces are thin shells, so
 * a body that moves more than a voxel a step passes through them between two poses.  For up to CVX_MODELS_MAX_INSTANCES poses with an integer
 * motion each, one call gives per pose the first step of a fixed lattice path at which the body overlaps the world, the last free offset and
 * the cvxc_contact_result of the touching pose.  Everything is integer arithmetic: the same call gives the same bytes.
 *   Moved instance.  For an instance I and an integer offset o, I + o has boxMin + o, boxMax + o, the same model, op and toModel.m, and
 *     toModel.t[i] - (m[i][0] o[0] + m[i][1] o[1] + m[i][2] o[2]) in int64.  By the map's definition (include/cpuvox_gpu_models.h)
 *     toModel'(d) = toModel(d - o) exactly: the body of I + o is the body of I shifted by o, voxel for voxel.  cvxs_instance_moved (pure host
 *     code, no context) makes it; CVX_ERR_INVALID_ARGUMENT for a NULL argument or a result beyond cvx_world_place_models' limits (a box
 *     coordinate beyond +-2^30, |t| beyond 2^46).
 *   Path.  A motion v = (vx, vy, vz), |v_a| <= CVXS_MAX_MOTION on every axis, has n = |vx| + |vy| + |vz| unit steps.  The k-th step of axis a
 *     (k = 1 .. |v_a|) has the parameter (2 k - 1) / (2 |v_a|); the steps are taken in ascending parameter, equal parameters going to the lower
 *     axis index (x, then y, then z); fractions are compared by cross-multiplying integers.  Each step moves one voxel along its axis with the
 *     sign of v_a.  o_0 = 0, o_n = v; the path is 6-connected and monotone on every axis.  cvxs_sweep_offset (pure host code) gives o_j and the
 *     axis of step j (-1 for j = 0); CVX_ERR_INVALID_ARGUMENT for a NULL argument, a motion beyond the limit or j outside 0 .. n.
 *   Sweep.  motions holds three int32 per instance.  hit_k is the least j in 0 .. n_k for which the overlap O of cvxc_world_contacts for
 *     I_k + o_j is not empty -- Solid, the body and solidOutside are that call's own --, -1 when there is none.  An instance's answer does not
 *     depend on the other instances.  sweeps[k] is its cvxs_sweep_result.  contacts (may be NULL: the sweeps alone; pointCapacity is then 0)
 *     receives per instance exactly the cvxc_contact_result cvxc_world_contacts gives for I_k + at, and points, under a capacity, that call's
 *     point list over those moved instances.  summary (may be NULL): the call's cvxs_sweeps_summary.
 * Ordering, CVX_ERR_NOT_READY, placing the levels that were uploaded and not placed yet and never writing the arena are cvxc_world_contacts'.
 * cvxs_world_sweep_device: the models' arrays, contactsDevice (instanceCount entries) and pointsDevice (pointCapacity entries) are device
 *   pointers on the context's device; the descriptors, the instances, the motions, sweeps and the summary are host memory.
 * CVX_ERR_INVALID_ARGUMENT, checked on the host before anything is enqueued: every check of cvxc_world_contacts (contacts taking the place of
 *   results, and allowed to be NULL), motions or sweeps NULL, a capacity above 0 without contacts, a motion component beyond CVXS_MAX_MOTION,
 *   an instance for which I + v leaves the limits (every I + o_j then stays inside them: each component of o is monotone between 0 and v).
 * CVX_ERR_CAPACITY: the jobs (below) are 2^31 - 1 or more, the scratch does not fit, or cvxc_world_contacts' own.  On an error the host arrays
 *   are untouched.  outDeviceMs (may be NULL): the device time of both phases.
 * Cost.  Phase 1: a station of a motion is the stretch of its path between two horizontal steps (H + 1 of them, H = |vx| + |vz|); a job is
 *   (instance, column of its box, station), footprint * (H + 1) an instance, and a wave takes one job: per 64 voxels of the body's column one
 *   binary search of the world column under the moved voxel finds the first of the station's y steps that touches.  A fall of n voxels costs
 *   about the jobs of one contacts call, not n of them; cost grows with the horizontal part of the motion alone.  Phase 2 is one
 *   cvxc_world_contacts over the moved instances.
 * Device memory while a call runs: 96 bytes an instance, 32 a model, 4 + 16 + 4 an instance for the jobs' prefix, the stations' index and the
 *   first touching step, 16 bytes a station; the host call also holds the models' arrays, once for both phases; phase 2 adds cvxc_world_contacts'.
 * Not part of this: sweeps of one body against another, rotation during the motion, sub-voxel motion, a device-resident instance list. */
#define CVXS_MAX_MOTION 4096

typedef struct cvxs_sweep_result { /* 48 bytes */
    int32_t steps;               /* n */
    int32_t hit;                 /* the first touching step, or -1 */
    int32_t axis;                /* the axis of step `hit`; -1 when hit <= 0 */
    int32_t sign;                /* the sign of v on that axis; 0 when hit <= 0 */
    int32_t free[3];             /* o_(hit - 1); 0 when hit == 0; v when hit == -1 */
    int32_t at[3];               /* o_hit; v when hit == -1 */
    int32_t pad_[2];             /* 0 */
} cvxs_sweep_result;

typedef struct cvxs_sweeps_summary { /* 32 bytes */
    int64_t hits;                /* instances with hit >= 0 */
    int64_t startsSolid;         /* instances with hit == 0 */
    int64_t jobs;                /* the (instance, column, station) jobs of phase 1 */
    int64_t points;              /* the contact points of the moved instances, whatever the capacity; 0 without contacts */
} cvxs_sweeps_summary;

int cvxs_world_sweep(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                     const int32_t *motions, int solidOutside, cvxs_sweep_result *sweeps, cvxc_contact_result *contacts, cvxc_contact_point *points,
                     int64_t pointCapacity, cvxs_sweeps_summary *summary, float *outDeviceMs);
int cvxs_world_sweep_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                            const int32_t *motions, int solidOutside, cvxs_sweep_result *sweeps, cvxc_contact_result *contactsDevice,
                            cvxc_contact_point *pointsDevice, int64_t pointCapacity, cvxs_sweeps_summary *summary, float *outDeviceMs);
int cvxs_sweep_offset(const int32_t motion[3], int j, int32_t offset[3], int *axis);
int cvxs_instance_moved(const cvx_model_instance *in, const int32_t offset[3], cvx_model_instance *out);

#ifdef __cplusplus
}
#endif
#endif
