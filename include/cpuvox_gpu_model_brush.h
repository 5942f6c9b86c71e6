/* cpuvox_gpu_model_brush.h -- world-space brush strokes that carve and paint placed voxel models: three entry points of libcpuvox_gpu.so, a
 * family of their own with the prefix cvxd_ (beside cvxc_, cvxp_, cvxq_, cvxv_, cvxs_, cvxm_ and the host library's cvxh_): the list of every
 * other header stays what its hosts were built against.  Error codes, cvx_context, cvx_brush_stroke, the CVX_BRUSH_* ops, the CVX_SHAPE_*
 * shapes, CVX_BRUSH_MAX_STROKES and cvx_last_error are include/cpuvox_gpu.h's; cvx_model, cvx_model_instance and cvx_model_map are
 * include/cpuvox_gpu_models.h's. */
#ifndef CPUVOX_GPU_MODEL_BRUSH_H
#define CPUVOX_GPU_MODEL_BRUSH_H

#include "cpuvox_gpu_models.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvxd_models_brush / _device: damage to the bodies in flight (the loop of include/cpuvox_gpu_lift.h).  cvx_world_brush edits the world and
 * leaves every lifted body untouched, because a lifted body is not in the world.  This call takes the same strokes, in world coordinates, and
 * carves or paints the voxels of the MODELS through the instances that place them, in the models' own arrays, and returns per model the mass
 * sums of what is left.  No world is read, placed or needed.  Everything is integer arithmetic: the same call gives the same bytes.
 *   Body.  cvxc_world_contacts' own: B_k is the set of voxels d inside instance k's own, unclipped box whose image s = toModel_k(d) lies in the
 *     model and is SET (solid[s] != 0 where the model has a mask, argb[s] != 0 otherwise).  instance.op is not read.  A body may lie at negative
 *     coordinates.
 *   Strokes.  cvx_brush_stroke with the four shapes and the voxel predicates of include/cpuvox_gpu.h, clipped to nothing.  The ops are
 *     CVX_BRUSH_CARVE and CVX_BRUSH_PAINT only: growing a body is not part of this, and a PAINT with argb == 0 would unset the voxels of a
 *     model without a mask.
 *   Touch.  Stroke j touches model voxel (g, s) iff some instance k with model == g has a d in B_k inside the shape of j with toModel_k(d) = s.
 *     EVERY instance of a model contributes: a model shared by several instances changes for all of them.  A host that wants one body damaged
 *     alone gives it a model of its own.
 *   Effect, the sequential form.  The strokes apply in array order, a later stroke sees what the earlier ones did (B_k shrinks as voxels are
 *     carved).  CARVE unsets the touched voxels: solid[s] = 0 where there is a mask, argb[s] = 0 where there is an argb array.  PAINT sets
 *     argb[s] = stroke.argb of the touched voxels (they are set).  A model without argb ignores PAINT.
 *   Effect, the order-free form.  Touch taken with B_k as it is BEFORE the call: a voxel ends unset iff it was unset or any CARVE touches it;
 *     otherwise it takes the colour of the touching PAINT with the highest index, or keeps its own.  The two forms are EQUAL: no op sets a
 *     voxel, so a voxel that an earlier stroke carved stays unset whatever follows, and of the PAINTs of a voxel that no CARVE touches the
 *     last one wins.  The device evaluates the second.
 *     Under a map that is not one-to-one a d outside every stroke leaves the body when a sibling d' with the same image is carved: the model
 *     voxel is what changes.  Model voxels that no d of any instance maps to keep their bytes.
 *   modelResults[g], one per model, touched or not: the cvxd_model_result of model g after the call.
 *   instanceResults (may be NULL), one per instance: which bodies were hit, counted over B_k as it is before the call.
 *   summary (may be NULL): the call's cvxd_brush_summary.
 *   Jobs.  An instance whose box meets the box around all strokes' footprints has one job per column (x, z) of its box; the others have none.
 * Ordering is cvxp_model_contacts': the call is ordered on the context's stream behind everything enqueued before it and returns when the
 *   results are on the host; the models' arrays, device arrays too, are then complete.  It works on a context with nothing uploaded and never
 *   returns CVX_ERR_NOT_READY.  outDeviceMs (may be NULL): the device time.
 * cvxd_models_brush: the models' arrays are host memory, WRITTEN IN PLACE although cvx_model declares them const: the descriptors say where
 *   they are, the call owns them until it returns.
 * cvxd_models_brush_device: the models' arrays are device pointers on the context's device, written in place; the descriptors, the instances,
 *   the strokes and all results are host memory.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued: cvxc_world_contacts' checks of models, instances, boxes and
 *   maps; cvx_world_brush' checks of the stroke count (1 .. CVX_BRUSH_MAX_STROKES) and the shapes; a CVX_BRUSH_FILL; a PAINT with argb == 0;
 *   modelResults NULL; two models whose arrays overlap in memory.
 * CVX_ERR_CAPACITY: the jobs are 2^31 - 1 or more, or the scratch does not fit.
 * On an error the host arrays are untouched, the models' arrays too in the host call; in the device call they are untouched if the error is
 *   found before the launch, which every argument error is.
 * Device memory while a call runs: 32 bytes a model, 96 an instance, 40 a stroke, 128 a model and 16 an instance for the results, 4 an
 *   instance and 4 + 8 a model for the prefixes, strokeCount / 8 bytes (rounded up to 8) an instance for the culled lists and FOUR BYTES PER
 *   MODEL VOXEL for the keys; the host call also holds the models' arrays.
 * Cost.  Three passes without a synchronisation in between: a lane per (instance, stroke) for the cull, a wave per job that holds 64 voxels of
 *   the column and walks the instance's culled strokes, and one pass over every voxel of every model, touched or not, which is what gives the
 *   results of all models.
 * Not part of this: FILL; splitting a body that a carve has cut in two (place it into a scratch world and cvx_world_lift_pieces it);
 *   shrinking a model to its new box; a device-resident instance list. */
typedef struct cvxd_model_result { /* 128 bytes */
    int64_t  voxels;      /* set voxels after the call */
    int64_t  carved;      /* voxels unset by this call */
    int64_t  painted;     /* set voxels after the call that a PAINT touched, whatever colour they had; 0 for a model without argb */
    uint64_t sum[3];      /* cvx_lifted_piece's sums with p = s over the set voxels after the call, modulo 2^64 */
    uint64_t moment[6];   /* p_x^2, p_y^2, p_z^2, p_x p_y, p_y p_z, p_z p_x */
    int32_t  min[3];      /* the tight box [min, max) of the set voxels after the call in model coordinates; all 0 when none is left */
    int32_t  max[3];
    int32_t  pad_[2];     /* 0 */
} cvxd_model_result;

typedef struct cvxd_instance_result { /* 16 bytes */
    int64_t carved;       /* the d of B_k before the call that lie inside at least one CARVE stroke */
    int64_t painted;      /* the d of B_k not so counted that lie inside at least one PAINT stroke; 0 for a model without argb */
} cvxd_instance_result;

typedef struct cvxd_brush_summary { /* 32 bytes */
    int64_t carved;       /* the sum of the models' carved */
    int64_t painted;      /* the sum of the models' painted */
    int64_t models;       /* models with carved + painted > 0 */
    int64_t jobs;         /* the (instance, column) jobs of the call */
} cvxd_brush_summary;

int cvxd_models_brush(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                      const cvx_brush_stroke *strokes, int strokeCount, cvxd_model_result *modelResults,
                      cvxd_instance_result *instanceResults, cvxd_brush_summary *summary, float *outDeviceMs);
int cvxd_models_brush_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                             const cvx_brush_stroke *strokes, int strokeCount, cvxd_model_result *modelResults,
                             cvxd_instance_result *instanceResults, cvxd_brush_summary *summary, float *outDeviceMs);

/* cvxd_model_mass: mass properties of a model after the call, made of unit cubes of unit mass.  Pure host code: no context, no device.  It is
 * cvx_lifted_piece_mass (include/cpuvox_gpu_lift.h) applied to { voxels, min = 0, sum, moment }, word for word: centre (may be NULL) and
 * inertia (may be NULL) in MODEL coordinates, a model voxel s being the cube [s, s + 1).
 * CVX_ERR_INVALID_ARGUMENT: r NULL, or voxels <= 0. */
int cvxd_model_mass(const cvxd_model_result *r, double centre[3], double inertia[6]);

#ifdef __cplusplus
}
#endif
#endif
