/* cpuvox_gpu_model_draw.h -- bodies in flight drawn into the rendered frame: four entry points of libcpuvox_gpu.so, a family of their own with
 * the prefix cvxv_ (as include/cpuvox_gpu_model_pick.h has cvxq_): the lists of the cvx_, cvxc_, cvxp_ and cvxq_ entry points stay what their hosts
 * were built against.  Error codes, cvx_context, cvx_camera_data, cvx_pick_ray and cvx_last_error are include/cpuvox_gpu.h's; cvx_model and
 * cvx_model_instance are include/cpuvox_gpu_models.h's. */
#ifndef CPUVOX_GPU_MODEL_DRAW_H
#define CPUVOX_GPU_MODEL_DRAW_H

#include "cpuvox_gpu_models.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CVXV_DRAW_WORLD 1      /* flags: the uploaded world occludes the bodies */
#define CVXV_DRAW_DEPTH_TEST 2 /* flags: `depth` is also read: a pixel's ray ends at the depth the pixel holds */
#define CVXV_MAX_SIZE 8192     /* cvxv_view: width and height */

/* cvxv_models_draw / _device: what cvxq_model_pick is for a handful of rays, for every pixel of a view.  A body in flight is not in the world,
 * so neither render kernel sees it; this call writes the nearest body of every pixel -- colour, depth and which instance it is -- straight into
 * the image cvx_blit_segments left on the device (cvx_screen_device_ptr), without a snapshot, a place and a restore of the world.
 *   The rule, per pixel (x, y) of the view, x = 0 .. width - 1, y = 0 .. height - 1, row 0 the BOTTOM row as cvx_blit_segments has it; the pixel is
 *   element y * width + x of image, depth and ids (cpuvox_amd/csrc/cvx_model_draw.h, compiled for host and device from one text, every operation
 *   rounded once and in this order):
 *     1. Ray.  In doubles a_c = (dir0_c + x * dirX_c) + y * dirY_c, len = sqrt((a_0 * a_0 + a_1 * a_1) + a_2 * a_2).  The ray is the cvx_pick_ray
 *        { origin, direction_c = (float)(a_c / len), maxT }, so t is distance in voxels.  Under CVXV_DRAW_DEPTH_TEST the ray's maxT is
 *        depth[pixel] where that is smaller than the view's; a depth that is NaN or negative is a miss.  A len that is 0 or not finite is a miss.
 *        cvxv_view_rays writes exactly these rays (without the depth test); the ray of a miss by len has direction 0 and maxT -1, which every
 *        pick call reads as a miss.
 *     2. Bodies.  cvxq_model_pick's pair rule for that ray against every instance, and its ray rule: the least reported float t wins, equal
 *        floats go to the lower index.
 *     3. World, under CVXV_DRAW_WORLD.  cvx_world_pick_device's rule for the same ray with maxT = the body's reported t (the bounded rule, or the
 *        repeating one where cvx_set_world_repeat is on).  The body SHOWS iff that pick is a miss; else the pixel is OCCLUDED.  Without the flag
 *        every body found shows.
 *     4. Where a body shows: image = the model's colour word of the voxel hit (0 for a model without argb), the same word a world voxel of
 *        that colour has in the blitted image; depth = t; ids = the instance's index.  Every other pixel of the three arrays is left as it was.
 *   The summary counts pixels of the rule alone: pixelsDrawn, pixelsOccluded, and jobs = the (pixel, instance) pairs whose box the pixel's ray
 *   crosses (steps 1 .. 3 of the pair rule), counted over ALL instances: the kernel's cull is conservative and cannot show in any output.
 *   The result is a function of the arguments (and, under the flags, of the world and of depth) alone.
 * image, depth, ids: width * height elements each; any may be NULL, not all three; depth must be given under CVXV_DRAW_DEPTH_TEST.
 * models, instances: cvxc_world_contacts' (include/cpuvox_gpu_contacts.h), with its checks and limits; instance.op is not read.
 * Ordering: both calls are ordered on the context's stream behind everything enqueued before them and return when the outputs are complete.
 *   outDeviceMs (may be NULL): device time of the call.  Without CVXV_DRAW_WORLD no world is read and none need be uploaded.
 * cvxv_models_draw_device: the models' arrays, image, depth and ids are device pointers on the context's device; descriptors, instances, view
 *   and summary are host memory.
 * CVX_ERR_INVALID_ARGUMENT, checked on the host before anything is enqueued: cvxc_world_contacts' checks of models and instances; a NULL view;
 *   width or height outside 1 .. CVXV_MAX_SIZE; a maxT that is NaN or negative (+inf is allowed); an origin, dir0, dirX or dirY that is not
 *   finite; a matrix [dirX dirY dir0] that is singular (the cull inverts it); unknown flag bits; image, depth and ids all NULL; the depth test
 *   without depth.  Under CVXV_DRAW_WORLD without an uploaded world: CVX_ERR_NOT_READY, as cvx_world_pick.  CVX_ERR_CAPACITY: the scratch does
 *   not fit.  On an error the host arrays are untouched; what the device arrays hold is then unspecified.
 * Cost.  A wave per 8 x 8 pixel tile; a rectangle of pixels per instance, computed once per call, keeps the instances off the tiles they cannot
 *   reach.  Device memory while a call runs: 32 bytes a model, 96 + 16 an instance; the host call also holds the models' arrays and the three
 *   images.
 * cvxv_view_from_camera: the view of a cvx_camera_data at width x height -- the eye from PositionXZ / PositionY, dir0, dirX, dirY from the
 *   centres of pixels (0, 0), (1, 0), (0, 1) unprojected through the inverse of WorldToScreenMatrix, in doubles.  A convenience: a host with its
 *   own camera fills the struct itself.  CVX_ERR_INVALID_ARGUMENT (-1) for NULL, a size outside the limits or a singular matrix.
 * cvxv_view_rays: the rays of step 1 for the pixels [x0, x0 + w) x [y0, y0 + h) of the view, row-major in that window. */
typedef struct cvxv_view {      /* 96 bytes */
    float   origin[3];          /* the eye, in cvx_pick_ray's space */
    float   maxT;               /* far limit of every pixel's ray, >= 0, +inf allowed */
    double  dir0[3];            /* un-normalised direction through the centre of pixel (0, 0) */
    double  dirX[3];            /* added per pixel step in x */
    double  dirY[3];            /* added per pixel step in y */
    int32_t width;
    int32_t height;
} cvxv_view;

typedef struct cvxv_draw_summary { /* 32 bytes */
    int64_t pixelsDrawn;        /* a body shows */
    int64_t pixelsOccluded;     /* a body was hit but the world lies in front */
    int64_t jobs;               /* (pixel, instance) pairs whose box the ray crosses, whatever the cull */
    int64_t pad_;               /* 0 */
} cvxv_draw_summary;

int cvxv_view_from_camera(const cvx_camera_data *camera, int width, int height, float maxT, cvxv_view *out);
int cvxv_view_rays(const cvxv_view *view, int x0, int y0, int w, int h, cvx_pick_ray *rays);
int cvxv_models_draw(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                     const cvxv_view *view, uint32_t flags, uint32_t *image, float *depth, int32_t *ids, cvxv_draw_summary *summary,
                     float *outDeviceMs);
int cvxv_models_draw_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                            const cvxv_view *view, uint32_t flags, uint32_t *imageDevice, float *depthDevice, int32_t *idsDevice,
                            cvxv_draw_summary *summary, float *outDeviceMs);

#ifdef __cplusplus
}
#endif
#endif
