// cvx_model_draw.hip -- libcpuvox_gpu.so, placed voxel models drawn into a view (cvxv_models_draw, cvxv_models_draw_device) and the two host
// calls that make a view and its rays.  See include/cpuvox_gpu_model_draw.h for the contract and cvx_model_draw.h for the rules.
//
//   1. rects  a thread per instance: the rectangle of pixels whose rays can reach the instance's box (cvxb::ModelDrawRectOf), once per call.
//   2. tiles  a WAVE per 8 x 8 pixel tile, lane l = pixel (l & 7, l >> 3), its ray in vector registers (cvxb::ModelDrawRayOf).  The wave tests
//             64 rectangles a step against its tile, one ballot; the set bits of the ballot ARE the tile's list of that step, in instance order,
//             in a scalar register pair: nothing is written to LDS and the list has no largest size.  For each listed instance the body goes into
//             scalar registers (cvxb::ModelPickBodyOf through readfirstlane, as pick_walk_kernel has it) and every lane clips and walks its own
//             ray (cvxb::ModelDrawBody: the pair rule a voxel at a time, the lane-per-job walk) into its own key; a lane leaves out the walk of
//             a box it enters behind its key.  Lanes with a key run the world pick (kWorld) and store colour, depth and index with plain
//             vector stores; the three counts come from ballots and go into the summary with one set of 64-bit atomic adds per wave.
// No LDS, no scratch memory (the compiler's figures: profiles/model_draw.md).  Host models and the three images are staged by
// cvxi::ModelStaging (cvx_model_call.h).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <vector>

#include "cvx_model_call.h"
#include "cvx_model_draw.h"

using cvxi::Fail;

namespace cvxmodeldraw {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr int kTile = cvxb::kModelDrawTile;
static_assert(kTile * kTile == CVX_WAVE, "a wave is a tile");
static_assert(sizeof(cvxv_view) == 96 && sizeof(cvxv_draw_summary) == 32 && sizeof(cvxb::ModelDrawRect) == 16, "the records of include/cpuvox_gpu_model_draw.h");
static_assert(((uint64_t)CVXV_MAX_SIZE / kTile) * (CVXV_MAX_SIZE / kTile) / kWaves < (1ull << 31), "the tiles fit a grid");

struct Args {
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	cvxb::ModelDrawRect *rects;          // one per instance
	int instanceCount;
	uint32_t flags;
	cvxv_view view;
	cvxb::ModelDrawCull cull;
	uint32_t tilesX, tiles;
	uint32_t *image;
	float *depth;
	int32_t *ids;
	unsigned long long *summary;         // pixelsDrawn, pixelsOccluded, jobs, 0
	cvxb::PickWorld world;               // kWorld only
};

__global__ __launch_bounds__(kThreads) void draw_rects_kernel(Args A)
{
	const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
	if (k >= A.instanceCount) { return; }
	const cvx_model_instance &I = A.instances[k];
	A.rects[k] = cvxb::ModelDrawRectOf(A.cull, A.view.origin, I.boxMin, I.boxMax, A.view.width, A.view.height);
}

template <bool kWorld> __global__ __launch_bounds__(kThreads) void draw_tiles_kernel(Args A)
{
	const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / CVX_WAVE));
	if (tile >= A.tiles) { return; }
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	const int tx = (int)(tile % A.tilesX) * kTile, ty = (int)(tile / A.tilesX) * kTile;
	const int x = tx + (lane & (kTile - 1)), y = ty + lane / kTile;
	const size_t pixel = (size_t)y * (size_t)A.view.width + (size_t)x;
	cvx_pick_ray ray;
	bool live = x < A.view.width && y < A.view.height;
	live = cvxb::ModelDrawRayOf(A.view, x, y, &ray) && live;
	if ((A.flags & CVXV_DRAW_DEPTH_TEST) && live) { live = cvxb::ModelDrawDepthLimit(A.depth[pixel], &ray.maxT); }

	uint64_t key = cvxb::kModelPickNoKey;
	uint32_t argb = 0u;
	unsigned long long jobs = 0ull;
	for (int base = 0; base < A.instanceCount; base += CVX_WAVE) {
		const int mine = base + lane;
		bool meets = false;
		if (mine < A.instanceCount) { meets = cvxb::ModelDrawRectMeetsTile(A.rects[mine], tx, ty); }
		uint64_t listed = __ballot(meets);
		while (listed != 0ull) {
			const int k = base + (int)__builtin_ctzll(listed);
			listed &= listed - 1ull;
			const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(cvxi::WaveUniform{}, A.models, A.instances[k]);
			const bool job = live && cvxb::ModelDrawBody(B, k, ray, true, &key, &argb);
			jobs += (unsigned long long)__popcll(__ballot(job));
		}
	}

	const bool hit = key != cvxb::kModelPickNoKey;
	const float t = cvxb::ModelDrawKeyT(key);
	bool shows = hit;
	if (kWorld) {
		if (hit) { shows = !cvxb::ModelDrawOccluded(A.world, ray, t); }
	}
	if (shows) {
		if (A.image) { A.image[pixel] = argb; }
		if (A.depth) { A.depth[pixel] = t; }
		if (A.ids) { A.ids[pixel] = (int32_t)(uint32_t)key; }
	}
	const unsigned long long drawn = (unsigned long long)__popcll(__ballot(shows)), occluded = (unsigned long long)__popcll(__ballot(hit && !shows));
	if (lane == 0) {
		if (drawn) { atomicAdd(&A.summary[0], drawn); }
		if (occluded) { atomicAdd(&A.summary[1], occluded); }
		if (jobs) { atomicAdd(&A.summary[2], jobs); }
	}
}

// LOD 0 of the arena as cvx_world_pick reads it (cvx_brush.hip's PickWorldOf)
static cvxb::PickWorld PickWorldOf(const cvx_context *ctx)
{
	const cvxb::CopyWorld W = cvxi::WorldOf(ctx);
	cvxb::PickWorld P;
	P.records = W.records;
	P.runs = W.runs;
	P.colours = reinterpret_cast<const uint8_t *>(W.colourSlots);
	P.rowShift = W.rowShift;
	P.colorShift = W.colorShift;
	P.dimX = W.dimX;
	P.dimY = W.dimY;
	P.dimZ = W.dimZ;
	P.repeat = ctx->worldRepeat;
	return P;
}

// Both calls: `device` says where the models' arrays, image, depth and ids live.
static int ModelsDraw(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                      const cvxv_view *view, uint32_t flags, uint32_t *image, float *depth, int32_t *ids, cvxv_draw_summary *summary, bool device, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	Args A{};
	if (!cvxb::ModelDrawValidate(models, modelCount, instances, instanceCount, view, flags, image, depth, ids, &A.cull, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	const bool world = (flags & CVXV_DRAW_WORLD) != 0;
	if (world && !ctx->levelSet[0]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD 0 has not been uploaded"); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	if (world) {
		int rc = cvxi::SyncWorld(ctx);
		if (rc == CVX_OK && ctx->worldRepeat) { rc = cvxi::ValidateRepeat(ctx); }
		if (rc != CVX_OK) { return rc; }
		A.world = PickWorldOf(ctx);
	}

	const size_t pixels = (size_t)view->width * (size_t)view->height;
	// (these outlive D: freeing the device blocks waits for a copy still under way)
	std::vector<uint32_t> backImage(!device && image ? pixels : 0);
	std::vector<float> backDepth(!device && depth ? pixels : 0);
	std::vector<int32_t> backIds(!device && ids ? pixels : 0);
	unsigned long long totals[4] = {};
	cvxi::ModelStaging staging(models, modelCount, device);
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	// host images: behind the models' arrays, in and out (the pixels nothing shows in keep what they held)
	const size_t oImage = !device && image ? staging.Add(pixels * 4, image) : 0, oDepth = !device && depth ? staging.Add(pixels * 4, depth) : 0,
	             oIds = !device && ids ? staging.Add(pixels * 4, ids) : 0;
	hipError_t e = staging.Allocate(D);
	if (e != hipSuccess) { return D.Fail(e); }
	cvxi::ScratchLayout carve;
	const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance);
	const size_t oTotals = carve(sizeof totals), oModels = carve(modelsBytes), oInstances = carve(instancesBytes),
	             oRects = carve((size_t)instanceCount * sizeof(cvxb::ModelDrawRect));
	e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = staging.Enqueue(ctx->stream); }
	if (e == hipSuccess) { e = hipMemsetAsync(scratch + oTotals, 0, sizeof totals, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
		A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
		A.rects = reinterpret_cast<cvxb::ModelDrawRect *>(scratch + oRects);
		A.instanceCount = instanceCount;
		A.flags = flags;
		A.view = *view;
		A.tilesX = (uint32_t)((view->width + kTile - 1) / kTile);
		A.tiles = A.tilesX * (uint32_t)((view->height + kTile - 1) / kTile);
		A.image = !image ? nullptr : (device ? image : reinterpret_cast<uint32_t *>(staging.block + oImage));
		A.depth = !depth ? nullptr : (device ? depth : reinterpret_cast<float *>(staging.block + oDepth));
		A.ids = !ids ? nullptr : (device ? ids : reinterpret_cast<int32_t *>(staging.block + oIds));
		A.summary = reinterpret_cast<unsigned long long *>(scratch + oTotals);
		hipLaunchKernelGGL(draw_rects_kernel, dim3(cvxi::Grid((size_t)instanceCount, kThreads)), dim3(kThreads), 0, ctx->stream, A);
		if (world) {
			hipLaunchKernelGGL(draw_tiles_kernel<true>, dim3(cvxi::Grid((size_t)A.tiles, kWaves)), dim3(kThreads), 0, ctx->stream, A);
		} else {
			hipLaunchKernelGGL(draw_tiles_kernel<false>, dim3(cvxi::Grid((size_t)A.tiles, kWaves)), dim3(kThreads), 0, ctx->stream, A);
		}
		e = hipGetLastError();
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(totals, A.summary, sizeof totals, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !backImage.empty()) { e = hipMemcpyAsync(backImage.data(), A.image, pixels * 4, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !backDepth.empty()) { e = hipMemcpyAsync(backDepth.data(), A.depth, pixels * 4, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !backIds.empty()) { e = hipMemcpyAsync(backIds.data(), A.ids, pixels * 4, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	// (nothing is handed out to the host before the call can no longer fail)
	if (!backImage.empty()) { std::memcpy(image, backImage.data(), pixels * 4); }
	if (!backDepth.empty()) { std::memcpy(depth, backDepth.data(), pixels * 4); }
	if (!backIds.empty()) { std::memcpy(ids, backIds.data(), pixels * 4); }
	if (summary) { *summary = cvxv_draw_summary{ (int64_t)totals[0], (int64_t)totals[1], (int64_t)totals[2], 0 }; }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxmodeldraw

extern "C" {

int cvxv_view_from_camera(const cvx_camera_data *camera, int width, int height, float maxT, cvxv_view *out)
{
	return cvxb::ModelDrawViewFromCamera(camera, width, height, maxT, out) == 0 ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

int cvxv_view_rays(const cvxv_view *view, int x0, int y0, int w, int h, cvx_pick_ray *rays)
{
	return cvxb::ModelDrawRays(view, x0, y0, w, h, rays) == 0 ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

int cvxv_models_draw(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvxv_view *view,
                     uint32_t flags, uint32_t *image, float *depth, int32_t *ids, cvxv_draw_summary *summary, float *outDeviceMs)
{
	return cvxmodeldraw::ModelsDraw(ctx, "cvxv_models_draw", models, modelCount, instances, instanceCount, view, flags, image, depth, ids, summary, false, outDeviceMs);
}

int cvxv_models_draw_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvxv_view *view,
                            uint32_t flags, uint32_t *imageDevice, float *depthDevice, int32_t *idsDevice, cvxv_draw_summary *summary, float *outDeviceMs)
{
	return cvxmodeldraw::ModelsDraw(ctx, "cvxv_models_draw_device", models, modelCount, instances, instanceCount, view, flags, imageDevice, depthDevice, idsDevice, summary,
	                                true, outDeviceMs);
}

} // extern "C"
