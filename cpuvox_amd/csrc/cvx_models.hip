// cvx_models.hip -- libcpuvox_gpu.so, voxel models at any orientation and scale into and out of the device-resident world
// (cvx_world_place_models[_device], cvx_world_read_model[_device], cvx_model_instance_from_matrix).  See include/cpuvox_gpu_models.h for the
// contract and cvx_models.h for the rules.
//
// A read is one kernel, a thread per element of the arrays, y fastest, as cvx_dense.hip's: each lane maps its model voxel into the world
// (cvxb::ModelMapApply, int64) and finds the voxel with a binary search of that column's runs.
// A place is the dense write with a per-voxel rule in front of the arrays; steps 2 .. 4 are cvxi::ColumnEdit (cvx_edit.hip), the count and the
// write kernel what it launches, a WAVE per LOD-0 column of the rounded rectangle:
//   0. cull   (both kernels begin with it): the wave walks the call's instances 64 at a time, a lane per instance (their boxes clipped to the
//             world, 32 bytes each: one contiguous load), and lists those whose box covers its column, in instance order, in LDS (a ballot and
//             the count of the kept lanes below); a reduction gives the union [lo, hi) of their y ranges
//   1. count  the column top-down, 64 voxels per step (cvx_dense.h's steps); every lane evaluates its voxel (cvxb::ModelsLaneVoxel: the listed
//             instances in order, the map's column part on the scalar side, three 64-bit multiply-adds, the bounds test and one gather per lane
//             and instance); steps wholly outside [lo, hi) and the arena's runs are taken in one go (cvxb::DenseAirSteps)
//   2. the counts are prefix-scanned into element offsets; ONE copy brings the total and the flag to the host
//   3. write  (same waves): the same walk, writing the runs and colours into their slots (mbcnt)
//   4. cvxi::EditFromDevice: the blob goes through cvx_world_edit's machinery (records, tails, growth, LOD 1 .. levelCount) unchanged.
// Nothing in the arena is written before step 4, so a rejected call leaves the world as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cvx_model_call.h"
#include "cvx_models.h"

using cvxi::Fail;

namespace cvxmodels {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE; // the one launch width of both place kernels: bounds, grid and the lists' size

struct ReadArgs {
	cvxb::CopyWorld W;
	cvx_model_map toWorld;
	int32_t size[3];
	uint32_t n; // elements
	uint32_t *argb;
	uint8_t *solid;
};

__global__ __launch_bounds__(kThreads) void model_read_kernel(ReadArgs A)
{
	const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t sizeY = (uint32_t)A.size[1], sizeZ = (uint32_t)A.size[2];
	const uint32_t column = i / sizeY, y = i - column * sizeY;
	const uint32_t x = column / sizeZ, z = column - x * sizeZ;
	const cvxb::Voxel v = cvxb::ModelReadVoxel(A.W, A.toWorld, x, y, z);
	if (A.argb) { A.argb[i] = v.argb; }
	if (A.solid) { A.solid[i] = v.solid ? 1 : 0; }
}

struct PlaceArgs {
	cvxb::CopyWorld W;
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances; // the instances that touch the world, in the call's order
	const cvxb::ModelCullBox *boxes;     // ... and their boxes clipped to the world, for the cull
	int instanceCount;
	int x0, z0, sizeZ, n;
	uint32_t *counts;     // per column: elements (-> offset after the scan)
	uint32_t *runCounts;  // per column: runs (0: the column is empty)
	unsigned int *overLimit;
	uint32_t *headers;    // write: the sub-world blob, n headers of 3 words
	uint32_t *elements;
};

// The instances whose box covers the wave's column, as ascending indices into A.instances, and the union [*lo, *hi) of their y ranges (empty: 0, 0).
// CVX_MODELS_MAX_INSTANCES 16-bit indices per wave always fit: there is no overflow path.  A wave's list is written and read by that wave alone:
// a wave-scope fence orders the lanes' stores before the other lanes' loads.  Returns the list's length.
__device__ __forceinline__ int CullInstances(const PlaceArgs &A, int cx, int cz, int lane, uint16_t *list, int *lo, int *hi)
{
	int count = 0, myLo = INT32_MAX, myHi = INT32_MIN;
	for (int base = 0; base < A.instanceCount; base += CVX_WAVE) {
		const int s = base + lane;
		cvxb::ModelCullBox b{};
		if (s < A.instanceCount) { b = A.boxes[s]; }
		const bool keep = s < A.instanceCount && cvxb::ModelCullCovers(b, cx, cz);
		const unsigned long long kept = __ballot(keep);
		if (keep) {
			list[count + (int)cvxi::LanesBelow(kept)] = (uint16_t)s;
			myLo = min(myLo, b.y0);
			myHi = max(myHi, b.y1);
		}
		count += __popcll(kept);
	}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (a lane reads what other lanes of its wave wrote)
	__builtin_amdgcn_wave_barrier();
	for (int offset = CVX_WAVE / 2; offset > 0; offset >>= 1) {
		myLo = min(myLo, __shfl_xor(myLo, offset));
		myHi = max(myHi, __shfl_xor(myHi, offset));
	}
	*lo = count > 0 ? __builtin_amdgcn_readfirstlane(myLo) : 0;
	*hi = count > 0 ? __builtin_amdgcn_readfirstlane(myHi) : 0;
	return count;
}

// The wave's walk of column `i` of the rectangle: cvx_dense.hip's WalkColumn with cvxb::ModelsLaneVoxel for the voxel.  kWrite: runs go to outRuns,
// colours to outColours (cvxb::ModelsColumn's out arrays).  Everything but y, the voxel and the lane's slots is the same in all lanes.
template <bool kWrite>
__device__ __forceinline__ cvxb::BrushResult WalkColumn(const PlaceArgs &A, int i, int lane, uint16_t *list, uint32_t *outRuns, uint32_t *outColours)
{
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const cvxb::ArenaColumn col = cvxb::CopyColumnAt(A.W, cx, cz);
	const int dimY = A.W.dimY;
	int lo, hi;
	const int listCount = CullInstances(A, cx, cz, lane, list, &lo, &hi);
	const uint32_t count = col.Count();
	uint32_t cursor = 0u;
	uint32_t *lane0Runs = kWrite && lane == 0 ? outRuns : nullptr;
	cvxb::DenseWalk w;
	for (int yTop = dimY - 1; yTop >= 0; yTop -= CVX_WAVE) {
		const int air = cvxb::DenseAirSteps(col, count, &cursor, lo, hi, yTop);
		if (air > 0) { // nothing but air down to the next run of the arena or the instances' boxes: all those steps at once
			const int voxels = air * CVX_WAVE < yTop + 1 ? air * CVX_WAVE : yTop + 1;
			cvxb::DenseAdvanceAir(w, (uint32_t)voxels, lane0Runs);
			yTop -= (air - 1) * CVX_WAVE;
			continue;
		}
		const uint32_t valid = (uint32_t)(yTop + 1 < CVX_WAVE ? yTop + 1 : CVX_WAVE);
		const cvxb::Voxel v = cvxb::ModelsLaneVoxel(cvxi::WaveUniform{}, col, A.W.colourSlots, A.W.colorShift, A.models, A.instances, list, listCount, cx, cz, yTop, yTop - lane);
		const uint64_t mask = __ballot(v.solid); // bit l: the voxel yTop - l
		const uint64_t starts = cvxb::DenseStarts(w, mask, valid);
		if (kWrite) {
			const uint32_t solidBelow = cvxi::LanesBelow(mask);
			cvxb::DenseLaneRun(w, mask, starts, lane, cvxi::LanesBelow(starts), solidBelow, outRuns);
			if (v.solid) { outColours[w.colours + solidBelow] = v.argb; }
		}
		cvxb::DenseAdvance(w, mask, starts, valid, yTop, lane0Runs);
	}
	return cvxb::DenseFinish(w, lane0Runs);
}

__global__ __launch_bounds__(kThreads) void models_count_kernel(PlaceArgs A)
{
	__shared__ uint16_t lists[kWaves][CVX_MODELS_MAX_INSTANCES];
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CVX_WAVE));
	const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves)) + wave;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	if (i >= A.n) { return; }
	const cvxb::BrushResult r = WalkColumn<false>(A, i, lane, lists[wave], nullptr, nullptr);
	if (lane != 0) { return; }
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
	A.runCounts[i] = r.runCount;
}

__global__ __launch_bounds__(kThreads) void models_write_kernel(PlaceArgs A)
{
	__shared__ uint16_t lists[kWaves][CVX_MODELS_MAX_INSTANCES];
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CVX_WAVE));
	const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves)) + wave;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	if (i >= A.n) { return; }
	const uint32_t off = A.counts[i], runCount = A.runCounts[i];
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (runCount == 0u) {
		if (lane < 3) { h[lane] = 0u; }
		return;
	}
	uint32_t *e = A.elements + off;
	// (the count kernel left the run count: the colours go behind the runs' second guard in the same walk)
	const cvxb::BrushResult r = WalkColumn<true>(A, i, lane, lists[wave], e + 1, e + runCount + 2u);
	if (lane != 0) { return; }
	e[0] = 0u;
	e[runCount + 1u] = 0u;
	h[0] = off;
	h[1] = runCount | (r.worldMin << 16);
	h[2] = r.worldMax;
}

} // namespace cvxmodels

namespace {

using cvxi::Grid;
using cvxmodels::kThreads;

int Read(cvx_context *ctx, const char *call, const int32_t size[3], const cvx_model_map *toWorld, uint32_t *argb, uint8_t *solid, bool device, void *hipStream,
         float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!size || !toWorld) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: size or toWorld is NULL", call); }
	if (!cvxb::ModelSizeValidate(size, "the model", message, sizeof message) || !cvxb::ModelMapValidate(*toWorld, "toWorld", message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	if (!argb && !solid) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: argb and solid are both NULL", call); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }
	cvxmodels::ReadArgs A{};
	const size_t n = (size_t)size[0] * (size_t)size[1] * (size_t)size[2];
	A.W = cvxi::WorldOf(ctx);
	A.toWorld = *toWorld;
	for (int a = 0; a < 3; a++) { A.size[a] = size[a]; }
	A.n = (uint32_t)n;
	void *const to[3] = { argb, solid, nullptr };
	const size_t bytes[3] = { n * 4, n, 0 };
	return cvxi::ReadArrays(
		ctx, call, to, bytes, device, hipStream,
		[&](const cvxi::ReadArraysJob &J) {
			A.argb = static_cast<uint32_t *>(J.array[0]);
			A.solid = static_cast<uint8_t *>(J.array[1]);
			hipLaunchKernelGGL(cvxmodels::model_read_kernel, dim3(Grid(n)), dim3(kThreads), 0, J.stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

// Both places: `device` says where the models' arrays live.
int Place(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, bool device,
          int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::ModelsValidate(models, modelCount, instances, instanceCount, levelCount, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int64_t dim[3] = { ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ };
	// the instances that touch the world, and the rectangle: the union of their clipped boxes' footprints rounded out to 2^levelCount, clipped again
	std::vector<cvx_model_instance> live;
	std::vector<cvxb::ModelCullBox> boxes;
	int64_t x0 = INT64_MAX, x1 = INT64_MIN, z0 = INT64_MAX, z1 = INT64_MIN;
	for (int k = 0; k < instanceCount; k++) {
		cvxb::ModelCullBox b;
		if (!cvxb::ModelCullBoxOf(instances[k], dim[0], dim[1], dim[2], &b)) { continue; }
		live.push_back(instances[k]);
		boxes.push_back(b);
		x0 = std::min<int64_t>(x0, b.x0);
		x1 = std::max<int64_t>(x1, b.x1);
		z0 = std::min<int64_t>(z0, b.z0);
		z1 = std::max<int64_t>(z1, b.z1);
	}
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	if (live.empty()) { return CVX_OK; }
	cvxi::EditRectangle R;
	int rc = cvxi::RoundEditRectangle(ctx, x0, x1, z0, z1, levelCount, "models over", &R);
	if (rc == CVX_OK) { rc = cvxi::PrepareWorld(ctx); }
	if (rc != CVX_OK) { return rc; }

	// host arrays: a device copy of them, uploaded behind the pipeline's start so that outDeviceMs covers it
	cvxi::ModelStaging staging(models, modelCount, device);
	cvxi::DeviceCall upload(ctx, call);
	const hipError_t allocated = staging.Allocate(upload);
	if (allocated != hipSuccess) { return upload.Fail(allocated); }
	cvxmodels::PlaceArgs A{};
	A.W = cvxi::WorldOf(ctx);
	A.instanceCount = (int)live.size();
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = live.size() * sizeof(cvx_model_instance), boxesBytes = boxes.size() * sizeof(cvxb::ModelCullBox);
	cvxi::ScratchLayout extra; // the run counts, the descriptors
	const size_t oRunCounts = extra((size_t)R.n * 4), oModels = extra(modelsBytes), oInstances = extra(instancesBytes), oBoxes = extra(boxesBytes);
	const dim3 grid(Grid((size_t)R.n, cvxmodels::kWaves)), block(kThreads);
	cvxi::ColumnEditCall edit{ call, CVX_ERR_HIP, "a column under the models", "the columns under the models" };
	edit.extraScratchBytes = extra.bytes;
	return cvxi::ColumnEdit(
		ctx, R, levelCount, edit,
		[&](const cvxi::ColumnEditJob &J) {
			hipError_t e = staging.Enqueue(ctx->stream);
			A.counts = J.counts;
			A.runCounts = reinterpret_cast<uint32_t *>(J.extra + oRunCounts);
			A.models = reinterpret_cast<const cvx_model *>(J.extra + oModels);
			A.instances = reinterpret_cast<const cvx_model_instance *>(J.extra + oInstances);
			A.boxes = reinterpret_cast<const cvxb::ModelCullBox *>(J.extra + oBoxes);
			A.overLimit = J.overLimit;
			if (e == hipSuccess) { e = hipMemcpyAsync(J.extra + oBoxes, boxes.data(), boxesBytes, hipMemcpyHostToDevice, ctx->stream); }
			if (e == hipSuccess) { e = hipMemcpyAsync(J.extra + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
			if (e == hipSuccess) { e = hipMemcpyAsync(J.extra + oInstances, live.data(), instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
			if (e == hipSuccess) { hipLaunchKernelGGL(cvxmodels::models_count_kernel, grid, block, 0, ctx->stream, A); }
			return e;
		},
		[&](const cvxi::ColumnEditJob &J) {
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxmodels::models_write_kernel, grid, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

} // namespace

extern "C" {

int cvx_world_place_models(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int levelCount,
                           float *outDeviceMs)
{
	return Place(ctx, "cvx_world_place_models", models, modelCount, instances, instanceCount, false, levelCount, outDeviceMs);
}

int cvx_world_place_models_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int levelCount,
                                  float *outDeviceMs)
{
	return Place(ctx, "cvx_world_place_models_device", models, modelCount, instances, instanceCount, true, levelCount, outDeviceMs);
}

int cvx_world_read_model(cvx_context *ctx, const int32_t size[3], const cvx_model_map *toWorld, uint32_t *argb, uint8_t *solid, float *outDeviceMs)
{
	return Read(ctx, "cvx_world_read_model", size, toWorld, argb, solid, false, nullptr, outDeviceMs);
}

int cvx_world_read_model_device(cvx_context *ctx, const int32_t size[3], const cvx_model_map *toWorld, uint32_t *argbDevice, uint8_t *solidDevice, void *hipStream)
{
	return Read(ctx, "cvx_world_read_model_device", size, toWorld, argbDevice, solidDevice, true, hipStream, nullptr);
}

int cvx_model_instance_from_matrix(const double forward[12], const int32_t size[3], int model, int op, cvx_model_instance *out)
{
	return cvxb::ModelInstanceFromMatrix(forward, size, model, op, out) ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

} // extern "C"
