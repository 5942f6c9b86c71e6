// cvx_model_brush.hip -- libcpuvox_gpu.so, world-space brush strokes that carve and paint placed voxel models (cvxd_models_brush,
// cvxd_models_brush_device, cvxd_model_mass).  See include/cpuvox_gpu_model_brush.h for the contract and cvx_model_brush.h for the rules.
//
//   1. cull   a WAVE per (instance, 64 strokes): a lane compares its stroke's footprint with the instance's box (cvxb::ModelBrushCullLane), the
//             ballot is one word of the instance's list: a bit per stroke, ascending, strokeCount / 8 bytes an instance.  Nothing is counted,
//             scanned or brought to the host: the jobs are the host's, the columns of the instances whose box meets the box around all
//             strokes (cvxb::ModelBrushJobs), so the call has no synchronisation in the middle.
//   2. mark   a WAVE per (instance, column of its box) job (beyond 2^18 jobs the waves take them in turn); the host uploads the prefix of the
//             instances' jobs and a wave finds its instance with cvx_pair_contacts.h's wave-uniform search.  The instance, its map, the model
//             and the strokes live on the scalar side (cvxb::ContactsColumnJobOf, ModelBrushLaneKey through readfirstlane).  The lanes are
//             the 64 voxels of a step of the column (the tall-box cut is cvxb::ContactsStepRange): a lane maps its voxel once and tests SET
//             once, the wave ballots and skips a step without a body voxel; then every lane takes the maximum key over the listed strokes
//             whose span holds its y, and a lane with a key issues ONE atomicMax on its element's word of the key array.  The instance's
//             counts come from two ballots a step; lane 0 adds them with two 64-bit atomics a job.  The models' arrays are only read.
//   3. apply  a WAVE per (model, chunk of 1024 elements) job, found by the same search in the prefix of the models' chunks: an element with a key
//             is cleared or recoloured with plain vector stores, and every element still set adds to the lane's counts, nine sums and box;
//             the wave reduces them and lane 0 adds them to the model's result: 64-bit atomic adds and 32-bit atomicMin / atomicMax, none for
//             a chunk without a set or carved voxel.
// The key array is a maximum and the results are sums, minima and maxima of integers: the schedule does not show.  No LDS, no float, no inline
// assembly.  Host models are staged by cvxi::ModelStaging (cvx_model_call.h) and copied back once the call can no longer fail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cvx_model_brush.h"
#include "cvx_model_call.h"
#include "cvx_pair_contacts.h"

using cvxi::Fail;

namespace cvxmodelbrush {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // 2^18 waves, the waves take the jobs in turn
static_assert(sizeof(cvxd_model_result) == 128 && sizeof(cvxd_instance_result) == 16 && sizeof(cvxd_brush_summary) == 32 && offsetof(cvxd_model_result, min) == 96,
              "the records as the header states them");
static_assert(sizeof(cvx_brush_stroke) == 40, "the stroke of include/cpuvox_gpu.h");

struct Args {
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	const cvx_brush_stroke *strokes;
	const uint32_t *prefix;              // instanceCount + 1: the mark jobs before every instance
	const uint32_t *chunkPrefix;         // modelCount + 1: the apply jobs before every model
	const uint64_t *volumePrefix;        // modelCount + 1: the elements before every model
	uint64_t *lists;                     // instanceCount x words: the strokes whose footprint meets the instance's box
	uint32_t *keys;                      // one word per element of every model
	cvxd_model_result *results;          // modelCount, initialised by the host
	unsigned long long *counts;          // instanceCount x 2: carved, painted
	int modelCount, instanceCount, strokeCount, words;
	uint32_t jobs, chunks;
};

// The LAST entry p of prefix[0 .. n) with prefix[p] <= job, the same in every lane: 64 probes a round.
__device__ __forceinline__ int32_t UnitOf(const uint32_t *prefix, int32_t n, uint32_t job, int lane)
{
	int32_t p = 0, within = n;
	while (within > 1) {
		const int32_t probe = cvxb::PairSearchProbe(p, within, lane);
		cvxb::PairSearchNarrow(&p, &within, __ballot(probe >= 0 && prefix[probe >= 0 ? probe : 0] <= job));
	}
	return __builtin_amdgcn_readfirstlane(p);
}

__global__ __launch_bounds__(kThreads) void brush_cull_kernel(Args A)
{
	cvxi::ForEachWaveJob((uint32_t)A.instanceCount * (uint32_t)A.words, kWaves, [&](uint64_t at, int lane) {
		const uint32_t k = (uint32_t)at / (uint32_t)A.words, w = (uint32_t)at % (uint32_t)A.words;
		const uint64_t kept = __ballot(cvxb::ModelBrushCullLane(A.strokes, A.strokeCount, A.instances[k], (int)(64u * w) + lane));
		if (lane == 0) { A.lists[at] = kept; }
	});
}

// cvxb::ModelBrushColumn's lanes on the device: a lane evaluates its own voxel, the wave ballots.
struct WaveLanes {
	int lane;
	mutable int64_t at;
	__device__ __forceinline__ uint64_t Body(const cvxb::ContactsColumnJob &J, int32_t yTop) const
	{
		at = cvxb::ModelBrushLaneElement(J, yTop - lane);
		return __ballot(at >= 0);
	}
	// (every lane walks the list, whatever its voxel: the walk's branches are the wave's)
	__device__ __forceinline__ void Mark(const cvxi::WaveUniform &U, const cvxb::ContactsColumnJob &J, const cvx_brush_stroke *strokes, const uint64_t *list, int words,
	                                     int32_t yTop, uint64_t, uint32_t *keys, uint64_t *carved, uint64_t *painted) const
	{
		const uint32_t found = cvxb::ModelBrushLaneKey(U, strokes, list, words, J.M.argb != nullptr, J.cx, J.cz, yTop, yTop - lane);
		const uint32_t key = at >= 0 ? found : 0u;
		if (key != 0u) { atomicMax(keys + at, key); }
		*carved = __ballot(key == cvxb::kModelBrushCarve);
		*painted = __ballot(key != 0u && key != cvxb::kModelBrushCarve);
	}
};

__global__ __launch_bounds__(kThreads) void brush_mark_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.jobs, kWaves, [&](uint64_t at, int lane) {
		const cvxi::WaveUniform U;
		const int32_t k = UnitOf(A.prefix, A.instanceCount, (uint32_t)at, lane);
		const cvx_model_instance &I = A.instances[k];
		const uint32_t column = (uint32_t)at - (uint32_t)U((int32_t)A.prefix[k]);
		const uint32_t sizeZ = (uint32_t)(U(I.boxMax[2]) - U(I.boxMin[2]));
		const int32_t cx = U(I.boxMin[0]) + (int32_t)(column / sizeZ), cz = U(I.boxMin[2]) + (int32_t)(column % sizeZ);
		const uint64_t first = (uint64_t)cvxb::ContactUniform64(U, A.volumePrefix[U(I.model)]);
		uint32_t carved = 0u, painted = 0u;
		cvxb::ModelBrushColumn(U, WaveLanes{ lane, -1 }, A.models, I, A.strokes, A.lists + (size_t)k * (size_t)A.words, A.words, cx, cz, A.keys + first, &carved, &painted);
		if (lane == 0 && carved != 0u) { atomicAdd(A.counts + 2 * (size_t)k, (unsigned long long)carved); }
		if (lane == 0 && painted != 0u) { atomicAdd(A.counts + 2 * (size_t)k + 1, (unsigned long long)painted); }
	});
}

__global__ __launch_bounds__(kThreads) void brush_apply_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.chunks, kWaves, [&](uint64_t at, int lane) {
		const cvxi::WaveUniform U;
		const int32_t g = UnitOf(A.chunkPrefix, A.modelCount, (uint32_t)at, lane);
		const uint32_t chunk = (uint32_t)at - (uint32_t)U((int32_t)A.chunkPrefix[g]);
		const cvx_model &G = A.models[g];
		cvx_model M;
		M.size[0] = U(G.size[0]);
		M.size[1] = U(G.size[1]);
		M.size[2] = U(G.size[2]);
		M.pad_ = 0;
		M.argb = reinterpret_cast<const uint32_t *>((uintptr_t)cvxb::ContactUniform64(U, (uint64_t)(uintptr_t)G.argb));
		M.solid = reinterpret_cast<const uint8_t *>((uintptr_t)cvxb::ContactUniform64(U, (uint64_t)(uintptr_t)G.solid));
		const uint64_t first = (uint64_t)cvxb::ContactUniform64(U, A.volumePrefix[g]);
		cvxb::ModelBrushSums S;
		cvxb::ModelBrushApplyLane(M, A.keys + first, A.strokes, (uint32_t)cvxb::ModelBrushVolume(M), chunk, lane, &S);
		if (__ballot(S.voxels != 0u || S.carved != 0u) == 0ull) { return; } // (a painted voxel is a set one)
		const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
		const auto least = [](int32_t a, int32_t b) { return a < b ? a : b; };
		const auto most = [](int32_t a, int32_t b) { return a > b ? a : b; };
		cvxd_model_result *r = A.results + g;
		const unsigned long long voxels = cvxi::WaveReduce((unsigned long long)S.voxels, add), carved = cvxi::WaveReduce((unsigned long long)S.carved, add),
		                         painted = cvxi::WaveReduce((unsigned long long)S.painted, add);
		if (lane == 0 && carved != 0ull) { atomicAdd(reinterpret_cast<unsigned long long *>(&r->carved), carved); }
		if (voxels == 0ull) { return; }
		if (lane == 0) { atomicAdd(reinterpret_cast<unsigned long long *>(&r->voxels), voxels); }
		if (lane == 0 && painted != 0ull) { atomicAdd(reinterpret_cast<unsigned long long *>(&r->painted), painted); }
		// (every array element is addressed by a constant: the sums stay in registers)
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const unsigned long long sum = cvxi::WaveReduce((unsigned long long)S.sum[a], add);
			const int32_t lo = cvxi::WaveReduce(S.min[a], least), hi = cvxi::WaveReduce(S.max[a], most);
			if (lane == 0) {
				atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum[a]), sum);
				atomicMin(&r->min[a], lo);
				atomicMax(&r->max[a], hi);
			}
		}
#pragma unroll
		for (int a = 0; a < 6; a++) {
			const unsigned long long moment = cvxi::WaveReduce((unsigned long long)S.moment[a], add);
			if (lane == 0) { atomicAdd(reinterpret_cast<unsigned long long *>(&r->moment[a]), moment); }
		}
	});
}

// Both calls: `device` says where the models' arrays live.
static int ModelsBrush(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                       const cvx_brush_stroke *strokes, int strokeCount, cvxd_model_result *modelResults, cvxd_instance_result *instanceResults, cvxd_brush_summary *summary,
                       bool device, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[200];
	if (!cvxb::ModelBrushValidate(models, modelCount, instances, instanceCount, strokes, strokeCount, modelResults, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	std::vector<uint32_t> prefix((size_t)instanceCount + 1), chunkPrefix((size_t)modelCount + 1);
	std::vector<uint64_t> volumePrefix((size_t)modelCount + 1);
	const int64_t jobs = cvxb::ModelBrushJobs(instances, instanceCount, strokes, strokeCount, prefix.data());
	if (jobs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the columns of the instances' boxes that the strokes can reach sum to 2^31 - 1 or more jobs", call); }
	uint64_t elements = 0u;
	uint32_t chunks = 0u; // (at most 2^21 a model, 256 models)
	for (int g = 0; g < modelCount; g++) {
		volumePrefix[g] = elements;
		chunkPrefix[g] = chunks;
		elements += (uint64_t)cvxb::ModelBrushVolume(models[g]);
		chunks += cvxb::ModelBrushChunks(cvxb::ModelBrushVolume(models[g]));
	}
	volumePrefix[modelCount] = elements;
	chunkPrefix[modelCount] = chunks;
	CVX_HIP(ctx, hipSetDevice(ctx->device));

	// (these outlive D: freeing the device blocks waits for a copy still under way)
	const int words = cvxb::ModelBrushWords(strokeCount);
	std::vector<cvxd_model_result> results((size_t)modelCount);
	std::vector<cvxd_instance_result> counts((size_t)instanceCount);
	for (cvxd_model_result &r : results) { cvxb::ModelBrushResultInit(&r); }
	cvxi::ModelStaging staging(models, modelCount, device);
	std::vector<uint8_t> back(device ? 0 : staging.layout.bytes);
	float ms = 0.f;
	{
		cvxi::DeviceCall D(ctx, call);
		uint8_t *scratch = nullptr;
		uint32_t *keys = nullptr;
		hipError_t e = staging.Allocate(D);
		if (e != hipSuccess) { return D.Fail(e); }
		cvxi::ScratchLayout carve;
		const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance),
		             strokesBytes = (size_t)strokeCount * sizeof(cvx_brush_stroke), prefixBytes = prefix.size() * 4, chunkBytes = chunkPrefix.size() * 4,
		             volumeBytes = volumePrefix.size() * 8, listsBytes = (size_t)instanceCount * (size_t)words * 8, resultsBytes = results.size() * sizeof(cvxd_model_result),
		             countsBytes = counts.size() * sizeof(cvxd_instance_result), keysBytes = (size_t)elements * 4;
		const size_t oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oStrokes = carve(strokesBytes), oPrefix = carve(prefixBytes), oChunks = carve(chunkBytes),
		             oVolumes = carve(volumeBytes), oLists = carve(listsBytes), oResults = carve(resultsBytes), oCounts = carve(countsBytes);
		e = D.Allocate(&scratch, carve.bytes);
		if (e == hipSuccess) { e = D.Allocate(&keys, keysBytes); }
		if (e == hipSuccess) { e = D.Begin(); }
		if (e == hipSuccess) { e = staging.Enqueue(ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oStrokes, strokes, strokesBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPrefix, prefix.data(), prefixBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oChunks, chunkPrefix.data(), chunkBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oVolumes, volumePrefix.data(), volumeBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oResults, results.data(), resultsBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemsetAsync(scratch + oCounts, 0, countsBytes, ctx->stream); }
		if (e == hipSuccess) { e = hipMemsetAsync(keys, 0, keysBytes, ctx->stream); }
		if (e == hipSuccess) {
			Args A{};
			A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
			A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
			A.strokes = reinterpret_cast<const cvx_brush_stroke *>(scratch + oStrokes);
			A.prefix = reinterpret_cast<const uint32_t *>(scratch + oPrefix);
			A.chunkPrefix = reinterpret_cast<const uint32_t *>(scratch + oChunks);
			A.volumePrefix = reinterpret_cast<const uint64_t *>(scratch + oVolumes);
			A.lists = reinterpret_cast<uint64_t *>(scratch + oLists);
			A.keys = keys;
			A.results = reinterpret_cast<cvxd_model_result *>(scratch + oResults);
			A.counts = reinterpret_cast<unsigned long long *>(scratch + oCounts);
			A.modelCount = modelCount;
			A.instanceCount = instanceCount;
			A.strokeCount = strokeCount;
			A.words = words;
			A.jobs = (uint32_t)jobs;
			A.chunks = chunks;
			if (jobs > 0) { // (a call whose strokes lie far from every body marks nothing; the results are still the models')
				const size_t lists = (size_t)instanceCount * (size_t)words;
				hipLaunchKernelGGL(brush_cull_kernel, dim3(std::min(cvxi::Grid(lists, kWaves), kMaxWorkgroups)), dim3(kThreads), 0, ctx->stream, A);
				hipLaunchKernelGGL(brush_mark_kernel, dim3(std::min(cvxi::Grid((size_t)jobs, kWaves), kMaxWorkgroups)), dim3(kThreads), 0, ctx->stream, A);
			}
			hipLaunchKernelGGL(brush_apply_kernel, dim3(std::min(cvxi::Grid((size_t)chunks, kWaves), kMaxWorkgroups)), dim3(kThreads), 0, ctx->stream, A);
			e = hipGetLastError();
		}
		if (e == hipSuccess) { e = hipMemcpyAsync(results.data(), scratch + oResults, resultsBytes, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(counts.data(), scratch + oCounts, countsBytes, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess && !back.empty()) { e = hipMemcpyAsync(back.data(), staging.block, back.size(), hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = D.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
		ms = D.Ms();
	}
	// (nothing is handed out to the host, the models' arrays included, before the call can no longer fail)
	for (const cvxi::ModelStaging::Upload &u : staging.uploads) {
		if (!back.empty()) { std::memcpy(const_cast<void *>(u.from), back.data() + u.at, u.bytes); }
	}
	for (cvxd_model_result &r : results) { cvxb::ModelBrushFinish(&r); }
	std::memcpy(modelResults, results.data(), results.size() * sizeof(cvxd_model_result));
	if (instanceResults) { std::memcpy(instanceResults, counts.data(), counts.size() * sizeof(cvxd_instance_result)); }
	if (summary) { *summary = cvxb::ModelBrushSummary(results.data(), modelCount, jobs); }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // namespace cvxmodelbrush

extern "C" {

int cvxd_models_brush(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_brush_stroke *strokes,
                      int strokeCount, cvxd_model_result *modelResults, cvxd_instance_result *instanceResults, cvxd_brush_summary *summary, float *outDeviceMs)
{
	return cvxmodelbrush::ModelsBrush(ctx, "cvxd_models_brush", models, modelCount, instances, instanceCount, strokes, strokeCount, modelResults, instanceResults, summary, false,
	                                  outDeviceMs);
}

int cvxd_models_brush_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_brush_stroke *strokes,
                             int strokeCount, cvxd_model_result *modelResults, cvxd_instance_result *instanceResults, cvxd_brush_summary *summary, float *outDeviceMs)
{
	return cvxmodelbrush::ModelsBrush(ctx, "cvxd_models_brush_device", models, modelCount, instances, instanceCount, strokes, strokeCount, modelResults, instanceResults, summary,
	                                  true, outDeviceMs);
}

int cvxd_model_mass(const cvxd_model_result *r, double centre[3], double inertia[6])
{
	if (!r || r->voxels <= 0) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxb::ModelBrushMass(*r, centre, inertia);
	return CVX_OK;
}

} // extern "C"
