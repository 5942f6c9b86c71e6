// cvx_model_pick.hip -- libcpuvox_gpu.so, first-hit rays against placed voxel models (cvxq_model_pick, cvxq_model_pick_device).  See
// include/cpuvox_gpu_model_pick.h for the contract and cvx_model_pick.h for the rules.
//
//   1. clip   a thread per (ray, instance) pair, pair = ray * instanceCount + instance, runs steps 1 .. 3 of the pair rule (cvxb::ModelPickClip).  The
//             pairs whose box the ray crosses are the jobs: count (one count per wave of 64 pairs, from a ballot), cvxi::ExclusiveScan, ONE copy
//             brings the number of jobs to the host, write (the same clip; a job is its pair's index, 4 bytes).  Nothing but the counts is sized
//             by the pairs.  The count pass also clears the rays' keys.
//   2. walk   a WAVE per job (at most kMaxWorkgroups workgroups take the jobs in turn).  The job's ray, the instance's box and map and the
//             model's descriptor live in scalar registers (readfirstlane), the clipped ray too.  Lane l of step n runs layer 64 n + l of the
//             box along the ray's dominant axis (cvxb::ModelPickLayer: closed-form entry state, then the rule's own loop over the layer's
//             voxels: the int64 map and one gather each).  One ballot of "hit or end" a step; the lowest such lane decides: a hit goes into
//             the ray's key with ONE 64-bit atomicMin (the reported float's bits above the instance), an end ends the job.  Before a step
//             the wave reads the key: once the step's entering time lies above it, by more than the float ulp the start state's rounding
//             could cost, nothing of this job can win and the wave stops.  The key is a minimum: the schedule does not show in it.
//   3. hits   a wave per ray reads the key and walks the winning pair again, the same walk, and the deciding lane writes the whole record
//             (voxel, face, colour, model voxel); a ray without a key gets the miss.  A re-walk rather than a record per job: 8 bytes a ray
//             instead of 48 a job, and the second walk of one pair per ray is cheap against the first walk of all of them.
// No LDS, no scratch memory in the walk.  No world is read: the calls work on a context with nothing uploaded.  Host models, rays and hits are
// staged by cvxi::ModelStaging (cvx_model_call.h); the turn loop is cvxi::ForEachWaveJob.
// CVXQ_LANE_PER_JOB (an experiment build, `make variant`): the walk as a lane per job running cvxb::ModelPickSequential, the measure
// tools/model_pick_bench.py compares the wave's walk with.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cvx_model_call.h"
#include "cvx_model_pick.h"

using cvxi::Fail;

namespace cvxmodelpick {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 8192; // of the walk: 2^15 waves
static_assert(sizeof(cvxq_model_hit) == 48 && sizeof(cvx_pick_ray) == 32, "the records of include/cpuvox_gpu_model_pick.h");
static_assert((uint64_t)CVXQ_PICK_MAX_RAYS * CVX_MODELS_MAX_INSTANCES <= (1ull << 28), "a pair's index fits a job's 32 bits");

struct Args {
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	const cvx_pick_ray *rays;
	int instanceCount, rayCount;
	uint32_t pairs;                      // rayCount * instanceCount
	uint32_t *counts;                    // one per wave of pairs: its jobs (-> the jobs before it after the scan)
	uint32_t *jobs;                      // a job's pair
	uint32_t jobCount;
	unsigned long long *keys;            // one per ray: cvxb::ModelPickKey of its nearest hit so far
	cvxq_model_hit *hits;
};

// The clip of pair `pair`, by the thread that owns it.
__device__ __forceinline__ bool PairCrosses(const Args &A, uint32_t pair)
{
	const cvx_pick_ray &ray = A.rays[pair / (uint32_t)A.instanceCount];
	const cvx_model_instance &I = A.instances[pair % (uint32_t)A.instanceCount];
	cvxb::ModelPickRay R;
	cvxb::ModelPickState S;
	return cvxb::ModelPickClip(ray.origin, ray.direction, ray.maxT, I.boxMin, I.boxMax, &R, &S);
}

template <bool kWrite> __global__ __launch_bounds__(kThreads) void pick_clip_kernel(Args A)
{
	const uint32_t pair = blockIdx.x * kThreads + threadIdx.x; // (below 2^28 + 256)
	const bool job = pair < A.pairs && PairCrosses(A, pair);
	const uint64_t jobs = __ballot(job);
	if (kWrite) {
		if (job) { A.jobs[A.counts[pair / CVX_WAVE] + cvxi::LanesBelow(jobs)] = pair; }
		return;
	}
	if (threadIdx.x % CVX_WAVE == 0 && pair < A.pairs) { A.counts[pair / CVX_WAVE] = (uint32_t)__popcll(jobs); }
	if (pair < (uint32_t)A.rayCount) { A.keys[pair] = cvxb::kModelPickNoKey; }
}

// What a wave knows of its job besides the body, the same in every lane: the clipped ray, the start state and the dominant axis, through
// readfirstlane into scalar registers.  False: the ray misses the box.
__device__ __forceinline__ bool JobOf(const Args &A, uint32_t rayIndex, const cvxb::ModelPickBody &B, cvxb::ModelPickRay *uniformRay, cvxb::ModelPickState *uniformStart, int *M)
{
	const cvxi::WaveUniform U;
	const cvx_pick_ray &ray = A.rays[rayIndex];
	const float o[3] = { U(ray.origin[0]), U(ray.origin[1]), U(ray.origin[2]) }, d[3] = { U(ray.direction[0]), U(ray.direction[1]), U(ray.direction[2]) };
	cvxb::ModelPickRay R;
	cvxb::ModelPickState S;
	if (!cvxb::ModelPickClip(o, d, U(ray.maxT), B.lo, B.hi, &R, &S)) { return false; }
	// (every array element is addressed by a constant)
	uniformRay->o[0] = U(R.o[0]), uniformRay->o[1] = U(R.o[1]), uniformRay->o[2] = U(R.o[2]);
	uniformRay->d[0] = U(R.d[0]), uniformRay->d[1] = U(R.d[1]), uniformRay->d[2] = U(R.d[2]);
	uniformRay->inv[0] = U(R.inv[0]), uniformRay->inv[1] = U(R.inv[1]), uniformRay->inv[2] = U(R.inv[2]);
	uniformRay->tEnter = U(R.tEnter);
	uniformRay->tExit = U(R.tExit);
	uniformStart->v[0] = U(S.v[0]), uniformStart->v[1] = U(S.v[1]), uniformStart->v[2] = U(S.v[2]);
	uniformStart->face = U(S.face);
	uniformStart->t = uniformRay->tEnter;
	*M = U(cvxb::ModelPickMajor(*uniformRay));
	return true;
}

// The wave's walk of a job.  kWrite false: its hit, if it has one, into the ray's key; true: the hit's record into *out (the job is the ray's
// winner: it has one).
template <bool kWrite> __device__ __forceinline__ void WalkJob(const Args &A, uint32_t rayIndex, int32_t instance, int lane, cvxq_model_hit *out)
{
	const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(cvxi::WaveUniform{}, A.models, A.instances[instance]);
	cvxb::ModelPickRay R;
	cvxb::ModelPickState start;
	int M;
	if (!JobOf(A, rayIndex, B, &R, &start, &M)) { return; }
	const int32_t startM = cvxb::ModelPickOf(M, start.v[0], start.v[1], start.v[2]);
	for (int64_t base = 0;; base += CVX_WAVE) {
		if (!kWrite) { // nothing from here on is earlier than the step's entering time
			const float enter = cvxb::ModelPickReported(base == 0 ? R.tEnter : cvxb::ModelPickLayerTime(R, M, startM, base));
			const unsigned long long key = __hip_atomic_load(&A.keys[rayIndex], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if ((uint64_t)cvxb::ModelPickFloatBits(enter) > (uint64_t)(key >> 32) + 1u) { return; }
		}
		cvxb::ModelPickState S;
		int64_t s[3];
		const int code = cvxb::ModelPickLayer(R, B, start, M, base + lane, &S, s);
		const uint64_t stops = __ballot(code != cvxb::kModelPickGo);
		if (stops == 0ull) { continue; }
		if (lane == (int)__builtin_ctzll(stops) && code == cvxb::kModelPickHit) {
			if (kWrite) {
				*out = cvxb::ModelPickHitOf(B, S, s, instance);
			} else {
				atomicMin(&A.keys[rayIndex], (unsigned long long)cvxb::ModelPickKey(cvxb::ModelPickReported(S.t), instance));
			}
		}
		return;
	}
}

#ifndef CVXQ_LANE_PER_JOB
__global__ __launch_bounds__(kThreads) void pick_walk_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.jobCount, kWaves, [&](uint64_t at, int lane) {
		const uint32_t pair = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)A.jobs[at]);
		WalkJob<false>(A, pair / (uint32_t)A.instanceCount, (int32_t)(pair % (uint32_t)A.instanceCount), lane, nullptr);
	});
}
#else
// the experiment: a lane per job, the pair rule a voxel at a time
__global__ __launch_bounds__(kThreads) void pick_walk_kernel(Args A)
{
	const uint32_t threads = gridDim.x * kThreads;
	for (uint64_t at = blockIdx.x * kThreads + threadIdx.x; at < A.jobCount; at += threads) {
		const uint32_t pair = A.jobs[at], rayIndex = pair / (uint32_t)A.instanceCount;
		const int32_t instance = (int32_t)(pair % (uint32_t)A.instanceCount);
		const cvx_pick_ray &ray = A.rays[rayIndex];
		const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(cvxb::SameInEveryLane{}, A.models, A.instances[instance]);
		cvxb::ModelPickRay R;
		cvxb::ModelPickState S;
		int64_t s[3];
		if (!cvxb::ModelPickClip(ray.origin, ray.direction, ray.maxT, B.lo, B.hi, &R, &S) || !cvxb::ModelPickSequential(R, B, &S, s)) { continue; }
		atomicMin(&A.keys[rayIndex], (unsigned long long)cvxb::ModelPickKey(cvxb::ModelPickReported(S.t), instance));
	}
}
#endif

// A wave per ray: the record of the key's hit, or the miss.
__global__ __launch_bounds__(kThreads) void pick_hits_kernel(Args A)
{
	const uint32_t rayIndex = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / CVX_WAVE));
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	if (rayIndex >= (uint32_t)A.rayCount) { return; }
	const unsigned long long key = A.keys[rayIndex];
	if (key == cvxb::kModelPickNoKey) {
		if (lane == 0) { A.hits[rayIndex] = cvxb::ModelPickMiss(A.rays[rayIndex].maxT); }
		return;
	}
	WalkJob<true>(A, rayIndex, __builtin_amdgcn_readfirstlane((int32_t)(uint32_t)key), lane, A.hits + rayIndex);
}

// Both calls: `device` says where the models' arrays, `rays` and `hits` live.
static int ModelPick(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                     const cvx_pick_ray *rays, int rayCount, cvxq_model_hit *hits, bool device, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::ModelPickValidate(models, modelCount, instances, instanceCount, rays, rayCount, hits, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	CVX_HIP(ctx, hipSetDevice(ctx->device));

	// (these outlive D: freeing the device blocks waits for a copy still under way)
	std::vector<cvxq_model_hit> back(device ? 0 : (size_t)rayCount);
	cvxi::ModelStaging staging(models, modelCount, device);
	unsigned long long jobCount = 0ull;
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	uint32_t *jobs = nullptr;
	const size_t raysBytes = (size_t)rayCount * sizeof(cvx_pick_ray), hitsBytes = (size_t)rayCount * sizeof(cvxq_model_hit);
	const size_t oRays = device ? 0 : staging.Add(raysBytes, rays), oHits = device ? 0 : staging.Add(hitsBytes, nullptr); // host rays and hits: behind the arrays
	hipError_t e = staging.Allocate(D);
	if (e != hipSuccess) { return D.Fail(e); }
	const size_t pairs = (size_t)rayCount * (size_t)instanceCount, waves = (pairs + CVX_WAVE - 1) / CVX_WAVE;
	const size_t chunks = (waves + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
	cvxi::ScratchLayout carve;
	const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance);
	const size_t oTotal = carve(8), oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oKeys = carve((size_t)rayCount * 8), oCounts = carve(waves * 4),
	             oChunks = carve(chunks * 8);
	Args A{};
	e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = staging.Enqueue(ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
		A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
		A.rays = device ? rays : reinterpret_cast<const cvx_pick_ray *>(staging.block + oRays);
		A.instanceCount = instanceCount;
		A.rayCount = rayCount;
		A.pairs = (uint32_t)pairs;
		A.counts = reinterpret_cast<uint32_t *>(scratch + oCounts);
		A.keys = reinterpret_cast<unsigned long long *>(scratch + oKeys);
		A.hits = device ? hits : reinterpret_cast<cvxq_model_hit *>(staging.block + oHits);
		hipLaunchKernelGGL(pick_clip_kernel<false>, dim3(cvxi::Grid(pairs, kThreads)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.counts, (int)waves, reinterpret_cast<unsigned long long *>(scratch + oChunks), reinterpret_cast<unsigned long long *>(scratch + oTotal));
		e = hipGetLastError();
	}
	// the one synchronisation in the middle: the job list is sized by the jobs found
	if (e == hipSuccess) { e = hipMemcpyAsync(&jobCount, scratch + oTotal, 8, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e == hipSuccess && jobCount > 0ull) { e = D.Allocate(&jobs, (size_t)jobCount * 4); }
	if (e == hipSuccess) {
		A.jobs = jobs;
		A.jobCount = (uint32_t)jobCount;
		if (jobCount > 0ull) {
			hipLaunchKernelGGL(pick_clip_kernel<true>, dim3(cvxi::Grid(pairs, kThreads)), dim3(kThreads), 0, ctx->stream, A);
#ifndef CVXQ_LANE_PER_JOB
			const unsigned walkGrid = std::min(cvxi::Grid((size_t)jobCount, kWaves), kMaxWorkgroups);
#else
			const unsigned walkGrid = std::min(cvxi::Grid((size_t)jobCount, kThreads), kMaxWorkgroups);
#endif
			hipLaunchKernelGGL(pick_walk_kernel, dim3(walkGrid), dim3(kThreads), 0, ctx->stream, A);
		}
		hipLaunchKernelGGL(pick_hits_kernel, dim3(cvxi::Grid((size_t)rayCount, kWaves)), dim3(kThreads), 0, ctx->stream, A);
		e = hipGetLastError();
	}
	if (e == hipSuccess && !device) { e = hipMemcpyAsync(back.data(), A.hits, hitsBytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	// (nothing is handed out to the host before the call can no longer fail)
	if (!back.empty()) { std::memcpy(hits, back.data(), hitsBytes); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxmodelpick

extern "C" {

int cvxq_model_pick(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_pick_ray *rays,
                    int rayCount, cvxq_model_hit *hits, float *outDeviceMs)
{
	return cvxmodelpick::ModelPick(ctx, "cvxq_model_pick", models, modelCount, instances, instanceCount, rays, rayCount, hits, false, outDeviceMs);
}

int cvxq_model_pick_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                           const cvx_pick_ray *raysDevice, int rayCount, cvxq_model_hit *hitsDevice, float *outDeviceMs)
{
	return cvxmodelpick::ModelPick(ctx, "cvxq_model_pick_device", models, modelCount, instances, instanceCount, raysDevice, rayCount, hitsDevice, true, outDeviceMs);
}

} // extern "C"
