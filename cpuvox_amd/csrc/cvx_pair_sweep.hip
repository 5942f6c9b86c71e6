// cvx_pair_sweep.hip -- libcpuvox_gpu.so, how far placed voxel models can move before they touch each other (cvxm_pair_sweep,
// cvxm_pair_sweep_device).  See include/cpuvox_gpu_pair_sweep.h for the contract and cvx_pair_sweep.h for the rules.
//
// Phase 1.  A WAVE per (pair, column of a's box that can come over b's box) job (beyond 2^18 jobs the waves take them in turn); the host uploads
// the prefix of the pairs' jobs and a wave finds its pair with cvx_pair_contacts.hip's wave-uniform search, 64 probes a round.  Both bodies'
// column jobs, the motion, the steps taken and the window of poses live on the scalar side (cvxb::PairSweepColumn through readfirstlane): body a
// stays where it is, body b goes the path backwards, a 64-bit addition per axis and pose.  The lanes are the 64 voxels of a step of a's column:
// a lane whose voxel is in a's body maps it into b's model at every pose of the window -- one multiply-add per axis, the shift, b's y range, one
// gather -- and the wave ballots; the first pose with a set bit is the step's candidate and ends its walk, a later step of a tall column walks
// only the poses before it.  The ballots leave the candidate the same in every lane, so there is nothing to reduce: the wave issues ONE 32-bit
// atomicMin on first[p].  No LDS, nothing but first[] is written, and first[] is never read back by a wave: every loop is a counted walk of
// its window (an early exit on another wave's minimum would be an agent-scope load a job, which cost cvx_sweep.hip 3.5 times, profiles/sweep.md).
// Phase 2.  The host reads first[] (4 bytes a pair), fills the sweeps and, if contacts are asked for, runs the body of cvxp_model_contacts
// (cvxi::PairContacts, cvx_pair_contacts.hip's kernels as they are) with body a of every pair at its pose `at`; the models' arrays are staged
// once for both phases.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cvx_model_call.h"
#include "cvx_pair_sweep.h"

using cvxi::Fail;

namespace cvxpairsweep {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // 2^18 waves, the waves take the jobs in turn
static_assert(sizeof(cvxm_pair_sweep_result) == 56 && sizeof(cvxm_pair_sweeps_summary) == 32 && offsetof(cvxm_pair_sweep_result, a) == 48, "the records as the header states them");

struct Args {
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	const int32_t *pairs;                // pairCount x 2
	const int32_t *motions;              // pairCount x 3
	const uint32_t *prefix;              // pairCount + 1: the jobs before every pair
	uint32_t *first;                     // per pair the least touching pose so far, kSweepNone: none
	int pairCount;
	uint32_t jobs;
};

// cvxb::PairSweepColumn's lanes on the device: a lane evaluates its own voxel, the wave ballots.
struct WaveLanes {
	int lane;
	__device__ __forceinline__ uint64_t Body(const cvxb::ContactsColumnJob &J, int32_t yTop, uint64_t among) const
	{
		return __ballot(((among >> lane) & 1ull) != 0ull && cvxb::ContactsLaneVoxel(J, yTop - lane));
	}
};

__device__ __forceinline__ void WalkJob(const Args &A, uint32_t job, int lane)
{
	const cvxi::WaveUniform U;
	int32_t p = 0, within = A.pairCount; // the last p with prefix[p] <= job: 64 probes a round
	while (within > 1) {
		const int32_t probe = cvxb::PairSearchProbe(p, within, lane);
		cvxb::PairSearchNarrow(&p, &within, __ballot(probe >= 0 && A.prefix[probe >= 0 ? probe : 0] <= job));
	}
	p = U(p);
	const uint32_t column = job - (uint32_t)U((int32_t)A.prefix[p]);
	const uint32_t best = cvxb::PairSweepJob(U, WaveLanes{ lane }, A.models, A.instances, A.pairs, A.motions, p, column);
	if (lane == 0 && best != cvxb::kSweepNone) { atomicMin(A.first + p, best); }
}

__global__ __launch_bounds__(kThreads) void pair_sweep_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.jobs, kWaves, [&](uint64_t at, int lane) { WalkJob(A, (uint32_t)at, lane); });
}

// Both calls: `device` says where the models' arrays and `contacts` live.
static int PairSweep(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                     const int32_t *motions, int pairCount, cvxm_pair_sweep_result *sweeps, cvxp_pair_result *contacts, bool device, cvxm_pair_sweeps_summary *summary,
                     float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[200];
	if (!cvxb::PairSweepValidate(models, modelCount, instances, instanceCount, pairs, motions, pairCount, sweeps, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	std::vector<uint32_t> prefix((size_t)pairCount + 1), first((size_t)pairCount);
	const int64_t jobs = cvxb::PairSweepJobs(instances, pairs, motions, pairCount, prefix.data());
	if (jobs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the columns of the moving bodies that can come over the other body sum to 2^31 - 1 or more jobs", call); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));

	// phase 1 (the vectors above outlive D: freeing the device blocks waits for a copy still under way)
	std::vector<cvxm_pair_sweep_result> out((size_t)pairCount);
	std::vector<int32_t> at(3 * (size_t)pairCount);
	cvxi::ModelStaging staging(models, modelCount, device);
	cvxm_pair_sweeps_summary totals{ 0, 0, jobs, 0 };
	float ms = 0.f;
	{
		cvxi::DeviceCall D(ctx, call);
		uint8_t *scratch = nullptr;
		hipError_t e = staging.Allocate(D);
		if (e != hipSuccess) { return D.Fail(e); }
		cvxi::ScratchLayout carve;
		const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance), pairsBytes = (size_t)pairCount * 8,
		             motionsBytes = (size_t)pairCount * 12, prefixBytes = prefix.size() * 4, firstBytes = first.size() * 4;
		const size_t oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oPairs = carve(pairsBytes), oMotions = carve(motionsBytes), oPrefix = carve(prefixBytes),
		             oFirst = carve(firstBytes);
		Args A{};
		e = D.Allocate(&scratch, carve.bytes);
		if (e == hipSuccess) { e = D.Begin(); }
		if (e == hipSuccess) { e = staging.Enqueue(ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPairs, pairs, pairsBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oMotions, motions, motionsBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPrefix, prefix.data(), prefixBytes, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemsetAsync(scratch + oFirst, 0xFF, firstBytes, ctx->stream); }
		if (e == hipSuccess && jobs > 0) { // (a call of pairs that all pass each other by has none)
			A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
			A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
			A.pairs = reinterpret_cast<const int32_t *>(scratch + oPairs);
			A.motions = reinterpret_cast<const int32_t *>(scratch + oMotions);
			A.prefix = reinterpret_cast<const uint32_t *>(scratch + oPrefix);
			A.first = reinterpret_cast<uint32_t *>(scratch + oFirst);
			A.pairCount = pairCount;
			A.jobs = (uint32_t)jobs;
			hipLaunchKernelGGL(pair_sweep_kernel, dim3(std::min(cvxi::Grid((size_t)jobs, kWaves), kMaxWorkgroups)), dim3(kThreads), 0, ctx->stream, A);
			e = hipGetLastError();
		}
		if (e == hipSuccess) { e = hipMemcpyAsync(first.data(), scratch + oFirst, firstBytes, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = D.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
		ms = D.Ms();

		// phase 2 (inside D's life: the staged arrays are its block)
		for (int p = 0; p < pairCount; p++) {
			out[p] = cvxb::PairSweepResultOf(motions + 3 * (size_t)p, first[p], pairs[2 * p], pairs[2 * p + 1]);
			totals.hits += out[p].sweep.hit >= 0 ? 1 : 0;
			totals.startsSolid += out[p].sweep.hit == 0 ? 1 : 0;
			std::memcpy(&at[3 * (size_t)p], out[p].sweep.at, 12);
		}
		if (contacts) {
			float second = 0.f;
			// (inside the limits: I_a + v is, and `at` lies between 0 and v on every axis)
			const int code = cvxi::PairContacts(ctx, call, staging.descriptors.data(), modelCount, instances, instanceCount, pairs, pairCount, at.data(), contacts, nullptr, 0, device,
			                                    true, nullptr, &second);
			if (code != CVX_OK) { return code; }
			ms += second;
		}
	}
	// (nothing is handed out to the host before the call can no longer fail)
	std::memcpy(sweeps, out.data(), out.size() * sizeof(cvxm_pair_sweep_result));
	if (summary) { *summary = totals; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // namespace cvxpairsweep

extern "C" {

int cvxm_pair_sweep(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                    const int32_t *motions, int pairCount, cvxm_pair_sweep_result *sweeps, cvxp_pair_result *contacts, cvxm_pair_sweeps_summary *summary, float *outDeviceMs)
{
	return cvxpairsweep::PairSweep(ctx, "cvxm_pair_sweep", models, modelCount, instances, instanceCount, pairs, motions, pairCount, sweeps, contacts, false, summary, outDeviceMs);
}

int cvxm_pair_sweep_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                           const int32_t *motions, int pairCount, cvxm_pair_sweep_result *sweeps, cvxp_pair_result *contactsDevice, cvxm_pair_sweeps_summary *summary,
                           float *outDeviceMs)
{
	return cvxpairsweep::PairSweep(ctx, "cvxm_pair_sweep_device", models, modelCount, instances, instanceCount, pairs, motions, pairCount, sweeps, contactsDevice, true,
	                               summary, outDeviceMs);
}

} // extern "C"
