// cvx_pair_contacts.hip -- libcpuvox_gpu.so, where placed voxel models touch each other (cvxp_model_contacts, cvxp_model_contacts_device,
// cvxp_box_pairs, cvxp_pair_response).  See include/cpuvox_gpu_pair_contacts.h for the contract and cvx_pair_contacts.h for the rules.
//
// The shape is cvx_contacts.hip's, with a second body in the place of the world.  A WAVE per (pair, column of X_p) job (beyond 2^18 jobs the
// waves take them in turn), jobs in the list's order (pair, then x, then z); the host uploads the prefix of the footprints of X_p and a wave
// finds its pair with a wave-uniform search of it, 64 probes a round (pairs with an empty X_p have no job and are never landed on).  BOTH bodies' column
// jobs live in scalar registers (cvxb::PairBodyJobOf through readfirstlane).  The lanes are the 64 voxels of a step, top down:
//   1. count  every lane maps its voxel into both models and gathers both voxels: two ballots, A and B; a step whose A & B is empty ends there.
//             The -Y / +Y faces come from the neighbouring lanes' bits of each body's own ballot and that body at the two voxels beyond the
//             step's ends.  The side faces are computed in overlap lanes only: for each of the four neighbour columns, one at a time, a scalar
//             column part per body, then the map's finish and one gather per lane.  Counts and face sums come from ballots on the scalar side;
//             only the sum of y is kept per lane and reduced once.  The wave then issues ONE set of integer atomics on its pair's result, a
//             lane each (64-bit adds, 32-bit min / max for the box).  With a list asked for, it also leaves the job's points.
//   2. finish (cvxi::FinishResults, a thread per 64 pairs: 65536 in all): firstPoint, the box as [min, max) or zeros, the summary.
//   3. write  (only with pointCapacity > 0): the same walk writes each point at its job's offset + the points of the steps above + the lanes
//             below in the ballot (lane order is descending y).
// No LDS in the walk, no float.  No world is read: the calls work on a context with nothing uploaded.  The host's side is cvxi::RunPointsCall
// (cvx_model_call.hip), a unit being a pair.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "cvx_model_call.h"
#include "cvx_pair_contacts.h"
#include "cvx_sweep.h"

using cvxi::Fail;

namespace cvxpairs {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // of the two walks: 2^18 waves
static_assert(sizeof(cvxp_pairs_summary) == 4 * sizeof(int64_t) && offsetof(cvxp_pairs_summary, points) == 2 * sizeof(int64_t), "the summary as cvxi::PointsCall takes it");

// the 64-bit words of a result the count kernel adds to, a lane each
static_assert(offsetof(cvxp_pair_result, overlap) == 0 && offsetof(cvxp_pair_result, points) == 8 && offsetof(cvxp_pair_result, sum) == 24 &&
              offsetof(cvxp_pair_result, pushA) == 48 && offsetof(cvxp_pair_result, pushB) == 72 && sizeof(cvxp_pair_result) == 144 && sizeof(cvxp_pair_point) == 32,
              "the lanes' atomics address the result by word");

struct Args {
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	const int32_t *pairs;                // pairCount x 2
	const uint32_t *prefix;              // pairCount + 1: the jobs before every pair
	int pairCount;
	uint32_t jobs;
	cvxp_pair_result *results;
	uint32_t *counts;                    // null, or jobs + 1: the points of every job (-> its first point after the scan)
	cvxp_pair_point *points;             // write: the list, entries below `limit`
	uint32_t limit;
	cvxp_pairs_summary *summary;
	const int32_t *names;                // null, or pairCount: the `a` every result is to carry (cvxi::PairContacts with offsets)
};

// The model's colour word of the image of voxel y of the job's column.
__device__ __forceinline__ uint32_t ColourAt(const cvxb::ContactsColumnJob &J, int32_t y)
{
	const int64_t s[3] = { cvxb::ModelMapFinish(J.part[0], J.m1[0], y), cvxb::ModelMapFinish(J.part[1], J.m1[1], y), cvxb::ModelMapFinish(J.part[2], J.m1[2], y) };
	return cvxb::PairModelColour(J.M, s);
}

// The wave's walk of job `job`.  kWrite false: the job's sums into its pair's result (and its points into A.counts); true: its points into the
// list from entry `first` on.
template <bool kWrite>
__device__ __forceinline__ void WalkJob(const Args &A, uint32_t job, int lane, uint32_t first)
{
	const cvxi::WaveUniform U;
	int32_t p = 0, within = A.pairCount; // the last p with prefix[p] <= job: 64 probes a round
	while (within > 1) {
		const int32_t probe = cvxb::PairSearchProbe(p, within, lane);
		cvxb::PairSearchNarrow(&p, &within, __ballot(probe >= 0 && A.prefix[probe >= 0 ? probe : 0] <= job));
	}
	p = U(p);
	const cvx_model_instance &Ia = A.instances[U(A.pairs[2 * p])], &Ib = A.instances[U(A.pairs[2 * p + 1])];
	// X_p (not empty: the pair has a job) on the scalar side
	const int32_t ax0 = U(Ia.boxMin[0]), bx0 = U(Ib.boxMin[0]), ay0 = U(Ia.boxMin[1]), by0 = U(Ib.boxMin[1]), az0 = U(Ia.boxMin[2]), bz0 = U(Ib.boxMin[2]);
	const int32_t ay1 = U(Ia.boxMax[1]), by1 = U(Ib.boxMax[1]), az1 = U(Ia.boxMax[2]), bz1 = U(Ib.boxMax[2]);
	const int32_t x0 = ax0 > bx0 ? ax0 : bx0, y0 = ay0 > by0 ? ay0 : by0, z0 = az0 > bz0 ? az0 : bz0, y1 = ay1 < by1 ? ay1 : by1, z1 = az1 < bz1 ? az1 : bz1;
	const uint32_t sizeZ = (uint32_t)(z1 - z0), column = job - A.prefix[p];
	const int32_t cx = x0 + (int32_t)(column / sizeZ), cz = z0 + (int32_t)(column % sizeZ);
	const cvxb::PairBodyJob Ja = cvxb::PairBodyJobOf(U, A.models, Ia, cx, cz), Jb = cvxb::PairBodyJobOf(U, A.models, Ib, cx, cz);
	cvxb::PairColumnSums S;
	uint64_t ySum = 0u;  // this lane's overlap voxels: the sum of y - origin.y
	uint32_t at = first; // write: the list entry of the step's first point
	int32_t top, low;
	cvxb::PairStepRange(Ja, Jb, y0, y1, &top, &low);
	for (int32_t yTop = top; yTop >= low; yTop -= CVX_WAVE) {
		const int32_t y = yTop - lane;
		const uint64_t inA = __ballot(cvxb::ContactsLaneVoxel(Ja.J, y)), inB = __ballot(cvxb::ContactsLaneVoxel(Jb.J, y));
		const uint64_t overlap = inA & inB;
		if (overlap == 0ull) { continue; } // (two maps and two gathers)
		const bool mine = ((overlap >> lane) & 1ull) != 0ull;
		const bool aboveA = cvxb::ContactsLaneVoxel(Ja.J, yTop + 1), belowA = cvxb::ContactsLaneVoxel(Ja.J, yTop - CVX_WAVE);
		const bool aboveB = cvxb::ContactsLaneVoxel(Jb.J, yTop + 1), belowB = cvxb::ContactsLaneVoxel(Jb.J, yTop - CVX_WAVE);
		int facesA = 0, facesB = 0;
		if (mine) {
			facesA = cvxb::PairLaneSideFaces(Ja, y) | cvxb::ContactsLaneEndFaces(inA, aboveA, belowA, lane);
			facesB = cvxb::PairLaneSideFaces(Jb, y) | cvxb::ContactsLaneEndFaces(inB, aboveB, belowB, lane);
		}
		const uint64_t points = __ballot((facesA | facesB) != 0);
		if (kWrite) {
			const uint32_t entry = at + cvxi::LanesBelow(points);
			if ((facesA | facesB) != 0 && entry < A.limit) { A.points[entry] = cvxp_pair_point{ { cx, y, cz }, p, facesA, facesB, ColourAt(Ja.J, y), ColourAt(Jb.J, y) }; }
			at += (uint32_t)__popcll(points);
			if (at >= A.limit) { return; }
		} else {
			uint64_t faceA[6], faceB[6];
			for (int f = 0; f < 6; f++) {
				faceA[f] = __ballot(((facesA >> f) & 1) != 0);
				faceB[f] = __ballot(((facesB >> f) & 1) != 0);
			}
			cvxb::PairStep(S, overlap, points, faceA, faceB, yTop);
			if (mine) { ySum += (uint64_t)(uint32_t)(y - y0); }
		}
	}
	if (kWrite) { return; }
	if (A.counts && lane == 0) { A.counts[job] = (uint32_t)S.points; }
	if (S.overlap == 0) { return; }
	// what cvxb::PairColumnDone adds, a lane per word of the result
	cvxp_pair_result *r = A.results + p;
	const uint64_t ySumAll = cvxi::WaveReduce((unsigned long long)ySum, [](unsigned long long a, unsigned long long b) { return a + b; });
	if (lane < 11) {
		const uint64_t value = lane == 0   ? (uint64_t)S.overlap
		                       : lane == 1 ? (uint64_t)S.points
		                       : lane == 2 ? (uint64_t)S.overlap * (uint64_t)((int64_t)cx - x0)
		                       : lane == 3 ? ySumAll
		                       : lane == 4 ? (uint64_t)S.overlap * (uint64_t)((int64_t)cz - z0)
		                       : lane < 8  ? (uint64_t)(int64_t)(lane == 5 ? S.pushA[0] : (lane == 6 ? S.pushA[1] : S.pushA[2]))
		                                   : (uint64_t)(int64_t)(lane == 8 ? S.pushB[0] : (lane == 9 ? S.pushB[1] : S.pushB[2]));
		unsigned long long *word = reinterpret_cast<unsigned long long *>(r) + (lane < 2 ? lane : lane + 1); // (firstPoint lies between points and sum)
		if (value != 0u) { atomicAdd(word, (unsigned long long)value); }
	} else if (lane < 14) {
		const int a = lane - 11;
		atomicMin(&r->min[a], a == 0 ? cx : (a == 1 ? S.yMin : cz));
	} else if (lane < 17) {
		const int a = lane - 14;
		atomicMax(&r->max[a], a == 0 ? cx : (a == 1 ? S.yMax : cz));
	}
}

__global__ __launch_bounds__(kThreads) void pairs_init_kernel(Args A)
{
	const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
	if (p >= A.pairCount) { return; }
	const int32_t a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
	cvxb::PairResultInit(A.instances[a], A.instances[b], a, b, A.results + p);
}

// Both walks: the launch's waves take the jobs in turn (cvxi::ForEachWaveJob: a launch has at most kMaxWorkgroups workgroups, whatever the jobs).
__global__ __launch_bounds__(kThreads) void pairs_count_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.jobs, kWaves, [&](uint64_t at, int lane) { WalkJob<false>(A, (uint32_t)at, lane, 0u); });
}

// The list holds min(A.limit, the points found) entries: the finish kernel has left the points in the summary, and the offsets are good only
// below 2^31 points (the host then fails the call).
__global__ __launch_bounds__(kThreads) void pairs_write_kernel(Args A)
{
	const uint64_t found = (uint64_t)A.summary->points;
	if (found >= (1ull << 31)) { return; }
	A.limit = found < A.limit ? (uint32_t)found : A.limit;
	cvxi::ForEachWaveJob(A.jobs, kWaves, [&](uint64_t at, int lane) {
		const uint32_t job = (uint32_t)at, first = A.counts[job];
		if (first >= A.limit || A.counts[job + 1u] == first) { return; }
		WalkJob<true>(A, job, lane, first);
	});
}

// One workgroup (cvxi::FinishResults): firstPoint, the box, the summary.
__global__ __launch_bounds__(cvxi::kFinishThreads) void pairs_finish_kernel(Args A)
{
	unsigned long long points;
	const unsigned long long *totals = cvxi::FinishResults<CVXP_MAX_PAIRS, 2>(
		A.results, A.pairCount, [](cvxp_pair_result *r) { cvxb::PairResultFinish(r); },
		[](const cvxp_pair_result &r, unsigned long long *sums) { // touching, overlap
			sums[0] += r.overlap > 0 ? 1ull : 0ull;
			sums[1] += (unsigned long long)r.overlap;
		},
		&points);
	if (threadIdx.x == 0) { *A.summary = cvxp_pairs_summary{ (int64_t)totals[0], (int64_t)totals[1], (int64_t)points, (int64_t)A.jobs }; }
}

// With offsets: every result's `a` back to the pair's own, as given (the walk ran on the moved copy behind the caller's instances).
__global__ __launch_bounds__(kThreads) void pairs_name_kernel(Args A)
{
	const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
	if (p < A.pairCount) { A.results[p].a = A.names[p]; }
}

} // namespace cvxpairs

// Both calls (and cvx_pair_sweep.hip's second phase: cvx_model_call.h): `device` says where the models' arrays, `results` and `points` live.
// With `offsets`, body a of pair p is I_a + offsets[p] for that pair alone: the moved instances (cvxb::SweepInstanceMoved, the caller has checked
// that they stay inside the limits) go behind the caller's own, one a pair, the walk's pairs name them, and pairs_name_kernel writes the pair as
// given into the results.  Without, nothing of that is built or launched.
int cvxi::PairContacts(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                       const int32_t *pairs, int pairCount, const int32_t *offsets, cvxp_pair_result *results, cvxp_pair_point *points, int64_t pointCapacity, bool device,
                       bool modelsStaged, cvxp_pairs_summary *summary, float *outDeviceMs)
{
	using namespace cvxpairs;
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::PairsValidate(models, modelCount, instances, instanceCount, pairs, pairCount, results, points, pointCapacity, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	std::vector<cvx_model_instance> placed;
	std::vector<int32_t> named; // the walk's pairs, then the names
	if (offsets) {
		placed.assign(instances, instances + instanceCount);
		placed.resize((size_t)instanceCount + (size_t)pairCount);
		named.resize(3 * (size_t)pairCount);
		for (int p = 0; p < pairCount; p++) {
			if (!cvxb::SweepInstanceMoved(instances[pairs[2 * p]], offsets + 3 * (size_t)p, &placed[(size_t)instanceCount + p])) {
				return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: pair %d: the moved instance leaves the limits", call, p);
			}
			named[2 * (size_t)p] = instanceCount + p;
			named[2 * (size_t)p + 1] = pairs[2 * p + 1];
			named[2 * (size_t)pairCount + p] = pairs[2 * p];
		}
		instances = placed.data();
		instanceCount += pairCount;
		pairs = named.data();
	}
	std::vector<uint32_t> prefix((size_t)pairCount + 1);
	const int64_t jobs = cvxb::PairJobs(instances, pairs, pairCount, prefix.data());
	if (jobs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the pairs' common footprints sum to 2^31 - 1 or more (pair, column) jobs", call); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));

	Args A{};
	A.pairCount = pairCount;
	A.jobs = (uint32_t)jobs;
	const dim3 walk(std::min(cvxi::Grid((size_t)jobs, kWaves), kMaxWorkgroups)), block(kThreads);
	const cvxi::PointsCall C{ call, models, modelCount, instances, instanceCount, prefix.data(), pairCount, jobs, pairs, (size_t)pairCount * (offsets ? 12 : 8),
		                      sizeof(cvxp_pair_result), sizeof(cvxp_pair_point), results, points, pointCapacity, device, reinterpret_cast<int64_t *>(summary), modelsStaged };
	return cvxi::RunPointsCall(
		ctx, C,
		[&](const cvxi::PointsJob &J) {
			A.models = J.models;
			A.instances = J.instances;
			A.pairs = static_cast<const int32_t *>(J.extra);
			A.prefix = J.prefix;
			A.results = static_cast<cvxp_pair_result *>(J.results);
			A.counts = J.counts;
			A.summary = reinterpret_cast<cvxp_pairs_summary *>(J.summary);
			hipLaunchKernelGGL(pairs_init_kernel, dim3(cvxi::Grid((size_t)pairCount)), block, 0, ctx->stream, A);
			if (jobs > 0) { hipLaunchKernelGGL(pairs_count_kernel, walk, block, 0, ctx->stream, A); } // (a call of pairs that all miss has none)
			hipLaunchKernelGGL(pairs_finish_kernel, dim3(1), dim3(cvxi::kFinishThreads), 0, ctx->stream, A);
			if (offsets) {
				A.names = A.pairs + 2 * (size_t)pairCount;
				hipLaunchKernelGGL(pairs_name_kernel, dim3(cvxi::Grid((size_t)pairCount)), block, 0, ctx->stream, A);
			}
			return hipSuccess;
		},
		[&](const cvxi::PointsJob &J) {
			A.points = static_cast<cvxp_pair_point *>(J.points);
			A.limit = J.limit;
			hipLaunchKernelGGL(pairs_write_kernel, walk, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

extern "C" {

int cvxp_model_contacts(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                        int pairCount, cvxp_pair_result *results, cvxp_pair_point *points, int64_t pointCapacity, cvxp_pairs_summary *summary, float *outDeviceMs)
{
	return cvxi::PairContacts(ctx, "cvxp_model_contacts", models, modelCount, instances, instanceCount, pairs, pairCount, nullptr, results, points, pointCapacity, false, false,
	                          summary, outDeviceMs);
}

int cvxp_model_contacts_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                               int pairCount, cvxp_pair_result *resultsDevice, cvxp_pair_point *pointsDevice, int64_t pointCapacity, cvxp_pairs_summary *summary,
                               float *outDeviceMs)
{
	return cvxi::PairContacts(ctx, "cvxp_model_contacts_device", models, modelCount, instances, instanceCount, pairs, pairCount, nullptr, resultsDevice, pointsDevice,
	                          pointCapacity, true, false, summary, outDeviceMs);
}

int cvxp_box_pairs(const cvx_model_instance *instances, int instanceCount, int margin, int32_t *pairs, int64_t pairCapacity, int64_t *found)
{
	return cvxb::BoxPairs(instances, instanceCount, margin, pairs, pairCapacity, found) ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

int cvxp_pair_response(const cvxp_pair_result *r, int which, double centre[3], double normal[3], double *depth)
{
	return cvxb::PairResponse(r, which, centre, normal, depth) ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

} // extern "C"
