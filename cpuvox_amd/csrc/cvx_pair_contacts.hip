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
//   2. finish (one workgroup, a thread per 64 pairs: 65536 in all): firstPoint by a scan of the pairs' points, the box as [min, max) or zeros,
//             the summary.  ONE copy brings the summary to the host.
//   3. write  (only with pointCapacity > 0): cvxi::ExclusiveScan turns the jobs' points into offsets; the same walk writes each point at
//             offset + the points of the steps above + the lanes below in the ballot (lane order is descending y).  A device list is
//             enqueued behind the finish, before the one synchronisation; a host list is sized by the points found, after it.
// No LDS in the walk, no float.  No world is read: the calls work on a context with nothing uploaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_pair_contacts.h"

using cvxi::Fail;

namespace cvxpairs {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // of the two walks: 2^18 waves
constexpr int kFinishThreads = 1024, kFinishEach = CVXP_MAX_PAIRS / kFinishThreads;
static_assert(kFinishThreads * kFinishEach == CVXP_MAX_PAIRS, "the finish kernel's one workgroup covers every pair");

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
};

__device__ __forceinline__ uint32_t LanesBelow(uint64_t mask) // the set bits of `mask` below this lane
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

struct WaveUniform { // cvxb::PairBodyJobOf's Uniform: the value is the same in every lane, keep it in a scalar register
	__device__ __forceinline__ int32_t operator()(int32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
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
	const WaveUniform U;
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
			const uint32_t entry = at + LanesBelow(points);
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

// Both walks: the launch's waves take the jobs in turn (a launch has at most kMaxWorkgroups workgroups, whatever the jobs).
__global__ __launch_bounds__(kThreads) void pairs_count_kernel(Args A)
{
	const uint32_t waves = gridDim.x * (uint32_t)kWaves;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	for (uint64_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / CVX_WAVE)); at < A.jobs; at += waves) {
		WalkJob<false>(A, (uint32_t)at, lane, 0u);
	}
}

// The list holds min(A.limit, the points found) entries: the finish kernel has left the points in the summary, and the offsets are good only
// below 2^31 points (the host then fails the call).
__global__ __launch_bounds__(kThreads) void pairs_write_kernel(Args A)
{
	const uint64_t found = (uint64_t)A.summary->points;
	if (found >= (1ull << 31)) { return; }
	A.limit = found < A.limit ? (uint32_t)found : A.limit;
	const uint32_t waves = gridDim.x * (uint32_t)kWaves;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	for (uint64_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / CVX_WAVE)); at < A.jobs; at += waves) {
		const uint32_t job = (uint32_t)at, first = A.counts[job];
		if (first >= A.limit || A.counts[job + 1u] == first) { continue; }
		WalkJob<true>(A, job, lane, first);
	}
}

// One workgroup.  Thread t finishes pairs kFinishEach * t ..: firstPoint from an inclusive scan of the threads' points, the box, the summary.
__global__ __launch_bounds__(kFinishThreads) void pairs_finish_kernel(Args A)
{
	__shared__ unsigned long long scan[kFinishThreads];
	__shared__ unsigned long long totals[2]; // touching, overlap
	const int t = (int)threadIdx.x;
	if (t < 2) { totals[t] = 0ull; }
	unsigned long long mine = 0ull;
	for (int j = 0; j < kFinishEach; j++) {
		const int p = kFinishEach * t + j;
		if (p < A.pairCount) { mine += (unsigned long long)A.results[p].points; }
	}
	scan[t] = mine;
	__syncthreads();
	for (int d = 1; d < kFinishThreads; d <<= 1) {
		const unsigned long long before = t >= d ? scan[t - d] : 0ull;
		__syncthreads();
		scan[t] += before;
		__syncthreads();
	}
	unsigned long long firstPoint = scan[t] - mine, touching = 0ull, overlap = 0ull;
	for (int j = 0; j < kFinishEach; j++) {
		const int p = kFinishEach * t + j;
		if (p >= A.pairCount) { break; }
		cvxp_pair_result *r = A.results + p;
		r->firstPoint = (int64_t)firstPoint;
		firstPoint += (unsigned long long)r->points;
		cvxb::PairResultFinish(r);
		touching += r->overlap > 0 ? 1ull : 0ull;
		overlap += (unsigned long long)r->overlap;
	}
	if (touching != 0ull) {
		atomicAdd(&totals[0], touching);
		atomicAdd(&totals[1], overlap);
	}
	__syncthreads();
	if (t == 0) { *A.summary = cvxp_pairs_summary{ (int64_t)totals[0], (int64_t)totals[1], (int64_t)scan[kFinishThreads - 1], (int64_t)A.jobs }; }
}

static unsigned Grid(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
static unsigned WalkGrid(int64_t jobs) { return std::min(Grid((size_t)jobs, kWaves), kMaxWorkgroups); }
static size_t Align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// Both calls: `device` says where the models' arrays, `results` and `points` live.
static int ModelContacts(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                         const int32_t *pairs, int pairCount, cvxp_pair_result *results, cvxp_pair_point *points, int64_t pointCapacity, bool device,
                         cvxp_pairs_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::PairsValidate(models, modelCount, instances, instanceCount, pairs, pairCount, results, points, pointCapacity, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	std::vector<uint32_t> prefix((size_t)pairCount + 1);
	const int64_t jobs = cvxb::PairJobs(instances, pairs, pairCount, prefix.data());
	if (jobs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the pairs' common footprints sum to 2^31 - 1 or more (pair, column) jobs", call); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));

	// (these outlive D: freeing the device blocks waits for a copy still under way)
	std::vector<cvxp_pair_result> backResults;
	std::vector<cvxp_pair_point> backPoints;
	std::vector<cvx_model> deviceModels(models, models + modelCount);
	cvxp_pairs_summary host{};
	cvxi::DeviceCall D(ctx, call);
	uint8_t *arrays = nullptr, *scratch = nullptr, *list = nullptr;
	struct Upload {
		size_t at, bytes;
		const void *from;
	};
	std::vector<Upload> uploads;
	hipError_t e = hipSuccess;
	if (!device) { // host arrays: a device copy of them
		size_t total = 0;
		for (int k = 0; k < modelCount; k++) {
			const size_t n = (size_t)models[k].size[0] * (size_t)models[k].size[1] * (size_t)models[k].size[2];
			if (models[k].argb) {
				uploads.push_back(Upload{ total, n * 4, models[k].argb });
				total += Align16(n * 4);
			}
			if (models[k].solid) {
				uploads.push_back(Upload{ total, n, models[k].solid });
				total += Align16(n);
			}
		}
		e = D.Allocate(&arrays, total);
		if (e != hipSuccess) { return D.Fail(e); }
		size_t u = 0;
		for (int k = 0; k < modelCount; k++) {
			if (models[k].argb) { deviceModels[k].argb = reinterpret_cast<const uint32_t *>(arrays + uploads[u++].at); }
			if (models[k].solid) { deviceModels[k].solid = arrays + uploads[u++].at; }
		}
		backResults.resize((size_t)pairCount);
	}
	const bool listing = pointCapacity > 0;
	cvxi::ScratchLayout carve;
	const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance),
	             pairsBytes = (size_t)pairCount * 8, prefixBytes = prefix.size() * 4, resultsBytes = (size_t)pairCount * sizeof(cvxp_pair_result);
	const size_t chunks = listing ? ((size_t)jobs + 1 + cvxi::ScanChunk() - 1) / cvxi::ScanChunk() : 0;
	const size_t oSummary = carve(sizeof host), oTotal = carve(8), oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oPairs = carve(pairsBytes),
	             oPrefix = carve(prefixBytes), oResults = carve(device ? 0 : resultsBytes), oCounts = carve(listing ? ((size_t)jobs + 1) * 4 : 0), oChunks = carve(chunks * 8);
	Args A{};
	e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	for (const Upload &u : uploads) {
		if (e == hipSuccess) { e = hipMemcpyAsync(arrays + u.at, u.from, u.bytes, hipMemcpyHostToDevice, ctx->stream); }
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, deviceModels.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPairs, pairs, pairsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPrefix, prefix.data(), prefixBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess && listing) { e = hipMemsetAsync(scratch + oCounts + (size_t)jobs * 4, 0, 4, ctx->stream); } // (the scan leaves the total behind the last job's offset)
	if (e == hipSuccess) {
		A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
		A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
		A.pairs = reinterpret_cast<const int32_t *>(scratch + oPairs);
		A.prefix = reinterpret_cast<const uint32_t *>(scratch + oPrefix);
		A.pairCount = pairCount;
		A.jobs = (uint32_t)jobs;
		A.results = device ? results : reinterpret_cast<cvxp_pair_result *>(scratch + oResults);
		A.counts = listing ? reinterpret_cast<uint32_t *>(scratch + oCounts) : nullptr;
		A.summary = reinterpret_cast<cvxp_pairs_summary *>(scratch + oSummary);
		hipLaunchKernelGGL(pairs_init_kernel, dim3(Grid((size_t)pairCount, kThreads)), dim3(kThreads), 0, ctx->stream, A);
		if (jobs > 0) { hipLaunchKernelGGL(pairs_count_kernel, dim3(WalkGrid(jobs)), dim3(kThreads), 0, ctx->stream, A); } // (a call of pairs that all miss has none)
		hipLaunchKernelGGL(pairs_finish_kernel, dim3(1), dim3(kFinishThreads), 0, ctx->stream, A);
		e = hipGetLastError();
	}
	// the list: the scan of the jobs' points and the second walk (its kernel cuts the list at the points found)
	auto list_points = [&](cvxp_pair_point *into, uint32_t limit) {
		if (jobs == 0) { return hipSuccess; }
		A.points = into;
		A.limit = limit;
		cvxi::ExclusiveScan(ctx->stream, A.counts, (int)(jobs + 1), reinterpret_cast<unsigned long long *>(scratch + oChunks), reinterpret_cast<unsigned long long *>(scratch + oTotal));
		hipLaunchKernelGGL(pairs_write_kernel, dim3(WalkGrid(jobs)), dim3(kThreads), 0, ctx->stream, A);
		return hipGetLastError();
	};
	// A device list needs nothing from the host: everything is enqueued before the one synchronisation.  A host list is sized by the points found.
	const bool staged = listing && !device;
	if (e == hipSuccess && listing && device) { e = list_points(points, (uint32_t)std::min<int64_t>(pointCapacity, 0x7FFFFFFF)); }
	if (e == hipSuccess) { e = hipMemcpyAsync(&host, A.summary, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !device) { e = hipMemcpyAsync(backResults.data(), A.results, resultsBytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !staged) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (listing && host.points >= ((int64_t)1 << 31)) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the contacts hold %lld points", call, (long long)host.points); }
	if (staged) {
		const size_t wanted = (size_t)std::min<int64_t>(host.points, pointCapacity);
		if (wanted) {
			backPoints.resize(wanted);
			e = D.Allocate(&list, wanted * sizeof(cvxp_pair_point));
			if (e == hipSuccess) { e = list_points(reinterpret_cast<cvxp_pair_point *>(list), (uint32_t)wanted); }
			if (e == hipSuccess) { e = hipMemcpyAsync(backPoints.data(), list, wanted * sizeof(cvxp_pair_point), hipMemcpyDeviceToHost, ctx->stream); }
		}
		if (e == hipSuccess) { e = D.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
	}
	// (nothing is handed out to the host before the call can no longer fail)
	if (!backResults.empty()) { std::memcpy(results, backResults.data(), resultsBytes); }
	if (!backPoints.empty()) { std::memcpy(points, backPoints.data(), backPoints.size() * sizeof(cvxp_pair_point)); }
	if (summary) { *summary = host; }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxpairs

extern "C" {

int cvxp_model_contacts(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                        int pairCount, cvxp_pair_result *results, cvxp_pair_point *points, int64_t pointCapacity, cvxp_pairs_summary *summary, float *outDeviceMs)
{
	return cvxpairs::ModelContacts(ctx, "cvxp_model_contacts", models, modelCount, instances, instanceCount, pairs, pairCount, results, points, pointCapacity, false, summary,
	                               outDeviceMs);
}

int cvxp_model_contacts_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                               int pairCount, cvxp_pair_result *resultsDevice, cvxp_pair_point *pointsDevice, int64_t pointCapacity, cvxp_pairs_summary *summary,
                               float *outDeviceMs)
{
	return cvxpairs::ModelContacts(ctx, "cvxp_model_contacts_device", models, modelCount, instances, instanceCount, pairs, pairCount, resultsDevice, pointsDevice,
	                               pointCapacity, true, summary, outDeviceMs);
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
