// cvx_contacts.hip -- libcpuvox_gpu.so, where placed voxel models touch the device-resident world (cvxc_world_contacts,
// cvxc_world_contacts_device, cvxc_contact_response).  See include/cpuvox_gpu_contacts.h for the contract and cvx_contacts.h for the rules.
//
// A WAVE per (instance, column of its box) pair (beyond 2^18 pairs the waves take them in turn), pairs in the list's order (instance, then x, then z); the host uploads the prefix of the boxes'
// footprints and a wave finds its instance with a wave-uniform binary search of it.  The map's column part, the box and the model's descriptor
// live in scalar registers (cvxb::ContactsColumnJobOf through readfirstlane).  The lanes are the 64 voxels of a step, top down:
//   1. count  every lane maps its voxel and gathers the model's voxel; a step whose ballot of SET voxels is empty ends there.  Otherwise every
//             lane finds its voxel in the centre column's runs and, where body and world overlap, in the four neighbours' (binary searches, no
//             voxel is scanned); the -Y / +Y faces come from the neighbouring lanes' bits of the centre ballot and the two voxels beyond the
//             step's ends.  Counts, face counts and bounds come from ballots on the scalar side; only the sum of y is kept per lane and reduced
//             once.  The wave then issues ONE set of integer atomics on its instance's result, a lane each (64-bit adds, 32-bit min / max for
//             the box): integer atomics keep the bytes independent of the order.  With a list asked for, it also leaves the pair's points.
//   2. finish (one workgroup, a thread per four instances): firstPoint by a scan of the instances' points, the box as [min, max) or zeros, the
//             summary.  ONE copy brings the summary to the host.
//   3. write  (only with pointCapacity > 0): cvxi::ExclusiveScan turns the pairs' points into offsets; the same walk writes each point at
//             offset + the points of the steps above + the lanes below in the ballot (lane order is descending y).  A device list is
//             enqueued behind the finish, before the one synchronisation; a host list is sized by the points found, after it.
// No LDS in the walk.  Nothing is written to the arena.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_contacts.h"

using cvxi::Fail;

namespace cvxcontacts {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // of the two walks: 2^18 waves, some thirty times what an MI355X holds at once
constexpr int kFinishThreads = 1024, kFinishEach = CVX_MODELS_MAX_INSTANCES / kFinishThreads;
static_assert(kFinishThreads * kFinishEach == CVX_MODELS_MAX_INSTANCES, "the finish kernel's one workgroup covers every instance");

// the 64-bit words of a result the count kernel adds to, a lane each
static_assert(offsetof(cvxc_contact_result, voxels) == 0 && offsetof(cvxc_contact_result, overlap) == 8 && offsetof(cvxc_contact_result, points) == 16 &&
              offsetof(cvxc_contact_result, sum) == 32 && offsetof(cvxc_contact_result, normal) == 56 && sizeof(cvxc_contact_result) == 120,
              "the lanes' atomics address the result by word");

struct Args {
	cvxb::CopyWorld W;
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	const uint32_t *prefix;              // instanceCount + 1: the pairs before every instance
	int instanceCount;
	uint32_t pairs;
	int solidOutside;
	cvxc_contact_result *results;
	uint32_t *counts;                    // null, or pairs + 1: the points of every pair (-> its first point after the scan)
	cvxc_contact_point *points;          // write: the list, entries below `limit`
	uint32_t limit;
	cvxc_contacts_summary *summary;
};

__device__ __forceinline__ uint32_t LanesBelow(uint64_t mask) // the set bits of `mask` below this lane
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

struct WaveUniform { // cvxb::ContactsColumnJobOf's Uniform: the value is the same in every lane, keep it in a scalar register
	__device__ __forceinline__ int32_t operator()(int32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
};

// The wave's walk of pair `pair`.  kWrite false: the pair's sums into its instance's result (and its points into A.counts); true: its points
// into the list from entry `first` on.
template <bool kWrite>
__device__ __forceinline__ void WalkPair(const Args &A, uint32_t pair, int lane, uint32_t first)
{
	const WaveUniform U;
	const int k = U(cvxb::ContactsPairInstance(A.prefix, A.instanceCount, pair));
	const cvx_model_instance &I = A.instances[k];
	const int32_t x0 = U(I.boxMin[0]), z0 = U(I.boxMin[2]);
	const uint32_t sizeZ = (uint32_t)(U(I.boxMax[2]) - z0), column = pair - A.prefix[k];
	const int32_t cx = x0 + (int32_t)(column / sizeZ), cz = z0 + (int32_t)(column % sizeZ);
	const cvxb::ContactsColumnJob J = cvxb::ContactsColumnJobOf(U, A.models, I, cx, cz);
	const cvxb::DistanceColumn centre = cvxb::DistanceColumnAt(A.W, cx, cz, A.solidOutside);
	const int64_t dimY = A.W.dimY;
	cvxb::ContactsColumnSums S;
	uint64_t ySum = 0u;  // this lane's overlap voxels: the sum of y - boxMin.y
	uint32_t at = first; // write: the list entry of the step's first point
	int32_t top, low;
	cvxb::ContactsStepRange(J, &top, &low);
	for (int32_t yTop = top; yTop >= low; yTop -= CVX_WAVE) {
		const int32_t y = yTop - lane;
		const uint64_t body = __ballot(cvxb::ContactsLaneVoxel(J, y));
		if (body == 0ull) { continue; } // (the map and one gather)
		const uint64_t solid = __ballot(cvxb::ContactColumnSolid(centre, dimY, y));
		const uint64_t overlap = body & solid;
		const bool mine = ((overlap >> lane) & 1ull) != 0ull;
		int faces = 0;
		if (overlap != 0ull) {
			const bool above = cvxb::ContactColumnSolid(centre, dimY, (int64_t)yTop + 1), below = cvxb::ContactColumnSolid(centre, dimY, (int64_t)yTop - CVX_WAVE);
			if (mine) { faces = cvxb::ContactsLaneSideFaces(A.W, cx, cz, A.solidOutside, y) | cvxb::ContactsLaneEndFaces(solid, above, below, lane); }
		}
		const uint64_t points = __ballot(faces != 0);
		if (kWrite) {
			const uint32_t entry = at + LanesBelow(points);
			if (faces != 0 && entry < A.limit) { A.points[entry] = cvxc_contact_point{ { cx, y, cz }, k, faces, cvxb::ContactColour(A.W, cx, y, cz) }; }
			at += (uint32_t)__popcll(points);
			if (at >= A.limit) { return; }
		} else {
			uint64_t face[6];
			for (int f = 0; f < 6; f++) { face[f] = overlap != 0ull ? __ballot(((faces >> f) & 1) != 0) : 0ull; }
			cvxb::ContactsStep(S, body, overlap, points, face, yTop);
			if (mine) { ySum += (uint64_t)(uint32_t)(y - J.yLo); }
		}
	}
	if (kWrite) { return; }
	if (A.counts && lane == 0) { A.counts[pair] = (uint32_t)S.points; }
	// what cvxb::ContactsColumnDone adds, a lane per word of the result
	cvxc_contact_result *r = A.results + k;
	if (S.overlap == 0) {
		if (S.voxels != 0 && lane == 0) { atomicAdd(reinterpret_cast<unsigned long long *>(&r->voxels), (unsigned long long)S.voxels); }
		return;
	}
	const uint64_t ySumAll = cvxi::WaveReduce((unsigned long long)ySum, [](unsigned long long a, unsigned long long b) { return a + b; });
	if (lane < 9) {
		const uint64_t value = lane == 0   ? (uint64_t)S.voxels
		                       : lane == 1 ? (uint64_t)S.overlap
		                       : lane == 2 ? (uint64_t)S.points
		                       : lane == 3 ? (uint64_t)S.overlap * (uint64_t)((int64_t)cx - x0)
		                       : lane == 4 ? ySumAll
		                       : lane == 5 ? (uint64_t)S.overlap * (uint64_t)((int64_t)cz - z0)
		                       : lane == 6 ? (uint64_t)(int64_t)S.normal[0]
		                       : lane == 7 ? (uint64_t)(int64_t)S.normal[1]
		                                   : (uint64_t)(int64_t)S.normal[2];
		unsigned long long *word = reinterpret_cast<unsigned long long *>(r) + (lane < 3 ? lane : lane + 1); // (firstPoint lies between points and sum)
		if (value != 0u) { atomicAdd(word, (unsigned long long)value); }
	} else if (lane < 12) {
		const int a = lane - 9;
		atomicMin(&r->min[a], a == 0 ? cx : (a == 1 ? S.yMin : cz));
	} else if (lane < 15) {
		const int a = lane - 12;
		atomicMax(&r->max[a], a == 0 ? cx : (a == 1 ? S.yMax : cz));
	}
}

__global__ __launch_bounds__(kThreads) void contacts_init_kernel(Args A)
{
	const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
	if (k < A.instanceCount) { cvxb::ContactResultInit(A.instances[k], A.results + k); }
}

// Both walks: the launch's waves take the pairs in turn (a launch has at most kMaxWorkgroups workgroups, whatever the pairs).
__global__ __launch_bounds__(kThreads) void contacts_count_kernel(Args A)
{
	const uint32_t waves = gridDim.x * (uint32_t)kWaves;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	for (uint64_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / CVX_WAVE)); at < A.pairs; at += waves) {
		WalkPair<false>(A, (uint32_t)at, lane, 0u);
	}
}

// The list holds min(A.limit, the points found) entries: the finish kernel has left the points in the summary, and the offsets are good only
// below 2^31 points (the host then fails the call).
__global__ __launch_bounds__(kThreads) void contacts_write_kernel(Args A)
{
	const uint64_t found = (uint64_t)A.summary->points;
	if (found >= (1ull << 31)) { return; }
	A.limit = found < A.limit ? (uint32_t)found : A.limit;
	const uint32_t waves = gridDim.x * (uint32_t)kWaves;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	for (uint64_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + threadIdx.x / CVX_WAVE)); at < A.pairs; at += waves) {
		const uint32_t pair = (uint32_t)at, first = A.counts[pair];
		if (first >= A.limit || A.counts[pair + 1u] == first) { continue; }
		WalkPair<true>(A, pair, lane, first);
	}
}

// One workgroup.  Thread t finishes instances kFinishEach * t ..: firstPoint from an inclusive scan of the threads' points, the box, the summary.
__global__ __launch_bounds__(kFinishThreads) void contacts_finish_kernel(Args A)
{
	__shared__ unsigned long long scan[kFinishThreads];
	__shared__ unsigned long long totals[3]; // touching, overlap, voxels
	const int t = (int)threadIdx.x;
	if (t < 3) { totals[t] = 0ull; }
	unsigned long long mine = 0ull;
	for (int j = 0; j < kFinishEach; j++) {
		const int k = kFinishEach * t + j;
		if (k < A.instanceCount) { mine += (unsigned long long)A.results[k].points; }
	}
	scan[t] = mine;
	__syncthreads();
	for (int d = 1; d < kFinishThreads; d <<= 1) {
		const unsigned long long before = t >= d ? scan[t - d] : 0ull;
		__syncthreads();
		scan[t] += before;
		__syncthreads();
	}
	unsigned long long firstPoint = scan[t] - mine, touching = 0ull, overlap = 0ull, voxels = 0ull;
	for (int j = 0; j < kFinishEach; j++) {
		const int k = kFinishEach * t + j;
		if (k >= A.instanceCount) { break; }
		cvxc_contact_result *r = A.results + k;
		r->firstPoint = (int64_t)firstPoint;
		firstPoint += (unsigned long long)r->points;
		cvxb::ContactResultFinish(r);
		touching += r->overlap > 0 ? 1ull : 0ull;
		overlap += (unsigned long long)r->overlap;
		voxels += (unsigned long long)r->voxels;
	}
	if (voxels != 0ull) {
		atomicAdd(&totals[0], touching);
		atomicAdd(&totals[1], overlap);
		atomicAdd(&totals[2], voxels);
	}
	__syncthreads();
	if (t == 0) { *A.summary = cvxc_contacts_summary{ (int64_t)totals[0], (int64_t)totals[1], (int64_t)scan[kFinishThreads - 1], (int64_t)totals[2] }; }
}

static unsigned Grid(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
static unsigned WalkGrid(int64_t pairs) { return std::min(Grid((size_t)pairs, kWaves), kMaxWorkgroups); }
static size_t Align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// Both calls: `device` says where the models' arrays, `results` and `points` live.
static int Contacts(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside,
                    cvxc_contact_result *results, cvxc_contact_point *points, int64_t pointCapacity, bool device, cvxc_contacts_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::ContactsValidate(models, modelCount, instances, instanceCount, solidOutside, results, points, pointCapacity, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	if (!ctx->levelSet[0]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD 0 has not been uploaded"); }
	std::vector<uint32_t> prefix((size_t)instanceCount + 1);
	const int64_t pairs = cvxb::ContactsPairs(instances, instanceCount, prefix.data());
	if (pairs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the boxes' footprints sum to 2^31 - 1 or more (instance, column) pairs", call); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	const int rc = cvxi::SyncWorld(ctx);
	if (rc != CVX_OK) { return rc; }

	// (these outlive D: freeing the device blocks waits for a copy still under way)
	std::vector<cvxc_contact_result> backResults;
	std::vector<cvxc_contact_point> backPoints;
	std::vector<cvx_model> deviceModels(models, models + modelCount);
	cvxc_contacts_summary host{};
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
		backResults.resize((size_t)instanceCount);
	}
	const bool listing = pointCapacity > 0;
	cvxi::ScratchLayout carve;
	const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance),
	             prefixBytes = prefix.size() * 4, resultsBytes = (size_t)instanceCount * sizeof(cvxc_contact_result);
	const size_t chunks = listing ? ((size_t)pairs + 1 + cvxi::ScanChunk() - 1) / cvxi::ScanChunk() : 0;
	const size_t oSummary = carve(sizeof host), oTotal = carve(8), oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oPrefix = carve(prefixBytes),
	             oResults = carve(device ? 0 : resultsBytes), oCounts = carve(listing ? ((size_t)pairs + 1) * 4 : 0), oChunks = carve(chunks * 8);
	Args A{};
	e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	for (const Upload &u : uploads) {
		if (e == hipSuccess) { e = hipMemcpyAsync(arrays + u.at, u.from, u.bytes, hipMemcpyHostToDevice, ctx->stream); }
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, deviceModels.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPrefix, prefix.data(), prefixBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess && listing) { e = hipMemsetAsync(scratch + oCounts + (size_t)pairs * 4, 0, 4, ctx->stream); } // (the scan leaves the total behind the last pair's offset)
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
		A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
		A.prefix = reinterpret_cast<const uint32_t *>(scratch + oPrefix);
		A.instanceCount = instanceCount;
		A.pairs = (uint32_t)pairs;
		A.solidOutside = solidOutside;
		A.results = device ? results : reinterpret_cast<cvxc_contact_result *>(scratch + oResults);
		A.counts = listing ? reinterpret_cast<uint32_t *>(scratch + oCounts) : nullptr;
		A.summary = reinterpret_cast<cvxc_contacts_summary *>(scratch + oSummary);
		hipLaunchKernelGGL(contacts_init_kernel, dim3(Grid((size_t)instanceCount, kThreads)), dim3(kThreads), 0, ctx->stream, A);
		hipLaunchKernelGGL(contacts_count_kernel, dim3(WalkGrid(pairs)), dim3(kThreads), 0, ctx->stream, A);
		hipLaunchKernelGGL(contacts_finish_kernel, dim3(1), dim3(kFinishThreads), 0, ctx->stream, A);
		e = hipGetLastError();
	}
	// the list: the scan of the pairs' points and the second walk (its kernel cuts the list at the points found)
	auto list_points = [&](cvxc_contact_point *into, uint32_t limit) {
		A.points = into;
		A.limit = limit;
		cvxi::ExclusiveScan(ctx->stream, A.counts, (int)(pairs + 1), reinterpret_cast<unsigned long long *>(scratch + oChunks), reinterpret_cast<unsigned long long *>(scratch + oTotal));
		hipLaunchKernelGGL(contacts_write_kernel, dim3(WalkGrid(pairs)), dim3(kThreads), 0, ctx->stream, A);
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
			e = D.Allocate(&list, wanted * sizeof(cvxc_contact_point));
			if (e == hipSuccess) { e = list_points(reinterpret_cast<cvxc_contact_point *>(list), (uint32_t)wanted); }
			if (e == hipSuccess) { e = hipMemcpyAsync(backPoints.data(), list, wanted * sizeof(cvxc_contact_point), hipMemcpyDeviceToHost, ctx->stream); }
		}
		if (e == hipSuccess) { e = D.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
	}
	// (nothing is handed out to the host before the call can no longer fail)
	if (!backResults.empty()) { std::memcpy(results, backResults.data(), resultsBytes); }
	if (!backPoints.empty()) { std::memcpy(points, backPoints.data(), backPoints.size() * sizeof(cvxc_contact_point)); }
	if (summary) { *summary = host; }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxcontacts

extern "C" {

int cvxc_world_contacts(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside,
                        cvxc_contact_result *results, cvxc_contact_point *points, int64_t pointCapacity, cvxc_contacts_summary *summary, float *outDeviceMs)
{
	return cvxcontacts::Contacts(ctx, "cvxc_world_contacts", models, modelCount, instances, instanceCount, solidOutside, results, points, pointCapacity, false, summary,
	                             outDeviceMs);
}

int cvxc_world_contacts_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside,
                               cvxc_contact_result *resultsDevice, cvxc_contact_point *pointsDevice, int64_t pointCapacity, cvxc_contacts_summary *summary,
                               float *outDeviceMs)
{
	return cvxcontacts::Contacts(ctx, "cvxc_world_contacts_device", models, modelCount, instances, instanceCount, solidOutside, resultsDevice, pointsDevice, pointCapacity,
	                             true, summary, outDeviceMs);
}

int cvxc_contact_response(const cvxc_contact_result *r, double centre[3], double normal[3], double *depth)
{
	return cvxb::ContactResponse(r, centre, normal, depth) ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

} // extern "C"
