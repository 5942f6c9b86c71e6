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
//   2. finish (cvxi::FinishResults, a thread per four instances): firstPoint, the box as [min, max) or zeros, the summary.
//   3. write  (only with pointCapacity > 0): the same walk writes each point at its pair's offset + the points of the steps above + the lanes
//             below in the ballot (lane order is descending y).
// No LDS in the walk.  Nothing is written to the arena.  The host's side -- staging, scratch, the scan, the device and the host list, the
// synchronisations and the copies back -- is cvxi::RunPointsCall (cvx_model_call.hip), a unit being an instance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "cvx_contacts.h"
#include "cvx_model_call.h"

using cvxi::Fail;

namespace cvxcontacts {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // of the two walks: 2^18 waves, some thirty times what an MI355X holds at once
static_assert(sizeof(cvxc_contacts_summary) == 4 * sizeof(int64_t) && offsetof(cvxc_contacts_summary, points) == 2 * sizeof(int64_t), "the summary as cvxi::PointsCall takes it");

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

// The wave's walk of pair `pair`.  kWrite false: the pair's sums into its instance's result (and its points into A.counts); true: its points
// into the list from entry `first` on.
template <bool kWrite>
__device__ __forceinline__ void WalkPair(const Args &A, uint32_t pair, int lane, uint32_t first)
{
	const cvxi::WaveUniform U;
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
			const uint32_t entry = at + cvxi::LanesBelow(points);
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

// Both walks: the launch's waves take the pairs in turn (cvxi::ForEachWaveJob: a launch has at most kMaxWorkgroups workgroups, whatever the pairs).
__global__ __launch_bounds__(kThreads) void contacts_count_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.pairs, kWaves, [&](uint64_t at, int lane) { WalkPair<false>(A, (uint32_t)at, lane, 0u); });
}

// The list holds min(A.limit, the points found) entries: the finish kernel has left the points in the summary, and the offsets are good only
// below 2^31 points (the host then fails the call).
__global__ __launch_bounds__(kThreads) void contacts_write_kernel(Args A)
{
	const uint64_t found = (uint64_t)A.summary->points;
	if (found >= (1ull << 31)) { return; }
	A.limit = found < A.limit ? (uint32_t)found : A.limit;
	cvxi::ForEachWaveJob(A.pairs, kWaves, [&](uint64_t at, int lane) {
		const uint32_t pair = (uint32_t)at, first = A.counts[pair];
		if (first >= A.limit || A.counts[pair + 1u] == first) { return; }
		WalkPair<true>(A, pair, lane, first);
	});
}

// One workgroup (cvxi::FinishResults): firstPoint, the box, the summary.  The totals stay zero when no body voxel was seen.
__global__ __launch_bounds__(cvxi::kFinishThreads) void contacts_finish_kernel(Args A)
{
	unsigned long long points;
	const unsigned long long *totals = cvxi::FinishResults<CVX_MODELS_MAX_INSTANCES, 3>(
		A.results, A.instanceCount, [](cvxc_contact_result *r) { cvxb::ContactResultFinish(r); },
		[](const cvxc_contact_result &r, unsigned long long *sums) { // touching, overlap, voxels
			sums[0] += r.overlap > 0 ? 1ull : 0ull;
			sums[1] += (unsigned long long)r.overlap;
			sums[2] += (unsigned long long)r.voxels;
		},
		&points);
	if (threadIdx.x == 0) { *A.summary = cvxc_contacts_summary{ (int64_t)totals[0], (int64_t)totals[1], (int64_t)points, (int64_t)totals[2] }; }
}

} // namespace cvxcontacts

// Both calls (and cvx_sweep.hip's second phase: cvx_model_call.h): `device` says where the models' arrays, `results` and `points` live.
int cvxi::WorldContacts(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount,
                        int solidOutside, cvxc_contact_result *results, cvxc_contact_point *points, int64_t pointCapacity, bool device, bool modelsStaged,
                        cvxc_contacts_summary *summary, float *outDeviceMs)
{
	using namespace cvxcontacts;
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::ContactsValidate(models, modelCount, instances, instanceCount, solidOutside, results, points, pointCapacity, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	std::vector<uint32_t> prefix((size_t)instanceCount + 1);
	const int64_t pairs = cvxb::ContactsPairs(instances, instanceCount, prefix.data());
	if (pairs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the boxes' footprints sum to 2^31 - 1 or more (instance, column) pairs", call); }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	Args A{};
	A.W = cvxi::WorldOf(ctx);
	A.instanceCount = instanceCount;
	A.pairs = (uint32_t)pairs;
	A.solidOutside = solidOutside;
	const dim3 walk(std::min(cvxi::Grid((size_t)pairs, kWaves), kMaxWorkgroups)), block(kThreads);
	const cvxi::PointsCall C{ call, models, modelCount, instances, instanceCount, prefix.data(), instanceCount, pairs, nullptr, 0, sizeof(cvxc_contact_result),
		                      sizeof(cvxc_contact_point), results, points, pointCapacity, device, reinterpret_cast<int64_t *>(summary), modelsStaged };
	return cvxi::RunPointsCall(
		ctx, C,
		[&](const cvxi::PointsJob &J) {
			A.models = J.models;
			A.instances = J.instances;
			A.prefix = J.prefix;
			A.results = static_cast<cvxc_contact_result *>(J.results);
			A.counts = J.counts;
			A.summary = reinterpret_cast<cvxc_contacts_summary *>(J.summary);
			hipLaunchKernelGGL(contacts_init_kernel, dim3(cvxi::Grid((size_t)instanceCount)), block, 0, ctx->stream, A);
			if (pairs > 0) { hipLaunchKernelGGL(contacts_count_kernel, walk, block, 0, ctx->stream, A); }
			hipLaunchKernelGGL(contacts_finish_kernel, dim3(1), dim3(cvxi::kFinishThreads), 0, ctx->stream, A);
			return hipSuccess;
		},
		[&](const cvxi::PointsJob &J) {
			A.points = static_cast<cvxc_contact_point *>(J.points);
			A.limit = J.limit;
			hipLaunchKernelGGL(contacts_write_kernel, walk, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

extern "C" {

int cvxc_world_contacts(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside,
                        cvxc_contact_result *results, cvxc_contact_point *points, int64_t pointCapacity, cvxc_contacts_summary *summary, float *outDeviceMs)
{
	return cvxi::WorldContacts(ctx, "cvxc_world_contacts", models, modelCount, instances, instanceCount, solidOutside, results, points, pointCapacity, false, false, summary,
	                           outDeviceMs);
}

int cvxc_world_contacts_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside,
                               cvxc_contact_result *resultsDevice, cvxc_contact_point *pointsDevice, int64_t pointCapacity, cvxc_contacts_summary *summary,
                               float *outDeviceMs)
{
	return cvxi::WorldContacts(ctx, "cvxc_world_contacts_device", models, modelCount, instances, instanceCount, solidOutside, resultsDevice, pointsDevice, pointCapacity,
	                           true, false, summary, outDeviceMs);
}

int cvxc_contact_response(const cvxc_contact_result *r, double centre[3], double normal[3], double *depth)
{
	return cvxb::ContactResponse(r, centre, normal, depth) ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

} // extern "C"
