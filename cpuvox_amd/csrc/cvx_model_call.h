// cvx_model_call.h -- what the calls on "models + instances" share (cvx_models.hip, cvx_contacts.hip, cvx_pair_contacts.hip, cvx_model_pick.hip):
// the staging of host model arrays on the device, the host driver of the calls that give results per unit and an optional list of points
// (cvx_model_call.hip, DESIGN.md "Results per unit and a list of points") and the body of their finish kernel.  Not part of the C ABI.
#pragma once

#include <vector>

#include "cpuvox_gpu_contacts.h"
#include "cpuvox_gpu_models.h"
#include "cpuvox_gpu_pair_contacts.h"
#include "cvx_context.h"

namespace cvxi {

// The host arrays of a call's models staged on the device: ONE block, every array at a multiple of 16, argb before solid per model, in model
// order, then whatever the caller adds.  With `device` the arrays are on the device already: nothing is planned, allocated or copied and the
// descriptors stay the caller's.  Copies read `descriptors` and the caller's arrays until the stream has run them: the staging is declared
// before the DeviceCall that owns its block.
struct ModelStaging {
	struct Upload {
		size_t at, bytes;
		const void *from; // null: room only
	};
	std::vector<cvx_model> descriptors; // what to upload for `models`: after Allocate, argb / solid point into the block where they were not NULL
	std::vector<Upload> uploads;
	ScratchLayout layout;               // layout.bytes: the block's size
	uint8_t *block = nullptr;
	bool device;

	ModelStaging(const cvx_model *models, int modelCount, bool device) : descriptors(models, models + modelCount), device(device)
	{
		for (int k = 0; k < modelCount && !device; k++) {
			const size_t n = (size_t)models[k].size[0] * (size_t)models[k].size[1] * (size_t)models[k].size[2];
			if (models[k].argb) { Add(n * 4, models[k].argb); }
			if (models[k].solid) { Add(n, models[k].solid); }
		}
	}
	// A further region behind the arrays, copied from `from` with them unless that is null (cvxq_model_pick's rays and hits): its offset
	size_t Add(size_t bytes, const void *from)
	{
		uploads.push_back(Upload{ layout(bytes), bytes, from });
		return uploads.back().at;
	}
	hipError_t Allocate(DeviceCall &D)
	{
		if (device) { return hipSuccess; }
		const hipError_t e = D.Allocate(&block, layout.bytes);
		if (e != hipSuccess) { return e; }
		size_t u = 0;
		for (cvx_model &m : descriptors) {
			if (m.argb) { m.argb = reinterpret_cast<const uint32_t *>(block + uploads[u++].at); }
			if (m.solid) { m.solid = block + uploads[u++].at; }
		}
		return hipSuccess;
	}
	hipError_t Enqueue(hipStream_t stream) const
	{
		hipError_t e = hipSuccess;
		for (const Upload &u : uploads) {
			if (e == hipSuccess && u.from) { e = hipMemcpyAsync(block + u.at, u.from, u.bytes, hipMemcpyHostToDevice, stream); }
		}
		return e;
	}
};

// ---- results per unit and an optional list of points (cvxc_world_contacts: a unit is an instance; cvxp_model_contacts: a pair) ----
// What the caller says of its call.  Its summary is four int64 words, the third the points found.
struct PointsCall {
	const char *call;
	const cvx_model *models;
	int modelCount;
	const cvx_model_instance *instances;
	int instanceCount;
	const uint32_t *prefix; // units + 1: the jobs before every unit
	int units;
	int64_t jobs;           // below 2^31 - 1; may be 0
	const void *extra;      // null, or one more host array the kernels read (the pairs)
	size_t extraBytes;
	size_t resultBytes, pointBytes; // of one record
	void *results, *points; // `device` says where these and the models' arrays live
	int64_t pointCapacity;
	bool device;
	int64_t *summary;       // may be null
	bool modelsStaged = false; // the models' arrays are on the device already whatever `device` says (cvxs_world_sweep's second phase)
};
// What RunPointsCall owns and hands to the caller's two launchers: device pointers all
struct PointsJob {
	const cvx_model *models;
	const cvx_model_instance *instances;
	const uint32_t *prefix;
	const void *extra;
	void *results;
	uint32_t *counts; // null without a list, else jobs + 1: the points of every job, the scan turns them into the jobs' first points
	int64_t *summary;
	void *points;     // the write launcher only: the list, entries below `limit` (its kernel cuts it at the points found)
	uint32_t limit;
};
// cvx_model_call.hip.  launchResults enqueues the family's init, count (unless there is no job) and finish kernels: the results complete and the
// summary at J.summary; launchWrite enqueues its write kernel and is never called without jobs.  The rules it keeps are written down at its definition.
int RunPointsCall(cvx_context *ctx, const PointsCall &call, Launcher<PointsJob> launchResults, Launcher<PointsJob> launchWrite, float *outDeviceMs);
// cvx_contacts.hip: the body of cvxc_world_contacts[_device] under the name `call`; `device` says where results and points live, and the models'
// arrays too unless modelsStaged says that they are on the device anyway (cvx_sweep.hip runs it on the moved instances).
int WorldContacts(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside,
                  cvxc_contact_result *results, cvxc_contact_point *points, int64_t pointCapacity, bool device, bool modelsStaged, cvxc_contacts_summary *summary,
                  float *outDeviceMs);
// cvx_pair_contacts.hip: the body of cvxp_model_contacts[_device] under the name `call`.  offsets (may be null: those calls as they are): three
// int32 a pair, body a of pair p is I_a + offsets[p] for that pair alone, and the results still carry the pair as given (cvx_pair_sweep.hip runs
// it on the touching poses; the offsets keep every moved instance inside the limits).  device and modelsStaged as WorldContacts'.
int PairContacts(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs,
                 int pairCount, const int32_t *offsets, cvxp_pair_result *results, cvxp_pair_point *points, int64_t pointCapacity, bool device, bool modelsStaged,
                 cvxp_pairs_summary *summary, float *outDeviceMs);

#ifdef __HIPCC__
constexpr int kFinishThreads = 1024;
// The body of a finish kernel of ONE workgroup of kFinishThreads threads.  Thread t finishes units kUnitsMax / kFinishThreads * t ..: firstPoint from
// an inclusive scan of the threads' points, finish(r) (the family's ...ResultFinish), fold(r, totals) adds the finished result to the thread's
// kTotals totals.  Returns the workgroup's totals (LDS) and leaves the points of all units in *points, for the thread that writes the summary.
template <int kUnitsMax, int kTotals, class Result, class Finish, class Fold>
__device__ __forceinline__ const unsigned long long *FinishResults(Result *results, int units, Finish finish, Fold fold, unsigned long long *points)
{
	constexpr int kEach = kUnitsMax / kFinishThreads;
	static_assert(kFinishThreads * kEach == kUnitsMax, "the finish kernel's one workgroup covers every unit");
	__shared__ unsigned long long scan[kFinishThreads];
	__shared__ unsigned long long totals[kTotals];
	const int t = (int)threadIdx.x;
	if (t < kTotals) { totals[t] = 0ull; }
	unsigned long long mine = 0ull;
	for (int j = 0; j < kEach; j++) {
		const int k = kEach * t + j;
		if (k < units) { mine += (unsigned long long)results[k].points; }
	}
	scan[t] = mine;
	__syncthreads();
	for (int d = 1; d < kFinishThreads; d <<= 1) {
		const unsigned long long before = t >= d ? scan[t - d] : 0ull;
		__syncthreads();
		scan[t] += before;
		__syncthreads();
	}
	unsigned long long firstPoint = scan[t] - mine, sums[kTotals] = {};
	for (int j = 0; j < kEach; j++) {
		const int k = kEach * t + j;
		if (k >= units) { break; }
		Result *r = results + k;
		r->firstPoint = (int64_t)firstPoint;
		firstPoint += (unsigned long long)r->points;
		finish(r);
		fold(*r, sums);
	}
#pragma unroll
	for (int i = 0; i < kTotals; i++) {
		if (sums[i] != 0ull) { atomicAdd(&totals[i], sums[i]); }
	}
	__syncthreads();
	*points = scan[kFinishThreads - 1];
	return totals;
}
#endif

} // namespace cvxi
