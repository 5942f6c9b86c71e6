// cvx_model_call.hip -- libcpuvox_gpu.so, the host driver of the calls that give results per unit and an optional list of points
// (cvxi::RunPointsCall, cvx_model_call.h): cvxc_world_contacts and cvxp_model_contacts with their _device forms.  No kernel lives here: the
// families launch their own through the two launchers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cvx_model_call.h"

namespace cvxi {

// The rules, each for every caller:
//   - what a copy reads from or writes to on the host is declared before the DeviceCall and so outlives it (freeing the device blocks waits for a
//     copy still under way)
//   - a failed allocation of the staging block fails the call before anything is enqueued; every failure goes through D.Fail
//   - the timing window opens behind the scratch allocation, before the first upload.  It closes before the ONE synchronisation of a call
//     without a host list, and behind the list's copy, before the second synchronisation, of a call with one
//   - a device list needs nothing from the host: its scan and write are enqueued behind the finish kernel, before the one synchronisation, with
//     the limit min(pointCapacity, 2^31 - 1); the write kernel cuts the list at the points found.  A host list is sized by the points found: a
//     block of min(points, pointCapacity) entries, the same scan and write, one copy back; with none wanted nothing is allocated or launched
//   - without jobs no walk and no scan is launched
//   - 2^31 points or more with a list asked for: CVX_ERR_CAPACITY, before anything is written to the caller's host memory
//   - results, points, the summary and the time are handed out only when the call can no longer fail
int RunPointsCall(cvx_context *ctx, const PointsCall &call, Launcher<PointsJob> launchResults, Launcher<PointsJob> launchWrite, float *outDeviceMs)
{
	const bool device = call.device, listing = call.pointCapacity > 0;
	const size_t jobs = (size_t)call.jobs, resultsBytes = (size_t)call.units * call.resultBytes;
	ModelStaging staging(call.models, call.modelCount, device || call.modelsStaged);
	std::vector<uint8_t> backResults(device ? 0 : resultsBytes), backPoints;
	int64_t host[4] = {};
	DeviceCall D(ctx, call.call);
	uint8_t *scratch = nullptr, *list = nullptr;
	hipError_t e = staging.Allocate(D);
	if (e != hipSuccess) { return D.Fail(e); }
	ScratchLayout carve;
	const size_t modelsBytes = (size_t)call.modelCount * sizeof(cvx_model), instancesBytes = (size_t)call.instanceCount * sizeof(cvx_model_instance),
	             prefixBytes = ((size_t)call.units + 1) * 4;
	const size_t chunks = listing ? (jobs + 1 + ScanChunk() - 1) / ScanChunk() : 0;
	const size_t oSummary = carve(sizeof host), oTotal = carve(8), oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oExtra = carve(call.extraBytes),
	             oPrefix = carve(prefixBytes), oResults = carve(backResults.size()), oCounts = carve(listing ? (jobs + 1) * 4 : 0), oChunks = carve(chunks * 8);
	PointsJob J{};
	e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = staging.Enqueue(ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, call.instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess && call.extra) { e = hipMemcpyAsync(scratch + oExtra, call.extra, call.extraBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPrefix, call.prefix, prefixBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess && listing) { e = hipMemsetAsync(scratch + oCounts + jobs * 4, 0, 4, ctx->stream); } // (the scan leaves the total behind the last job's offset)
	if (e == hipSuccess) {
		J.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
		J.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
		J.extra = call.extra ? scratch + oExtra : nullptr;
		J.prefix = reinterpret_cast<const uint32_t *>(scratch + oPrefix);
		J.results = device ? call.results : scratch + oResults;
		J.counts = listing ? reinterpret_cast<uint32_t *>(scratch + oCounts) : nullptr;
		J.summary = reinterpret_cast<int64_t *>(scratch + oSummary);
		e = launchResults(J);
		if (e == hipSuccess) { e = hipGetLastError(); }
	}
	// the list: the scan of the jobs' points and the second walk
	auto list_points = [&](void *into, uint32_t limit) {
		if (jobs == 0) { return hipSuccess; }
		J.points = into;
		J.limit = limit;
		ExclusiveScan(ctx->stream, J.counts, (int)(jobs + 1), reinterpret_cast<unsigned long long *>(scratch + oChunks), reinterpret_cast<unsigned long long *>(scratch + oTotal));
		const hipError_t launched = launchWrite(J);
		return launched == hipSuccess ? hipGetLastError() : launched;
	};
	const bool staged = listing && !device;
	if (e == hipSuccess && listing && device) { e = list_points(call.points, (uint32_t)std::min<int64_t>(call.pointCapacity, 0x7FFFFFFF)); }
	if (e == hipSuccess) { e = hipMemcpyAsync(host, J.summary, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !device) { e = hipMemcpyAsync(backResults.data(), J.results, resultsBytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && !staged) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (listing && host[2] >= ((int64_t)1 << 31)) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the contacts hold %lld points", call.call, (long long)host[2]); }
	if (staged) {
		const size_t wanted = (size_t)std::min<int64_t>(host[2], call.pointCapacity) * call.pointBytes;
		if (wanted) {
			backPoints.resize(wanted);
			e = D.Allocate(&list, wanted);
			if (e == hipSuccess) { e = list_points(list, (uint32_t)(wanted / call.pointBytes)); }
			if (e == hipSuccess) { e = hipMemcpyAsync(backPoints.data(), list, wanted, hipMemcpyDeviceToHost, ctx->stream); }
		}
		if (e == hipSuccess) { e = D.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
	}
	if (!backResults.empty()) { std::memcpy(call.results, backResults.data(), resultsBytes); }
	if (!backPoints.empty()) { std::memcpy(call.points, backPoints.data(), backPoints.size()); }
	if (call.summary) { std::memcpy(call.summary, host, sizeof host); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxi
