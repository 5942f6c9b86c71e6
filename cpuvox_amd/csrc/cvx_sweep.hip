// cvx_sweep.hip -- libcpuvox_gpu.so, how far placed voxel models can move before they touch the device-resident world (cvxs_world_sweep,
// cvxs_world_sweep_device, cvxs_sweep_offset, cvxs_instance_moved).  See include/cpuvox_gpu_sweep.h for the contract and cvx_sweep.h for the rules.
//
// Phase 1.  A WAVE per (instance, column of its box, station) job; a station is the stretch of the instance's path between two horizontal
// steps, so all of its poses lie over one column of the world.  The host uploads the prefix of footprint * stations, 16 bytes an instance
// (where its stations begin) and the 16-byte station records; a wave finds its instance with cvxb::ContactsPairInstance's wave-uniform binary
// search.  The column of the body is cvx_contacts.hip's: cvxb::ContactsColumnJobOf through readfirstlane, a tall box cut to the body by
// cvxb::ContactsStepRange.  The station and the world's column under it are wave-uniform too.  The lanes are the 64 voxels of a step: a lane
// whose voxel is in the body finds, by ONE binary search of the world column's runs (cvxb::SweepFirstSolid), the first of the station's y steps
// at which that voxel is solid; its candidate is the step's index on the path.  The lanes keep their minimum over the steps, the wave reduces
// it once and issues one 32-bit atomicMin on first[k].  No LDS, nothing is written to the arena.
// (Not built in: a wave that reads first[k] <= j0 at its start could return at once, the result being a minimum.  The read has to see other
// waves' atomics, so it is an agent-scope load that goes past the caches; measured on an MI355X it made the kernel 3.5 times slower on vertical
// motions and saved nothing on the others, which are bound by the loads that come before it -- profiles/sweep.md.)
// Phase 2.  The host reads first[] (4 bytes an instance), fills the sweeps and, unless the contacts are not asked for, runs the body of
// cvxc_world_contacts[_device] (cvxi::WorldContacts, cvx_contacts.hip's kernels as they are) on the instances moved to `at`; the models' arrays
// are staged once for both phases.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cvx_model_call.h"
#include "cvx_sweep.h"

using cvxi::Fail;

namespace cvxsweep {

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr unsigned kMaxWorkgroups = 65536; // 2^18 waves, the waves take the jobs in turn
static_assert(sizeof(cvxs_sweep_result) == 48 && sizeof(cvxs_sweeps_summary) == 32 && sizeof(cvxb::SweepStation) == 16 && sizeof(cvxb::SweepInstanceJob) == 16,
              "the records as the header and the uploads state them");

struct Args {
	cvxb::CopyWorld W;
	const cvx_model *models;             // device copies; the arrays they point to are on the device
	const cvx_model_instance *instances;
	const uint32_t *prefix;              // instanceCount + 1: the jobs before every instance
	const cvxb::SweepInstanceJob *info;
	const cvxb::SweepStation *stations;  // of all instances, in order
	uint32_t *first;                     // per instance the least touching step so far, kSweepNone: none
	int instanceCount;
	uint32_t jobs;
	int solidOutside;
};

__device__ __forceinline__ void WalkJob(const Args &A, uint32_t job, int lane)
{
	const cvxi::WaveUniform U;
	const int k = U(cvxb::ContactsPairInstance(A.prefix, A.instanceCount, job));
	const cvx_model_instance &I = A.instances[k];
	const cvxb::SweepInstanceJob &N = A.info[k];
	const int32_t x0 = U(I.boxMin[0]), z0 = U(I.boxMin[2]);
	const uint32_t sizeX = (uint32_t)(U(I.boxMax[0]) - x0), sizeZ = (uint32_t)(U(I.boxMax[2]) - z0), footprint = sizeX * sizeZ;
	const uint32_t local = job - A.prefix[k], q = local / footprint, column = local - q * footprint;
	const cvxb::SweepStation &R = A.stations[(uint32_t)U((int32_t)N.stationBase) + q];
	const uint32_t word = (uint32_t)U(*reinterpret_cast<const int32_t *>(&R)); // ox, oz
	const cvxb::SweepStation S{ (int16_t)(word & 0xFFFFu), (int16_t)(word >> 16), U(R.j0), U(R.dy0), U(R.dyCount) };
	const int32_t signY = U(N.signY);
	const int32_t cx = x0 + (int32_t)(column / sizeZ), cz = z0 + (int32_t)(column % sizeZ);
	const cvxb::ContactsColumnJob J = cvxb::ContactsColumnJobOf(U, A.models, I, cx, cz);
	const cvxb::DistanceColumn world = cvxb::DistanceColumnAt(A.W, (int64_t)cx + S.ox, (int64_t)cz + S.oz, A.solidOutside);
	const int64_t dimY = A.W.dimY;
	uint32_t best = cvxb::kSweepNone;
	int32_t top, low;
	cvxb::ContactsStepRange(J, &top, &low);
	for (int32_t yTop = top; yTop >= low; yTop -= CVX_WAVE) {
		const uint32_t mine = cvxb::SweepLane(J, world, dimY, S, signY, yTop - lane);
		best = mine < best ? mine : best;
	}
	best = cvxi::WaveReduce(best, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
	if (lane == 0 && best != cvxb::kSweepNone) { atomicMin(A.first + k, best); }
}

__global__ __launch_bounds__(kThreads) void sweep_kernel(Args A)
{
	cvxi::ForEachWaveJob(A.jobs, kWaves, [&](uint64_t at, int lane) { WalkJob(A, (uint32_t)at, lane); });
}

// Both calls: `device` says where the models' arrays, `contacts` and `points` live.
static int Sweep(cvx_context *ctx, const char *call, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *motions,
                 int solidOutside, cvxs_sweep_result *sweeps, cvxc_contact_result *contacts, cvxc_contact_point *points, int64_t pointCapacity, bool device,
                 cvxs_sweeps_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[200];
	if (!cvxb::SweepValidate(models, modelCount, instances, instanceCount, motions, solidOutside, sweeps, contacts, points, pointCapacity, message, sizeof message)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message);
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	std::vector<uint32_t> prefix((size_t)instanceCount + 1), first((size_t)instanceCount);
	std::vector<cvxb::SweepInstanceJob> info((size_t)instanceCount);
	int64_t stationCount = 0;
	const int64_t jobs = cvxb::SweepJobs(instances, motions, instanceCount, prefix.data(), info.data(), &stationCount);
	if (jobs < 0) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: the boxes' footprints times their motions' stations sum to 2^31 - 1 or more jobs", call); }
	std::vector<cvxb::SweepStation> stations((size_t)stationCount);
	for (int k = 0; k < instanceCount; k++) { cvxb::SweepStations(motions + 3 * (size_t)k, stations.data() + info[k].stationBase); }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	// phase 1 (the vectors above outlive D: freeing the device blocks waits for a copy still under way)
	std::vector<cvxs_sweep_result> out((size_t)instanceCount);
	std::vector<cvx_model_instance> moved((size_t)instanceCount);
	cvxi::ModelStaging staging(models, modelCount, device);
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	hipError_t e = staging.Allocate(D);
	if (e != hipSuccess) { return D.Fail(e); }
	cvxi::ScratchLayout carve;
	const size_t modelsBytes = (size_t)modelCount * sizeof(cvx_model), instancesBytes = (size_t)instanceCount * sizeof(cvx_model_instance),
	             prefixBytes = prefix.size() * 4, infoBytes = info.size() * sizeof(cvxb::SweepInstanceJob), stationsBytes = stations.size() * sizeof(cvxb::SweepStation),
	             firstBytes = first.size() * 4;
	const size_t oModels = carve(modelsBytes), oInstances = carve(instancesBytes), oPrefix = carve(prefixBytes), oInfo = carve(infoBytes), oStations = carve(stationsBytes),
	             oFirst = carve(firstBytes);
	Args A{};
	e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = staging.Enqueue(ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oModels, staging.descriptors.data(), modelsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInstances, instances, instancesBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPrefix, prefix.data(), prefixBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oInfo, info.data(), infoBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oStations, stations.data(), stationsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemsetAsync(scratch + oFirst, 0xFF, firstBytes, ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.models = reinterpret_cast<const cvx_model *>(scratch + oModels);
		A.instances = reinterpret_cast<const cvx_model_instance *>(scratch + oInstances);
		A.prefix = reinterpret_cast<const uint32_t *>(scratch + oPrefix);
		A.info = reinterpret_cast<const cvxb::SweepInstanceJob *>(scratch + oInfo);
		A.stations = reinterpret_cast<const cvxb::SweepStation *>(scratch + oStations);
		A.first = reinterpret_cast<uint32_t *>(scratch + oFirst);
		A.instanceCount = instanceCount;
		A.jobs = (uint32_t)jobs;
		A.solidOutside = solidOutside;
		hipLaunchKernelGGL(sweep_kernel, dim3(std::min(cvxi::Grid((size_t)jobs, kWaves), kMaxWorkgroups)), dim3(kThreads), 0, ctx->stream, A);
		e = hipGetLastError();
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(first.data(), A.first, firstBytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }

	// phase 2
	cvxs_sweeps_summary totals{ 0, 0, jobs, 0 };
	for (int k = 0; k < instanceCount; k++) {
		out[k] = cvxb::SweepResultOf(motions + 3 * (size_t)k, first[k]);
		totals.hits += out[k].hit >= 0 ? 1 : 0;
		totals.startsSolid += out[k].hit == 0 ? 1 : 0;
		cvxb::SweepInstanceMoved(instances[k], out[k].at, &moved[k]); // (inside the limits: I + v is, and `at` lies between 0 and v)
	}
	float ms = D.Ms();
	if (contacts) {
		cvxc_contacts_summary found{};
		float second = 0.f;
		const int code = cvxi::WorldContacts(ctx, call, staging.descriptors.data(), modelCount, moved.data(), instanceCount, solidOutside, contacts, points, pointCapacity,
		                                     device, true, &found, &second);
		if (code != CVX_OK) { return code; }
		totals.points = found.points;
		ms += second;
	}
	// (nothing is handed out to the host before the call can no longer fail)
	std::memcpy(sweeps, out.data(), out.size() * sizeof(cvxs_sweep_result));
	if (summary) { *summary = totals; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // namespace cvxsweep

extern "C" {

int cvxs_world_sweep(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *motions,
                     int solidOutside, cvxs_sweep_result *sweeps, cvxc_contact_result *contacts, cvxc_contact_point *points, int64_t pointCapacity,
                     cvxs_sweeps_summary *summary, float *outDeviceMs)
{
	return cvxsweep::Sweep(ctx, "cvxs_world_sweep", models, modelCount, instances, instanceCount, motions, solidOutside, sweeps, contacts, points, pointCapacity, false, summary,
	                       outDeviceMs);
}

int cvxs_world_sweep_device(cvx_context *ctx, const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *motions,
                            int solidOutside, cvxs_sweep_result *sweeps, cvxc_contact_result *contactsDevice, cvxc_contact_point *pointsDevice, int64_t pointCapacity,
                            cvxs_sweeps_summary *summary, float *outDeviceMs)
{
	return cvxsweep::Sweep(ctx, "cvxs_world_sweep_device", models, modelCount, instances, instanceCount, motions, solidOutside, sweeps, contactsDevice, pointsDevice,
	                       pointCapacity, true, summary, outDeviceMs);
}

int cvxs_sweep_offset(const int32_t motion[3], int j, int32_t offset[3], int *axis)
{
	if (!motion || !offset || !axis) { return CVX_ERR_INVALID_ARGUMENT; }
	for (int a = 0; a < 3; a++) {
		if (motion[a] < -CVXS_MAX_MOTION || motion[a] > CVXS_MAX_MOTION) { return CVX_ERR_INVALID_ARGUMENT; }
	}
	return cvxb::SweepOffset(motion, j, offset, axis) ? CVX_OK : CVX_ERR_INVALID_ARGUMENT;
}

int cvxs_instance_moved(const cvx_model_instance *in, const int32_t offset[3], cvx_model_instance *out)
{
	if (!in || !offset || !out) { return CVX_ERR_INVALID_ARGUMENT; }
	cvx_model_instance moved;
	if (!cvxb::SweepInstanceMoved(*in, offset, &moved)) { return CVX_ERR_INVALID_ARGUMENT; }
	*out = moved;
	return CVX_OK;
}

} // extern "C"
