// cvx_snapshot.hip -- libcpuvox_gpu.so, snapshots of rectangles of the device-resident world that stay on the device: cvx_world_snapshot,
// cvx_world_snapshot_restore, cvx_world_snapshot_diff / _device.  See include/cpuvox_gpu_snapshot.h for the contracts, cvx_snapshot.h for the
// per-column rule of the comparison and DESIGN.md section 3.
//
// A snapshot joins three things the library had: the read-back's count, scan and write into a device blob (cvxi::RegionReadCount /
// RegionReadWrite, cvx_readback.hip), run for every held level with ONE synchronisation for all totals; the edit's patch of any level from a
// (headers, elements) pair (cvxi::PatchLevelsFromDevice, cvx_edit.hip), one job per level and no downsampling; and the one kernel that was
// missing, the comparison:
//   1. count  (a thread per column of the rectangle): cvxs::DiffColumn of the arena's column and the snapshot's; 1 for a changed column, its
//             [yMin, yMax) kept for the write; the totals and the bounding box reduced per workgroup (shuffles, then LDS) into one partial each
//   2. the flags are prefix-scanned into list positions, the partials reduced by one workgroup (sums, minima and maxima of integers: the same
//      in every order; no atomic anywhere -- 16 384 waves adding to one address cost more than the comparison); ONE copy brings the summary
//      to the host
//   3. write  (same threads): the entries below the capacity, each at its scanned position -- the column order, with no sort and no atomic
//             deciding a place.
// A lane per column is the read-back's mapping; a wave waits for its tallest column while colours are compared.  The result does not depend
// on the mapping: every column's entry is a function of that column alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>

#include "cpuvox_gpu_snapshot.h"
#include "cvx_context.h"
#include "cvx_snapshot.h"

using cvxi::Fail;
using cvxi::Grid;
using cvxi::kThreads;

struct cvx_snapshot {
	cvx_context *ctx = nullptr;
	int device = 0;
	cvx_snapshot_info info{};
	uint8_t *blob[CVX_LOD_LEVELS] = {}; // per held level: (rectangle >> level) headers of 12 bytes, then the element pool
};

namespace cvxsnap {

struct Partial { // what a workgroup's columns add to the summary; Neutral() for none
	unsigned long long changedColumns, changedVoxels;
	int min[3], max[3];
};

struct Totals {
	unsigned long long listed; // the scan's total (= sum.changedColumns)
	Partial sum;
};

__device__ __forceinline__ Partial Neutral() { return Partial{ 0ull, 0ull, { INT_MAX, INT_MAX, INT_MAX }, { INT_MIN, INT_MIN, INT_MIN } }; }

__device__ __forceinline__ Partial Combine(const Partial &a, const Partial &b)
{
	Partial c{ a.changedColumns + b.changedColumns, a.changedVoxels + b.changedVoxels, {}, {} };
	for (int k = 0; k < 3; k++) {
		c.min[k] = a.min[k] < b.min[k] ? a.min[k] : b.min[k];
		c.max[k] = a.max[k] > b.max[k] ? a.max[k] : b.max[k];
	}
	return c;
}

// The workgroup's (256 threads) combined partial, valid in thread 0.  Every thread takes part.
__device__ __forceinline__ Partial BlockReduce(Partial p)
{
	__shared__ Partial waves[4];
	auto sum = [](unsigned long long a, unsigned long long b) { return a + b; };
	auto least = [](int a, int b) { return a < b ? a : b; };
	auto most = [](int a, int b) { return a > b ? a : b; };
	p.changedColumns = cvxi::WaveReduce(p.changedColumns, sum);
	p.changedVoxels = cvxi::WaveReduce(p.changedVoxels, sum);
	for (int k = 0; k < 3; k++) {
		p.min[k] = cvxi::WaveReduce(p.min[k], least);
		p.max[k] = cvxi::WaveReduce(p.max[k], most);
	}
	if ((threadIdx.x & 63u) == 0u) { waves[threadIdx.x >> 6] = p; }
	__syncthreads();
	if (threadIdx.x == 0u) { p = Combine(Combine(waves[0], waves[1]), Combine(waves[2], waves[3])); }
	return p;
}

struct DiffArgs {
	cvxb::CopyWorld W;
	int x0, z0, sizeZ, n;
	const uint32_t *headers, *elements; // the snapshot's LOD 0
	int ignoreColour;
	uint32_t *offsets;                  // per column: 1 = changed (-> list position after the scan)
	uint2 *ranges;                      // per column: yMin, yMax
	Partial *partials;                  // per workgroup of the count
	int groups;
	Totals *totals;
	cvx_snapshot_change *changes;
	uint32_t limit;
};

__global__ __launch_bounds__(256) void snapshot_diff_count_kernel(DiffArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	cvxs::ColumnDiff d{ 0u, 0u, 0u };
	int x = 0, z = 0;
	if (i < A.n) {
		x = A.x0 + i / A.sizeZ;
		z = A.z0 + i % A.sizeZ;
		d = cvxs::DiffColumn(cvxb::CopyColumnAt(A.W, x, z), A.W.colourSlots, A.W.colorShift, A.W.dimY, A.headers + 3 * (size_t)i, A.elements, A.ignoreColour != 0);
		A.offsets[i] = d.voxels ? 1u : 0u;
		A.ranges[i] = make_uint2(d.yMin, d.yMax);
	}
	Partial p = Neutral();
	if (d.voxels != 0u) { p = Partial{ 1ull, d.voxels, { x, (int)d.yMin, z }, { x + 1, (int)d.yMax, z + 1 } }; }
	p = BlockReduce(p); // (every thread takes part: the ones behind the rectangle and the unchanged columns with the neutral partial)
	if (threadIdx.x == 0u) { A.partials[blockIdx.x] = p; }
}

// One workgroup: the partials of the count's workgroups into the summary
__global__ __launch_bounds__(256) void snapshot_diff_reduce_kernel(DiffArgs A)
{
	Partial p = Neutral();
	for (int g = threadIdx.x; g < A.groups; g += 256) { p = Combine(p, A.partials[g]); }
	p = BlockReduce(p);
	if (threadIdx.x == 0u) { A.totals->sum = p; }
}

__global__ __launch_bounds__(256) void snapshot_diff_write_kernel(DiffArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const uint2 range = A.ranges[i];
	const uint32_t at = A.offsets[i];
	if (range.y == 0u || at >= A.limit) { return; } // (yMax = 0: nothing differs in the column)
	A.changes[at] = cvx_snapshot_change{ A.x0 + i / A.sizeZ, A.z0 + i % A.sizeZ, (int32_t)range.x, (int32_t)range.y };
}

// What restore and diff ask of a (context, snapshot) pair before anything is enqueued
static int CheckPair(cvx_context *ctx, const cvx_snapshot *snap, const char *call)
{
	if (!snap) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: snap is NULL", call); }
	if (snap->ctx != ctx) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another context", call); }
	return CVX_OK;
}

static int CheckWorld(cvx_context *ctx, const cvx_snapshot *snap, const char *call)
{
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const DevWorld &W = ctx->hostWorld;
	const cvx_snapshot_info &I = snap->info;
	if (W.dimX != I.dimX || W.dimY != I.dimY || W.dimZ != I.dimZ) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: the world is %d x %d x %d, the snapshot was taken from one of %d x %d x %d", call, W.dimX, W.dimY, W.dimZ, I.dimX,
		            I.dimY, I.dimZ);
	}
	return cvxi::PrepareWorld(ctx);
}

// Both calls: `device` says where `changes` lives.
static int Diff(cvx_context *ctx, const char *call, const cvx_snapshot *snap, int flags, cvx_snapshot_change *changes, bool device, int64_t changeCapacity,
                cvx_snapshot_diff_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	int rc = CheckPair(ctx, snap, call);
	if (rc != CVX_OK) { return rc; }
	if (flags & ~CVX_SNAPSHOT_IGNORE_COLOUR) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: unknown flags bits 0x%x", call, (unsigned)flags); }
	if (changeCapacity < 0 || (changeCapacity > 0 && !changes)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: changeCapacity %lld with %s list", call, (long long)changeCapacity, changes ? "a" : "no");
	}
	rc = CheckWorld(ctx, snap, call);
	if (rc != CVX_OK) { return rc; }

	const cvx_snapshot_info &I = snap->info;
	const int n = I.sizeX * I.sizeZ;
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	cvxi::ScratchLayout carve;
	const size_t chunks = ((size_t)n + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
	const size_t groups = Grid((size_t)n);
	const size_t oTotals = carve(sizeof(Totals)), oOffsets = carve((size_t)n * 4), oRanges = carve((size_t)n * 8), oChunks = carve(chunks * 8),
	             oPartials = carve(groups * sizeof(Partial));
	Totals host{};
	DiffArgs A{};
	hipError_t e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.x0 = I.x0;
		A.z0 = I.z0;
		A.sizeZ = I.sizeZ;
		A.n = n;
		A.headers = reinterpret_cast<const uint32_t *>(snap->blob[0]);
		A.elements = reinterpret_cast<const uint32_t *>(snap->blob[0] + (size_t)n * 12);
		A.ignoreColour = (flags & CVX_SNAPSHOT_IGNORE_COLOUR) != 0;
		A.totals = reinterpret_cast<Totals *>(scratch + oTotals);
		A.offsets = reinterpret_cast<uint32_t *>(scratch + oOffsets);
		A.ranges = reinterpret_cast<uint2 *>(scratch + oRanges);
		A.partials = reinterpret_cast<Partial *>(scratch + oPartials);
		A.groups = (int)groups;
		hipLaunchKernelGGL(snapshot_diff_count_kernel, dim3((unsigned)groups), dim3(kThreads), 0, ctx->stream, A);
		hipLaunchKernelGGL(snapshot_diff_reduce_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.offsets, n, reinterpret_cast<unsigned long long *>(scratch + oChunks), &A.totals->listed);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host, A.totals, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) { return D.Fail(e); }
	const cvxi::ListCall list{ sizeof(cvx_snapshot_change), host.sum.changedColumns, changeCapacity, changes, device };
	rc = cvxi::FinishList(ctx, D, list, [&](const cvxi::ListJob &J) {
		A.changes = static_cast<cvx_snapshot_change *>(J.into);
		A.limit = J.limit;
		hipLaunchKernelGGL(snapshot_diff_write_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, A);
		return hipSuccess;
	});
	if (rc != CVX_OK) { return rc; }
	if (summary) {
		std::memset(summary, 0, sizeof *summary);
		summary->changedColumns = (int64_t)host.sum.changedColumns;
		summary->changedVoxels = (int64_t)host.sum.changedVoxels;
		for (int a = 0; a < 3 && host.sum.changedColumns; a++) {
			summary->min[a] = host.sum.min[a];
			summary->max[a] = host.sum.max[a];
		}
	}
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxsnap

extern "C" {

int cvx_world_snapshot(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, int levelCount, cvx_snapshot **out, float *outDeviceMs)
{
	static const char *const call = "cvx_world_snapshot";
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!out) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: out is NULL", call); }
	*out = nullptr;
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const DevWorld &W = ctx->hostWorld;
	const int64_t x1 = std::min<int64_t>((int64_t)x0 + sizeX, W.dimX), z1 = std::min<int64_t>((int64_t)z0 + sizeZ, W.dimZ);
	if (sizeX < 1 || sizeZ < 1 || std::max(x0, 0) >= x1 || std::max(z0, 0) >= z1) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "rectangle (%d, %d) + %d x %d does not meet the world's %d x %d columns", x0, z0, sizeX, sizeZ, W.dimX, W.dimZ);
	}
	cvxi::EditRectangle R{};
	int rc = cvxi::RoundEditRectangle(ctx, std::max(x0, 0), x1, std::max(z0, 0), z1, levelCount, "a snapshot of", &R);
	if (rc != CVX_OK) { return rc; }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	cvx_snapshot *snap = new (std::nothrow) cvx_snapshot();
	if (!snap) { return Fail(ctx, CVX_ERR_CAPACITY, "%s: no host memory", call); }
	struct Holder { // (the blobs are the call's until the snapshot is complete)
		cvx_snapshot *s;
		~Holder() { delete s; }
	} holder{ snap };
	snap->ctx = ctx;
	snap->device = ctx->device;
	snap->info = cvx_snapshot_info{ R.x0, R.z0, R.sizeX, R.sizeZ, levelCount, W.dimX, W.dimY, W.dimZ, 0, 0 };

	cvxi::DeviceCall D(ctx, call);
	cvxi::RegionRead reads[CVX_LOD_LEVELS];
	hipError_t e = D.Begin();
	// count and scan every level, ONE synchronisation for all totals
	for (int k = 0; k <= levelCount && e == hipSuccess; k++) {
		reads[k] = cvxi::RegionRead{ k, R.x0 >> k, R.z0 >> k, R.sizeX >> k, R.sizeZ >> k, nullptr, 0 };
		e = cvxi::RegionReadCount(ctx, D, &reads[k]);
	}
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	uint8_t *blobs[CVX_LOD_LEVELS] = {};
	for (int k = 0; k <= levelCount; k++) {
		if (reads[k].total >= ((unsigned long long)1 << 31)) { // (storageOffset is an int32)
			return Fail(ctx, CVX_ERR_CAPACITY, "LOD %d: the snapshot needs %llu elements", k, reads[k].total);
		}
	}
	// the blobs, each in memory of its own
	for (int k = 0; k <= levelCount && e == hipSuccess; k++) {
		const size_t headerBytes = (size_t)reads[k].sizeX * (size_t)reads[k].sizeZ * 12, bytes = headerBytes + (size_t)reads[k].total * 4;
		e = D.Allocate(&blobs[k], bytes);
		if (e == hipSuccess) { e = cvxi::RegionReadWrite(ctx, reads[k], blobs[k], headerBytes); }
		snap->info.deviceBytes += (int64_t)bytes;
		snap->info.elements += (int64_t)reads[k].total;
	}
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	for (int k = 0; k <= levelCount; k++) { snap->blob[k] = D.Keep(blobs[k]); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	holder.s = nullptr;
	*out = snap;
	return CVX_OK;
}

int cvx_snapshot_info_get(const cvx_snapshot *snap, cvx_snapshot_info *out)
{
	if (!snap || !out) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_snapshot_info_get: a NULL pointer"); }
	*out = snap->info;
	return CVX_OK;
}

int cvx_world_snapshot_restore(cvx_context *ctx, const cvx_snapshot *snap, float *outDeviceMs)
{
	static const char *const call = "cvx_world_snapshot_restore";
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	int rc = cvxsnap::CheckPair(ctx, snap, call);
	if (rc == CVX_OK) { rc = cvxsnap::CheckWorld(ctx, snap, call); }
	if (rc != CVX_OK) { return rc; }
	const cvx_snapshot_info &I = snap->info;
	const uint32_t *headers[CVX_LOD_LEVELS], *elements[CVX_LOD_LEVELS];
	for (int k = 0; k <= I.levelCount; k++) {
		headers[k] = reinterpret_cast<const uint32_t *>(snap->blob[k]);
		elements[k] = reinterpret_cast<const uint32_t *>(snap->blob[k] + (size_t)(I.sizeX >> k) * (size_t)(I.sizeZ >> k) * 12);
	}
	cvxi::DeviceCall D(ctx, call);
	const hipError_t e = D.Begin();
	if (e != hipSuccess) { return D.Fail(e, CVX_ERR_HIP); }
	rc = cvxi::PatchLevelsFromDevice(ctx, I.x0, I.z0, I.sizeX, I.sizeZ, headers, elements, I.levelCount, D.Event(1));
	if (rc == CVX_OK && outDeviceMs) { *outDeviceMs = D.Ms(); }
	return rc;
}

int cvx_world_snapshot_diff(cvx_context *ctx, const cvx_snapshot *snap, int flags, cvx_snapshot_change *changes, int64_t changeCapacity,
                            cvx_snapshot_diff_summary *summary, float *outDeviceMs)
{
	return cvxsnap::Diff(ctx, "cvx_world_snapshot_diff", snap, flags, changes, false, changeCapacity, summary, outDeviceMs);
}

int cvx_world_snapshot_diff_device(cvx_context *ctx, const cvx_snapshot *snap, int flags, cvx_snapshot_change *changesDevice, int64_t changeCapacity,
                                   cvx_snapshot_diff_summary *summary, float *outDeviceMs)
{
	return cvxsnap::Diff(ctx, "cvx_world_snapshot_diff_device", snap, flags, changesDevice, true, changeCapacity, summary, outDeviceMs);
}

void cvx_snapshot_destroy(cvx_snapshot *snap)
{
	if (!snap) { return; }
	(void)hipSetDevice(snap->device);
	for (uint8_t *b : snap->blob) { if (b) { (void)hipFree(b); } }
	delete snap;
}

} // extern "C"
