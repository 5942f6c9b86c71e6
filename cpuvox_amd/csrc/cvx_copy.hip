// cvx_copy.hip -- libcpuvox_gpu.so, copying, moving and rotating voxel boxes inside the device-resident world (cvx_world_copy).  See
// include/cpuvox_gpu.h for the contract and cvx_copy.h for the column rule.
//
// A copy is a brush whose columns are composed from other columns of the arena, step for step cvx_world_brush:
//   1. count  (a thread per LOD-0 column of the rounded rectangle): the column after the placements (cvxb::CopyColumn), the elements its new
//             column needs ([guard][runs][guard][colours]); columns the format cannot hold raise a flag
//   2. the counts are prefix-scanned into element offsets; ONE copy brings the total and the flag to the host
//   3. write  (same threads): the sub-world blob in the reference's layout, 12-byte RLEColumn headers then the element pool
//   4. cvxi::EditFromDevice: the blob goes through cvx_world_edit's machinery (records, tails, growth, LOD 1 .. levelCount) unchanged.
// Nothing in the arena is written before step 4: every source voxel is read from the world as it was before the call, which is what makes
// overlapping sources and destinations safe, and a rejected copy leaves the world as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cvx_context.h"
#include "cvx_copy.h"

using cvxi::Fail;

namespace cvxcopy {

struct CopyArgs {
	cvxb::CopyWorld W;
	int x0, z0, sizeZ, n;
	const cvx_copy_placement *placements;
	int placementCount;
	uint32_t *counts;              // per column: elements (-> offset after the scan)
	unsigned int *overLimit;
	uint32_t *headers;             // write: the sub-world blob, n headers of 3 words
	uint32_t *elements;
};

__global__ __launch_bounds__(256) void copy_count_kernel(CopyArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const cvxb::BrushResult r = cvxb::CopyColumn(A.W, A.placements, A.placementCount, cx, cz, nullptr, nullptr);
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = r.runCount ? r.runCount + 2u + r.colours : 0u;
}

__global__ __launch_bounds__(256) void copy_write_kernel(CopyArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	// (the colours go behind the runs' second guard, a place known once the runs are counted: the walk runs twice, the second time writing)
	const cvxb::BrushResult r = cvxb::CopyColumn(A.W, A.placements, A.placementCount, cx, cz, nullptr, nullptr);
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (r.runCount == 0u) {
		h[0] = 0u;
		h[1] = 0u;
		h[2] = 0u;
		return;
	}
	cvxb::CopyColumn(A.W, A.placements, A.placementCount, cx, cz, e + 1, e + r.runCount + 2u);
	e[0] = 0u;
	e[r.runCount + 1u] = 0u;
	h[0] = off;
	h[1] = r.runCount | (r.worldMin << 16);
	h[2] = r.worldMax;
}

} // namespace cvxcopy

namespace {

constexpr unsigned kThreads = 256;

unsigned Grid(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// Grows [x0, x1) x [z0, z1) by the columns [a0, a1) x [b0, b1)
void Cover(int64_t a0, int64_t a1, int64_t b0, int64_t b1, int64_t *x0, int64_t *x1, int64_t *z0, int64_t *z1)
{
	*x0 = std::min(*x0, a0);
	*x1 = std::max(*x1, a1);
	*z0 = std::min(*z0, b0);
	*z1 = std::max(*z1, b1);
}

} // namespace

extern "C" {

int cvx_world_copy(cvx_context *ctx, const cvx_copy_placement *placements, int placementCount, int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!placements || placementCount <= 0 || placementCount > CVX_COPY_MAX_PLACEMENTS) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placementCount %d outside 1 .. %d", placementCount, CVX_COPY_MAX_PLACEMENTS);
	}
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	for (int i = 0; i < placementCount; i++) {
		const cvx_copy_placement &p = placements[i];
		if (p.op < CVX_BRUSH_FILL || p.op > CVX_COPY_REPLACE) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placement %d: bad op %d", i, p.op); }
		if (p.move != 0 && p.move != 1) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placement %d: move %d is not 0 or 1", i, p.move); }
		if (p.transform & ~15) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placement %d: unknown transform bits 0x%x", i, (unsigned)p.transform); }
		for (int a = 0; a < 3; a++) {
			if (p.dst[a] < -(1 << 30) || p.dst[a] > (1 << 30)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placement %d: |dst[%d]| = %d above 2^30", i, a, p.dst[a]); }
			if (p.srcMin[a] < 0 || p.srcMin[a] >= p.srcMax[a]) {
				return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placement %d: source box [%d, %d) on axis %d is empty or outside the world", i, p.srcMin[a], p.srcMax[a], a);
			}
		}
	}
	if (!ctx->levelSet[0]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD 0 has not been uploaded"); }
	const int dim[3] = { ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ };
	for (int i = 0; i < placementCount; i++) {
		const cvx_copy_placement &p = placements[i];
		for (int a = 0; a < 3; a++) {
			if (p.srcMax[a] > dim[a]) {
				return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "placement %d: source box [%d, %d) on axis %d is outside the world (0 .. %d)", i, p.srcMin[a], p.srcMax[a], a,
				            dim[a]);
			}
		}
	}
	// the placements that change something, and the rectangle: every clipped destination footprint and every moving source footprint, rounded
	// out to 2^levelCount, clipped to the world
	std::vector<cvx_copy_placement> live;
	int64_t x0 = INT64_MAX, x1 = INT64_MIN, z0 = INT64_MAX, z1 = INT64_MIN;
	for (int i = 0; i < placementCount; i++) {
		const cvx_copy_placement &p = placements[i];
		int64_t sizeX, sizeZ;
		cvxb::CopyDestinationSize(p, &sizeX, &sizeZ);
		const int64_t size[3] = { sizeX, (int64_t)p.srcMax[1] - p.srcMin[1], sizeZ };
		int64_t lo[3], hi[3];
		bool writes = true;
		for (int a = 0; a < 3; a++) {
			lo[a] = std::max<int64_t>(p.dst[a], 0);
			hi[a] = std::min<int64_t>((int64_t)p.dst[a] + size[a], dim[a]);
			writes = writes && lo[a] < hi[a];
		}
		if (writes) { Cover(lo[0], hi[0], lo[2], hi[2], &x0, &x1, &z0, &z1); }
		if (p.move) { Cover(p.srcMin[0], p.srcMax[0], p.srcMin[2], p.srcMax[2], &x0, &x1, &z0, &z1); }
		if (writes || p.move) { live.push_back(p); }
	}
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	if (live.empty()) { return CVX_OK; }
	const int64_t align = ((int64_t)1 << levelCount) - 1;
	x0 &= ~align;
	z0 &= ~align;
	x1 = std::min<int64_t>((x1 + align) & ~align, dim[0]);
	z1 = std::min<int64_t>((z1 + align) & ~align, dim[2]);
	if (((x1 - x0) & align) || ((z1 - z0) & align)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the world (%d x %d columns) is narrower than 2^levelCount = %lld", dim[0], dim[2], (long long)align + 1);
	}
	const int sizeX = (int)(x1 - x0), sizeZ = (int)(z1 - z0);
	const int n = sizeX * sizeZ;
	if ((int64_t)sizeX * sizeZ >= ((int64_t)1 << 31) / 12) { return Fail(ctx, CVX_ERR_CAPACITY, "a copy over %d x %d columns", sizeX, sizeZ); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	int rc = cvxi::SyncWorld(ctx);
	if (rc != CVX_OK) { return rc; }

	hipEvent_t ev[2] = { nullptr, nullptr };
	uint8_t *scratch = nullptr, *dSrc = nullptr;
	auto release = [&]() {
		if (scratch) { (void)hipFree(scratch); }
		if (dSrc) { (void)hipFree(dSrc); }
		for (hipEvent_t e : ev) { if (e) { (void)hipEventDestroy(e); } }
	};
	const size_t chunks = ((size_t)n + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
	size_t bytes = 0;
	auto carve = [&](size_t b) { const size_t at = bytes; bytes = (bytes + b + 15) & ~(size_t)15; return at; };
	const size_t oPlacements = carve(live.size() * sizeof(cvx_copy_placement)), oCounts = carve((size_t)n * 4), oTotals = carve(2 * 8),
	             oChunks = carve(chunks * 8);
	struct { unsigned long long total, overLimit; } host = { 0, 0 };
	cvxcopy::CopyArgs A{};
	hipError_t e = hipEventCreate(&ev[0]);
	if (e == hipSuccess) { e = hipEventCreate(&ev[1]); }
	if (e == hipSuccess) { e = hipMalloc((void **)&scratch, bytes); }
	if (e == hipSuccess) { e = hipEventRecord(ev[0], ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + oPlacements, live.data(), live.size() * sizeof(cvx_copy_placement), hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) { e = hipMemsetAsync(scratch + oTotals, 0, 2 * 8, ctx->stream); }
	if (e == hipSuccess) {
		const DevWorldLevel &L = ctx->hostWorld.level[0];
		A.W.records = reinterpret_cast<const uint32_t *>(ctx->arena + L.recordsOff);
		A.W.runs = reinterpret_cast<const uint32_t *>(ctx->arena + L.runsOff);
		A.W.colourSlots = reinterpret_cast<const uint32_t *>(ctx->arena + L.elementsOff);
		A.W.rowShift = L.rowShift;
		A.W.colorShift = L.colorShift;
		A.W.dimX = dim[0];
		A.W.dimY = dim[1];
		A.W.dimZ = dim[2];
		A.x0 = (int)x0;
		A.z0 = (int)z0;
		A.sizeZ = sizeZ;
		A.n = n;
		A.placements = reinterpret_cast<const cvx_copy_placement *>(scratch + oPlacements);
		A.placementCount = (int)live.size();
		A.counts = reinterpret_cast<uint32_t *>(scratch + oCounts);
		unsigned long long *totals = reinterpret_cast<unsigned long long *>(scratch + oTotals);
		A.overLimit = reinterpret_cast<unsigned int *>(totals + 1);
		// 1, 2. count, scan, one copy back
		hipLaunchKernelGGL(cvxcopy::copy_count_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.counts, n, reinterpret_cast<unsigned long long *>(scratch + oChunks), totals);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host, totals, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) {
		release();
		return Fail(ctx, CVX_ERR_HIP, "copy failed: %s", hipGetErrorString(e));
	}
	if (host.overLimit) {
		release();
		return Fail(ctx, CVX_ERR_CAPACITY, "a copied column would need more than 65535 runs, a run longer than 32767 voxels or a colour index above 32767");
	}
	if (host.total >= ((unsigned long long)1 << 31) - (unsigned long long)n * 3) {
		release();
		return Fail(ctx, CVX_ERR_CAPACITY, "the copied columns need %llu elements", host.total);
	}
	// 3. the sub-world blob
	const size_t blobBytes = (size_t)n * 12 + (size_t)host.total * 4;
	e = hipMalloc((void **)&dSrc, std::max<size_t>(blobBytes, 4));
	if (e == hipSuccess) {
		A.headers = reinterpret_cast<uint32_t *>(dSrc);
		A.elements = reinterpret_cast<uint32_t *>(dSrc + (size_t)n * 12);
		hipLaunchKernelGGL(cvxcopy::copy_write_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, A);
		e = hipGetLastError();
	}
	if (e != hipSuccess) {
		release();
		return Fail(ctx, CVX_ERR_HIP, "copy failed: %s", hipGetErrorString(e));
	}
	// 4. cvx_world_edit's machinery
	rc = cvxi::EditFromDevice(ctx, (int)x0, (int)z0, sizeX, sizeZ, dSrc, (int64_t)host.total, n, levelCount, ev[1]);
	if (rc == CVX_OK && outDeviceMs) {
		float ms = 0.f;
		e = hipEventElapsedTime(&ms, ev[0], ev[1]);
		*outDeviceMs = e == hipSuccess ? ms : 0.f;
	}
	release();
	return rc;
}

} // extern "C"
