// cvx_copy.hip -- libcpuvox_gpu.so, copying, moving and rotating voxel boxes inside the device-resident world (cvx_world_copy).  See
// include/cpuvox_gpu.h for the contract and cvx_copy.h for the column rule.
//
// A copy is a brush whose columns are composed from other columns of the arena; steps 2 .. 4 are cvxi::ColumnEdit (cvx_edit.hip), the count and the
// write kernel what it launches:
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
	A.counts[i] = cvxb::BlobElements(r);
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
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::CopyColumn(A.W, A.placements, A.placementCount, cx, cz, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
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
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
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
	cvxi::EditRectangle R;
	int rc = cvxi::RoundEditRectangle(ctx, x0, x1, z0, z1, levelCount, "a copy over", &R);
	if (rc != CVX_OK) { return rc; }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	const size_t placementBytes = live.size() * sizeof(cvx_copy_placement);
	cvxcopy::CopyArgs A{};
	A.W = cvxi::WorldOf(ctx);
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	A.placementCount = (int)live.size();
	cvxi::ColumnEditCall call{ "copy", CVX_ERR_HIP, "a copied column", "the copied columns" };
	call.extraScratchBytes = placementBytes;
	return cvxi::ColumnEdit(
		ctx, R, levelCount, call,
		[&](const cvxi::ColumnEditJob &J) {
			A.placements = reinterpret_cast<const cvx_copy_placement *>(J.extra);
			A.counts = J.counts;
			A.overLimit = J.overLimit;
			const hipError_t e = hipMemcpyAsync(J.extra, live.data(), placementBytes, hipMemcpyHostToDevice, ctx->stream);
			if (e == hipSuccess) { hipLaunchKernelGGL(cvxcopy::copy_count_kernel, dim3(Grid((size_t)R.n)), dim3(kThreads), 0, ctx->stream, A); }
			return e;
		},
		[&](const cvxi::ColumnEditJob &J) {
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxcopy::copy_write_kernel, dim3(Grid((size_t)R.n)), dim3(kThreads), 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

} // extern "C"
