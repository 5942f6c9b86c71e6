// cvx_heights.hip -- libcpuvox_gpu.so, terrain as height maps out of and into the device-resident world (cvx_world_read_heights[_device],
// cvx_world_write_heights[_device]).  See include/cpuvox_gpu_heights.h for the contract and cvx_heights.h for the rules.
//
// A read is one kernel, a thread per column of the footprint: consecutive lanes are consecutive z, so the loads of the records and the stores of
// the three arrays are contiguous.  Each lane finds the run at the window's top with one binary search (cvxb::HeightsTop); no voxel is scanned.
// A write is a brush whose one interval per column comes from the height arrays; steps 2 .. 4 are cvxi::ColumnEdit (cvx_edit.hip), the count and
// the write kernel what it launches:
//   1. count  (a thread per LOD-0 column of the rounded rectangle): the column from the arena, its [b, H) from the arrays (at most five loads of
//             the heights, adjacent in z and in rows), walked span by span (cvxb::HeightsColumn); the elements and the runs its new column needs;
//             columns the format cannot hold raise a flag.  Columns of the rectangle outside the footprint re-emit the arena's column.
//   2. the counts are prefix-scanned into element offsets; ONE copy brings the total and the flag to the host
//   3. write  (same threads): the same walk, writing the runs and, behind their second guard (the count kernel left the run count), the colours
//   4. cvxi::EditFromDevice: the blob goes through cvx_world_edit's machinery (records, tails, growth, LOD 1 .. levelCount) unchanged.
// Nothing in the arena is written before step 4, so a rejected write leaves the world as it was.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cvx_box.h"
#include "cvx_context.h"
#include "cvx_heights.h"

using cvxi::Fail;

namespace cvxheights {

constexpr unsigned kThreads = 256;

struct ReadArgs {
	cvxb::CopyWorld W;
	cvxb::HeightsBox box;
	uint32_t n; // columns of the footprint
	int32_t *heights;
	uint32_t *argb;
	int32_t *bottoms;
};

__global__ __launch_bounds__(kThreads) void heights_read_kernel(ReadArgs A)
{
	const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t sizeZ = (uint32_t)A.box.sizeZ;
	const uint32_t x = i / sizeZ, z = i - x * sizeZ;
	const cvxb::HeightsRead r = cvxb::HeightsTop(A.W, A.box, (int64_t)A.box.x0 + x, (int64_t)A.box.z0 + z);
	if (A.heights) { A.heights[i] = r.height; }
	if (A.argb) { A.argb[i] = r.argb; }
	if (A.bottoms) { A.bottoms[i] = r.bottom; }
}

struct WriteArgs {
	cvxb::CopyWorld W;
	cvxb::HeightsBox box;
	cvxb::HeightsArrays arrays;
	int op;
	int x0, z0, sizeZ, n; // the rounded rectangle
	uint32_t *counts;     // per column: elements (-> offset after the scan)
	uint32_t *runCounts;  // per column: runs (0: the column is empty)
	unsigned int *overLimit;
	uint32_t *headers;    // write: the sub-world blob, n headers of 3 words
	uint32_t *elements;
};

__global__ __launch_bounds__(kThreads) void heights_count_kernel(WriteArgs A)
{
	const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
	if (i >= A.n) { return; }
	const int64_t cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const cvxb::BrushResult r = cvxb::HeightsColumn(cvxb::CopyColumnAt(A.W, cx, cz), A.W.colourSlots, A.W.colorShift, A.box, A.arrays, A.op, cx, cz, A.W.dimY,
	                                                nullptr, nullptr);
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
	A.runCounts[i] = r.runCount;
}

__global__ __launch_bounds__(kThreads) void heights_write_kernel(WriteArgs A)
{
	const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
	if (i >= A.n) { return; }
	const int64_t cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const uint32_t off = A.counts[i], runCount = A.runCounts[i];
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	uint32_t *e = A.elements + off;
	const cvxb::BrushResult r = cvxb::HeightsColumn(cvxb::CopyColumnAt(A.W, cx, cz), A.W.colourSlots, A.W.colorShift, A.box, A.arrays, A.op, cx, cz, A.W.dimY,
	                                                e + 1, e + runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

} // namespace cvxheights

namespace {

using cvxheights::kThreads;
using cvxi::Grid;

// The checks both directions share; *columns receives the footprint's column count.
int CheckBox(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], cvxb::HeightsBox *box, int64_t *columns)
{
	char bad[cvxb::kBoxMessage];
	if (cvxb::BoxCheck(boxMin, boxMax, cvxb::kBoxWithin | cvxb::kBoxFootprint, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, bad); }
	const int64_t sizeX = (int64_t)boxMax[0] - boxMin[0], sizeZ = (int64_t)boxMax[2] - boxMin[2];
	*box = cvxb::HeightsBox{ boxMin[0], boxMin[2], (int32_t)sizeX, (int32_t)sizeZ, boxMin[1], boxMax[1] };
	*columns = sizeX * sizeZ;
	return CVX_OK;
}

int Read(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int32_t *heights, uint32_t *argb, int32_t *bottoms, bool device,
         void *hipStream, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxheights::ReadArgs A{};
	int64_t n = 0;
	int rc = CheckBox(ctx, call, boxMin, boxMax, &A.box, &n);
	if (rc != CVX_OK) { return rc; }
	if (!heights && !argb && !bottoms) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: heights, argb and bottoms are all NULL", call); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }
	A.W = cvxi::WorldOf(ctx);
	A.n = (uint32_t)n;
	void *const to[3] = { heights, argb, bottoms };
	const size_t bytes[3] = { (size_t)n * 4, (size_t)n * 4, (size_t)n * 4 };
	return cvxi::ReadArrays(
		ctx, call, to, bytes, device, hipStream,
		[&](const cvxi::ReadArraysJob &J) {
			A.heights = static_cast<int32_t *>(J.array[0]);
			A.argb = static_cast<uint32_t *>(J.array[1]);
			A.bottoms = static_cast<int32_t *>(J.array[2]);
			hipLaunchKernelGGL(cvxheights::heights_read_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, J.stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

// Both writes: `device` says where the three arrays live.
int Write(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], const int32_t *heights, const uint32_t *argb, const uint32_t *sideArgb,
          bool device, int thickness, int flags, int op, int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxheights::WriteArgs A{};
	int64_t columns = 0;
	int rc = CheckBox(ctx, call, boxMin, boxMax, &A.box, &columns);
	if (rc != CVX_OK) { return rc; }
	if (op < CVX_BRUSH_FILL || op > CVX_COPY_REPLACE) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: bad op %d", call, op); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (!heights) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: heights is NULL", call); }
	if (!argb && op != CVX_BRUSH_CARVE) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: argb is NULL (only a CARVE may leave it out)", call); }
	if (thickness < 0 || thickness > 32767) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: thickness %d outside 0 .. 32767", call, thickness); }
	if (flags & ~CVX_HEIGHTS_WALLED) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", call, (unsigned)(flags & ~CVX_HEIGHTS_WALLED)); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int dim[3] = { ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ };
	// the rectangle: the box clipped to the world, its footprint rounded out to 2^levelCount, clipped again
	int64_t lo[3], hi[3];
	bool touches = true;
	for (int a = 0; a < 3; a++) {
		lo[a] = std::max<int64_t>(boxMin[a], 0);
		hi[a] = std::min<int64_t>(boxMax[a], dim[a]);
		touches = touches && lo[a] < hi[a];
	}
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	if (!touches) { return CVX_OK; }
	cvxi::EditRectangle R;
	rc = cvxi::RoundEditRectangle(ctx, lo[0], hi[0], lo[2], hi[2], levelCount, "a height map over", &R);
	if (rc == CVX_OK) { rc = cvxi::PrepareWorld(ctx); }
	if (rc != CVX_OK) { return rc; }

	// host arrays: a device copy of them, uploaded behind the pipeline's start so that outDeviceMs covers it
	cvxi::DeviceCall upload(ctx, call);
	uint32_t *copy = nullptr;
	const void *const host[3] = { heights, argb, sideArgb };
	const uint32_t *dev[3] = { reinterpret_cast<const uint32_t *>(heights), argb, sideArgb };
	const size_t arrayBytes = (size_t)columns * 4;
	if (!device) {
		size_t arrays = 0;
		for (const void *p : host) { arrays += p ? 1 : 0; }
		const hipError_t e = upload.Allocate(&copy, arrays * arrayBytes);
		if (e != hipSuccess) { return upload.Fail(e); }
		size_t k = 0;
		for (int a = 0; a < 3; a++) { dev[a] = host[a] ? copy + (k++) * (size_t)columns : nullptr; }
	}
	A.W = cvxi::WorldOf(ctx);
	A.arrays = cvxb::HeightsArrays{ reinterpret_cast<const int32_t *>(dev[0]), dev[1], dev[2], thickness, flags };
	A.op = op;
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	const dim3 grid(Grid((size_t)R.n)), block(kThreads);
	cvxi::ColumnEditCall edit{ call, CVX_ERR_HIP, "a written column", "the written columns" };
	edit.extraScratchBytes = (size_t)R.n * 4; // the run counts
	return cvxi::ColumnEdit(
		ctx, R, levelCount, edit,
		[&](const cvxi::ColumnEditJob &J) {
			hipError_t e = hipSuccess;
			for (int a = 0; a < 3 && !device; a++) {
				if (e == hipSuccess && host[a]) { e = hipMemcpyAsync(const_cast<uint32_t *>(dev[a]), host[a], arrayBytes, hipMemcpyHostToDevice, ctx->stream); }
			}
			A.counts = J.counts;
			A.runCounts = reinterpret_cast<uint32_t *>(J.extra);
			A.overLimit = J.overLimit;
			if (e == hipSuccess) { hipLaunchKernelGGL(cvxheights::heights_count_kernel, grid, block, 0, ctx->stream, A); }
			return e;
		},
		[&](const cvxi::ColumnEditJob &J) {
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxheights::heights_write_kernel, grid, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

} // namespace

extern "C" {

int cvx_world_read_heights(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int32_t *heights, uint32_t *argb, int32_t *bottoms, float *outDeviceMs)
{
	return Read(ctx, "cvx_world_read_heights", boxMin, boxMax, heights, argb, bottoms, false, nullptr, outDeviceMs);
}

int cvx_world_read_heights_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int32_t *heightsDevice, uint32_t *argbDevice,
                                  int32_t *bottomsDevice, void *hipStream)
{
	return Read(ctx, "cvx_world_read_heights_device", boxMin, boxMax, heightsDevice, argbDevice, bottomsDevice, true, hipStream, nullptr);
}

int cvx_world_write_heights(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const int32_t *heights, const uint32_t *argb, const uint32_t *sideArgb,
                            int thickness, int flags, int op, int levelCount, float *outDeviceMs)
{
	return Write(ctx, "cvx_world_write_heights", boxMin, boxMax, heights, argb, sideArgb, false, thickness, flags, op, levelCount, outDeviceMs);
}

int cvx_world_write_heights_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const int32_t *heightsDevice, const uint32_t *argbDevice,
                                   const uint32_t *sideArgbDevice, int thickness, int flags, int op, int levelCount, float *outDeviceMs)
{
	return Write(ctx, "cvx_world_write_heights_device", boxMin, boxMax, heightsDevice, argbDevice, sideArgbDevice, true, thickness, flags, op, levelCount, outDeviceMs);
}

} // extern "C"
