// cvx_dense.hip -- libcpuvox_gpu.so, dense voxel boxes out of and into the device-resident world (cvx_world_read_voxels[_device],
// cvx_world_write_voxels[_device]).  See include/cpuvox_gpu.h for the contract and cvx_dense.h for the rules.
//
// A read is one kernel, a thread per element of the arrays: consecutive lanes are consecutive y of a column and go on into the next column (z,
// then x) where the box is lower than a wave, so the stores are contiguous whatever the box's height.  Each lane finds its voxel with a binary
// search of its column's runs (cvxb::DenseVoxel).
// A write is a brush whose columns come from the dense arrays; steps 2 .. 4 are cvxi::ColumnEdit (cvx_edit.hip), the count and the write kernel what
// it launches:
//   1. count  (a WAVE per LOD-0 column of the rounded rectangle): the column top-down, 64 voxels per step; every lane evaluates its voxel
//             (cvxb::DenseFinal: the arrays inside the box, read contiguously, the arena elsewhere), a ballot gives the step's solid mask, its
//             changes against itself shifted by one voxel the run starts, popcounts the run and colour counts; the steps between
//             one run of the arena (or the box) and the next hold nothing but air and are taken in one go (a wave-uniform cursor over the
//             column's runs), so a tall column costs its few live steps; columns the format cannot hold raise a flag
//   2. the counts are prefix-scanned into element offsets; ONE copy brings the total and the flag to the host
//   3. write  (same waves): the same walk; a lane that starts a run writes it when it ends at the next start of its step, prefix popcounts
//             (mbcnt) give it its run slot and every solid lane its colour slot; the run that crosses a step is carried in wave-uniform state
//   4. cvxi::EditFromDevice: the blob goes through cvx_world_edit's machinery (records, tails, growth, LOD 1 .. levelCount) unchanged.
// Nothing in the arena is written before step 4, so a rejected write leaves the world as it was.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cvx_context.h"
#include "cvx_dense.h"

using cvxi::Fail;

namespace cvxdense {

constexpr unsigned kThreads = 256;
constexpr int kWavesPerBlock = kThreads / CVX_WAVE;

struct ReadArgs {
	cvxb::CopyWorld W;
	cvxb::DenseBox box;
	uint32_t n; // elements
	uint32_t *argb;
	uint8_t *solid;
};

__global__ __launch_bounds__(kThreads) void dense_read_kernel(ReadArgs A)
{
	const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t sizeY = (uint32_t)A.box.size[1], sizeZ = (uint32_t)A.box.size[2];
	const uint32_t column = i / sizeY, y = i - column * sizeY;
	const uint32_t x = column / sizeZ, z = column - x * sizeZ;
	const cvxb::Voxel v = cvxb::DenseVoxel(A.W, (int64_t)A.box.min[0] + x, (int64_t)A.box.min[1] + y, (int64_t)A.box.min[2] + z);
	if (A.argb) { A.argb[i] = v.argb; }
	if (A.solid) { A.solid[i] = v.solid ? 1 : 0; }
}

struct WriteArgs {
	cvxb::CopyWorld W;
	cvxb::DenseBox box;
	const uint32_t *argb;
	const uint8_t *solid;
	int op;
	int x0, z0, sizeZ, n;
	uint32_t *counts;     // per column: elements (-> offset after the scan)
	uint32_t *runCounts;  // per column: runs (0: the column is empty)
	unsigned int *overLimit;
	uint32_t *headers;    // write: the sub-world blob, n headers of 3 words
	uint32_t *elements;
};

// The wave's walk of column `i` of the rectangle (the steps of cvx_dense.h).  kWrite: runs go to outRuns, colours to outColours
// (cvxb::DenseColumn's out arrays).  Everything but y, the voxel and the lane's slots is the same in all lanes.
template <bool kWrite>
__device__ __forceinline__ cvxb::BrushResult WalkColumn(const WriteArgs &A, int i, int lane, uint32_t *outRuns, uint32_t *outColours)
{
	const int64_t cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const cvxb::ArenaColumn col = cvxb::CopyColumnAt(A.W, cx, cz);
	const int dimY = A.W.dimY;
	int64_t lo, hi, base;
	cvxb::DenseSpan(A.box, cx, cz, dimY, &lo, &hi, &base);
	const uint32_t count = col.Count();
	uint32_t cursor = 0u;
	uint32_t *lane0Runs = kWrite && lane == 0 ? outRuns : nullptr;
	cvxb::DenseWalk w;
	for (int yTop = dimY - 1; yTop >= 0; yTop -= CVX_WAVE) {
		const int air = cvxb::DenseAirSteps(col, count, &cursor, lo, hi, yTop);
		if (air > 0) { // nothing but air down to the next run of the arena or the box: all those steps at once
			const int voxels = air * CVX_WAVE < yTop + 1 ? air * CVX_WAVE : yTop + 1;
			cvxb::DenseAdvanceAir(w, (uint32_t)voxels, lane0Runs);
			yTop -= (air - 1) * CVX_WAVE;
			continue;
		}
		const int y = yTop - lane;
		const uint32_t valid = (uint32_t)(yTop + 1 < CVX_WAVE ? yTop + 1 : CVX_WAVE);
		cvxb::Voxel v{ false, 0u };
		if (y >= 0) { v = cvxb::DenseFinal(col, A.W.colourSlots, A.W.colorShift, lo <= y && y < hi, base + y, A.argb, A.solid, A.op, y); }
		const uint64_t mask = __ballot(v.solid); // bit l: the voxel yTop - l
		const uint64_t starts = cvxb::DenseStarts(w, mask, valid);
		if (kWrite) {
			const uint32_t solidBelow = cvxi::LanesBelow(mask);
			cvxb::DenseLaneRun(w, mask, starts, lane, cvxi::LanesBelow(starts), solidBelow, outRuns);
			if (v.solid) { outColours[w.colours + solidBelow] = v.argb; }
		}
		cvxb::DenseAdvance(w, mask, starts, valid, yTop, lane0Runs);
	}
	return cvxb::DenseFinish(w, lane0Runs);
}

__global__ __launch_bounds__(kThreads) void dense_count_kernel(WriteArgs A)
{
	const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / CVX_WAVE));
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	if (i >= A.n) { return; }
	const cvxb::BrushResult r = WalkColumn<false>(A, i, lane, nullptr, nullptr);
	if (lane != 0) { return; }
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
	A.runCounts[i] = r.runCount;
}

__global__ __launch_bounds__(kThreads) void dense_write_kernel(WriteArgs A)
{
	const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / CVX_WAVE));
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	if (i >= A.n) { return; }
	const uint32_t off = A.counts[i], runCount = A.runCounts[i];
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (runCount == 0u) {
		if (lane < 3) { h[lane] = 0u; }
		return;
	}
	uint32_t *e = A.elements + off;
	// (the count kernel left the run count: the colours go behind the runs' second guard in the same walk)
	const cvxb::BrushResult r = WalkColumn<true>(A, i, lane, e + 1, e + runCount + 2u);
	if (lane != 0) { return; }
	e[0] = 0u;
	e[runCount + 1u] = 0u;
	h[0] = off;
	h[1] = runCount | (r.worldMin << 16);
	h[2] = r.worldMax;
}

} // namespace cvxdense

namespace {

using cvxdense::kThreads;
using cvxi::Grid;

int Read(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], uint32_t *argb, uint8_t *solid, bool device, void *hipStream,
         float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxdense::ReadArgs A{};
	int64_t n = 0;
	char bad[cvxb::kBoxMessage];
	if (cvxb::DenseBoxCheck(boxMin, boxMax, &A.box, &n, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, bad); }
	if (!argb && !solid) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: argb and solid are both NULL", call); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }
	A.W = cvxi::WorldOf(ctx);
	A.n = (uint32_t)n;
	void *const to[3] = { argb, solid, nullptr };
	const size_t bytes[3] = { (size_t)n * 4, (size_t)n, 0 };
	return cvxi::ReadArrays(
		ctx, call, to, bytes, device, hipStream,
		[&](const cvxi::ReadArraysJob &J) {
			A.argb = static_cast<uint32_t *>(J.array[0]);
			A.solid = static_cast<uint8_t *>(J.array[1]);
			hipLaunchKernelGGL(cvxdense::dense_read_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, J.stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

// Both writes: `device` says where argb / solid live.
int Write(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], const uint32_t *argb, const uint8_t *solid, bool device, int op,
          int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxdense::WriteArgs A{};
	int64_t elements = 0;
	char bad[cvxb::kBoxMessage];
	if (cvxb::DenseBoxCheck(boxMin, boxMax, &A.box, &elements, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, bad); }
	if (op < CVX_BRUSH_FILL || op > CVX_COPY_REPLACE) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: bad op %d", call, op); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (!argb && !(op == CVX_BRUSH_CARVE && solid)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: argb is NULL (only a CARVE with a solid mask may leave it out)", call); }
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
	int rc = cvxi::RoundEditRectangle(ctx, lo[0], hi[0], lo[2], hi[2], levelCount, "a write over", &R);
	if (rc == CVX_OK) { rc = cvxi::PrepareWorld(ctx); }
	if (rc != CVX_OK) { return rc; }

	// host arrays: a device copy of them, uploaded behind the pipeline's start so that outDeviceMs covers it
	cvxi::DeviceCall upload(ctx, call);
	uint8_t *dense = nullptr;
	const size_t argbBytes = argb ? ((size_t)elements * 4 + 15) & ~(size_t)15 : 0, solidBytes = solid ? (size_t)elements : 0;
	if (!device) {
		const hipError_t e = upload.Allocate(&dense, argbBytes + solidBytes);
		if (e != hipSuccess) { return upload.Fail(e); }
	}
	A.W = cvxi::WorldOf(ctx);
	A.argb = device ? argb : (argb ? reinterpret_cast<const uint32_t *>(dense) : nullptr);
	A.solid = device ? solid : (solid ? dense + argbBytes : nullptr);
	A.op = op;
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	const dim3 grid(Grid((size_t)R.n, cvxdense::kWavesPerBlock)), block(kThreads);
	cvxi::ColumnEditCall edit{ call, CVX_ERR_HIP, "a written column", "the written columns" };
	edit.extraScratchBytes = (size_t)R.n * 4; // the run counts
	return cvxi::ColumnEdit(
		ctx, R, levelCount, edit,
		[&](const cvxi::ColumnEditJob &J) {
			hipError_t e = hipSuccess;
			if (!device && argb) { e = hipMemcpyAsync(dense, argb, (size_t)elements * 4, hipMemcpyHostToDevice, ctx->stream); }
			if (e == hipSuccess && !device && solid) { e = hipMemcpyAsync(dense + argbBytes, solid, solidBytes, hipMemcpyHostToDevice, ctx->stream); }
			A.counts = J.counts;
			A.runCounts = reinterpret_cast<uint32_t *>(J.extra);
			A.overLimit = J.overLimit;
			if (e == hipSuccess) { hipLaunchKernelGGL(cvxdense::dense_count_kernel, grid, block, 0, ctx->stream, A); }
			return e;
		},
		[&](const cvxi::ColumnEditJob &J) {
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxdense::dense_write_kernel, grid, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

} // namespace

extern "C" {

int cvx_world_read_voxels(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], uint32_t *argb, uint8_t *solid, float *outDeviceMs)
{
	return Read(ctx, "cvx_world_read_voxels", boxMin, boxMax, argb, solid, false, nullptr, outDeviceMs);
}

int cvx_world_read_voxels_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], uint32_t *argbDevice, uint8_t *solidDevice, void *hipStream)
{
	return Read(ctx, "cvx_world_read_voxels_device", boxMin, boxMax, argbDevice, solidDevice, true, hipStream, nullptr);
}

int cvx_world_write_voxels(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const uint32_t *argb, const uint8_t *solid, int op, int levelCount,
                           float *outDeviceMs)
{
	return Write(ctx, "cvx_world_write_voxels", boxMin, boxMax, argb, solid, false, op, levelCount, outDeviceMs);
}

int cvx_world_write_voxels_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const uint32_t *argbDevice, const uint8_t *solidDevice, int op,
                                  int levelCount, float *outDeviceMs)
{
	return Write(ctx, "cvx_world_write_voxels_device", boxMin, boxMax, argbDevice, solidDevice, true, op, levelCount, outDeviceMs);
}

} // extern "C"
