// cvx_brush.hip -- libcpuvox_gpu.so, voxel brushes (cvx_world_brush) and ray picking (cvx_world_pick, cvx_world_pick_device) on the device-resident
// world.  See include/cpuvox_gpu.h for the contract, cvx_brush.h for the per-column rules and DESIGN.md sections 3 and 4.
//
// A brush is cvx_world_edit with the sub-world built on the device instead of uploaded; steps 2 .. 4 are cvxi::ColumnEdit (cvx_edit.hip), the count and
// the write kernel what it launches:
//   0. cull   (both kernels begin with it): each wave lists the strokes whose footprint meets its 64 columns, in stroke order, in LDS
//   1. count  (a thread per LOD-0 column of the rounded rectangle): the column from the arena, the wave's strokes in order (cvxb::BrushColumnOver), the
//             elements its new column needs ([guard][runs][guard][colours]); columns the format cannot hold raise a flag
//   2. the counts are prefix-scanned into element offsets; ONE copy brings the total and the flag to the host
//   3. write  (same threads): the sub-world blob in the reference's layout, 12-byte RLEColumn headers then the element pool
//   4. cvxi::EditFromDevice: the blob goes through cvx_world_edit's machinery (records, tails, growth, LOD 1 .. levelCount) unchanged.
// Nothing in the arena is written before step 4, so a rejected brush leaves the world as it was.
// A pick is one thread per ray (a wave per 64 rays) walking LOD 0's records (cvxb::PickRay).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "cvx_brush.h"
#include "cvx_context.h"

using cvxi::Fail;

namespace cvxbrush {

struct BrushArgs {
	const uint8_t *arena;
	uint32_t recordsOff, runsOff, elementsOff;
	int rowShift, colorShift, dimY;
	int x0, z0, sizeZ, n;
	const cvx_brush_stroke *strokes;
	int strokeCount;
	uint32_t *counts;              // per column: elements (-> offset after the scan)
	unsigned int *overLimit;
	uint32_t *headers;             // write: the sub-world blob, n headers of 3 words
	uint32_t *elements;
};

__device__ __forceinline__ cvxb::ArenaColumn Column(const BrushArgs &A, int cx, int cz)
{
	const uint4 r = reinterpret_cast<const uint4 *>(A.arena + A.recordsOff)[((size_t)cx << A.rowShift) + (size_t)cz];
	return cvxb::ArenaColumn{ r.x, r.y, r.z, r.w, reinterpret_cast<const uint32_t *>(A.arena + A.runsOff) };
}

constexpr int kBrushThreads = 256, kBrushWaves = kBrushThreads / CVX_WAVE; // the one launch width of both brush kernels: bounds, grid and the lists' size

// The strokes a wave's 64 columns can meet, as ascending indices into A.strokes (cvxb::ListedStrokes): the wave takes the XZ box of its strip of the
// rectangle (cvxb::StripBox) and walks the call's list 64 strokes at a time, a lane per stroke; a ballot and the count of the kept lanes below
// append the survivors in stroke order.  CVX_BRUSH_MAX_STROKES 16-bit indices per wave always fit: there is no overflow path.
// A wave's list is written and read by that wave alone, so the waves of a workgroup do not wait for one another: a wave-scope fence orders the
// lanes' stores before the other lanes' loads (LDS operations of one wave complete in order).  Returns the list's length.
__device__ __forceinline__ int CullStrokes(const BrushArgs &A, uint16_t (*lists)[CVX_BRUSH_MAX_STROKES], const uint16_t **outList)
{
	const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / CVX_WAVE), lane = (int)threadIdx.x % CVX_WAVE;
	const int first = (int)blockIdx.x * kBrushThreads + wave * CVX_WAVE, last = min(first + CVX_WAVE, A.n) - 1;
	uint16_t *list = lists[wave];
	int count = 0;
	if (first <= last) {
		int64_t x0, x1, z0, z1;
		cvxb::StripBox(first, last, A.x0, A.z0, A.sizeZ, &x0, &x1, &z0, &z1);
		for (int base = 0; base < A.strokeCount; base += CVX_WAVE) {
			const int s = base + lane;
			const bool keep = s < A.strokeCount && cvxb::StrokeMeetsStrip(A.strokes[s], x0, x1, z0, z1);
			const unsigned long long kept = __ballot(keep);
			if (keep) { list[count + (int)cvxi::LanesBelow(kept)] = (uint16_t)s; }
			count += __popcll(kept);
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // (a lane reads what other lanes of its wave wrote)
	__builtin_amdgcn_wave_barrier();
	*outList = list;
	return count;
}

__global__ __launch_bounds__(kBrushThreads) void brush_count_kernel(BrushArgs A)
{
	__shared__ uint16_t lists[kBrushWaves][CVX_BRUSH_MAX_STROKES];
	const uint16_t *list;
	const int listCount = CullStrokes(A, lists, &list);
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const uint32_t *colours = reinterpret_cast<const uint32_t *>(A.arena + A.elementsOff);
	const cvxb::ListedStrokes strokes{ A.strokes, list };
	const cvxb::BrushResult r = cvxb::BrushColumnOver(Column(A, cx, cz), colours, A.colorShift, strokes, listCount, cx, cz, A.dimY, nullptr, nullptr);
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(kBrushThreads) void brush_write_kernel(BrushArgs A)
{
	__shared__ uint16_t lists[kBrushWaves][CVX_BRUSH_MAX_STROKES];
	const uint16_t *list;
	const int listCount = CullStrokes(A, lists, &list);
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const uint32_t *colours = reinterpret_cast<const uint32_t *>(A.arena + A.elementsOff);
	const cvxb::ListedStrokes strokes{ A.strokes, list };
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	// (the colours go behind the runs' second guard, a place known once the runs are counted: the walk runs twice, the second time writing)
	const cvxb::ArenaColumn col = Column(A, cx, cz);
	const cvxb::BrushResult r = cvxb::BrushColumnOver(col, colours, A.colorShift, strokes, listCount, cx, cz, A.dimY, nullptr, nullptr);
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::BrushColumnOver(col, colours, A.colorShift, strokes, listCount, cx, cz, A.dimY, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

__global__ __launch_bounds__(CVX_WAVE) void pick_kernel(cvxb::PickWorld W, int rayCount, const cvx_pick_ray *rays, cvx_pick_hit *hits)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= rayCount) { return; }
	const cvx_pick_ray ray = rays[i];
	const cvxb::PickResult r = W.repeat ? cvxb::PickRayRepeat(W, ray.origin, ray.direction, ray.maxT) : cvxb::PickRay(W, ray.origin, ray.direction, ray.maxT);
	cvx_pick_hit out;
	out.voxel[0] = r.voxel[0];
	out.voxel[1] = r.voxel[1];
	out.voxel[2] = r.voxel[2];
	out.face = r.face;
	out.argb = r.argb;
	out.t = r.t;
	hits[i] = out;
}

} // namespace cvxbrush

namespace {

using cvxi::Grid;

int Prepare(cvx_context *ctx)
{
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	return cvxi::PrepareWorld(ctx);
}

// The columns [x0, x1) x [z0, z1) a stroke can touch, clipped to the world; false: none (the stroke does nothing)
bool Footprint(const cvx_brush_stroke &s, int dimX, int dimY, int dimZ, int64_t *x0, int64_t *x1, int64_t *z0, int64_t *z1)
{
	int64_t lo[3], hi[3];
	cvxb::StrokeFootprint(s, lo, hi);
	const int64_t dim[3] = { dimX, dimY, dimZ };
	for (int a = 0; a < 3; a++) {
		lo[a] = std::max<int64_t>(lo[a], 0);
		hi[a] = std::min<int64_t>(hi[a], dim[a]);
		if (lo[a] >= hi[a]) { return false; }
	}
	*x0 = lo[0];
	*x1 = hi[0];
	*z0 = lo[2];
	*z1 = hi[2];
	return true;
}

cvxb::PickWorld PickWorldOf(const cvx_context *ctx)
{
	const cvxb::CopyWorld W = cvxi::WorldOf(ctx);
	cvxb::PickWorld P;
	P.records = W.records;
	P.runs = W.runs;
	P.colours = reinterpret_cast<const uint8_t *>(W.colourSlots);
	P.rowShift = W.rowShift;
	P.colorShift = W.colorShift;
	P.dimX = W.dimX;
	P.dimY = W.dimY;
	P.dimZ = W.dimZ;
	P.repeat = ctx->worldRepeat;
	return P;
}

} // namespace

namespace cvxi {
void FreeBrushState(cvx_context *ctx)
{
	if (ctx->pickScratch) { (void)hipFree(ctx->pickScratch); }
	ctx->pickScratch = nullptr;
	ctx->pickScratchBytes = 0;
}
} // namespace cvxi

extern "C" {

int cvx_world_brush(cvx_context *ctx, const cvx_brush_stroke *strokes, int strokeCount, int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (!cvxb::StrokeCountValidate(strokes, strokeCount, message, sizeof message)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", message); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (!cvxb::StrokeShapesValidate(strokes, strokeCount, message, sizeof message)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", message); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int dimX = ctx->hostWorld.dimX, dimY = ctx->hostWorld.dimY, dimZ = ctx->hostWorld.dimZ;
	// the strokes that touch the world, and the rectangle: the union of their footprints rounded out to 2^levelCount, clipped to the world
	std::vector<cvx_brush_stroke> live;
	int64_t x0 = INT64_MAX, x1 = INT64_MIN, z0 = INT64_MAX, z1 = INT64_MIN;
	for (int s = 0; s < strokeCount; s++) {
		int64_t a0, a1, b0, b1;
		if (!Footprint(strokes[s], dimX, dimY, dimZ, &a0, &a1, &b0, &b1)) { continue; }
		live.push_back(strokes[s]);
		x0 = std::min(x0, a0);
		x1 = std::max(x1, a1);
		z0 = std::min(z0, b0);
		z1 = std::max(z1, b1);
	}
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	if (live.empty()) { return CVX_OK; }
	cvxi::EditRectangle R;
	int rc = cvxi::RoundEditRectangle(ctx, x0, x1, z0, z1, levelCount, "a brush over", &R);
	if (rc == CVX_OK) { rc = Prepare(ctx); }
	if (rc != CVX_OK) { return rc; }

	const size_t strokeBytes = live.size() * sizeof(cvx_brush_stroke);
	const DevWorldLevel &L = ctx->hostWorld.level[0];
	cvxbrush::BrushArgs A{};
	A.arena = ctx->arena;
	A.recordsOff = L.recordsOff;
	A.runsOff = L.runsOff;
	A.elementsOff = L.elementsOff;
	A.rowShift = L.rowShift;
	A.colorShift = L.colorShift;
	A.dimY = dimY;
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	A.strokeCount = (int)live.size();
	const dim3 grid(Grid((size_t)R.n, cvxbrush::kBrushThreads)), block(cvxbrush::kBrushThreads);
	cvxi::ColumnEditCall call{ "brush", CVX_ERR_HIP, "a brushed column", "the brushed columns" };
	call.extraScratchBytes = strokeBytes;
	return cvxi::ColumnEdit(
		ctx, R, levelCount, call,
		[&](const cvxi::ColumnEditJob &J) {
			A.strokes = reinterpret_cast<const cvx_brush_stroke *>(J.extra);
			A.counts = J.counts;
			A.overLimit = J.overLimit;
			const hipError_t e = hipMemcpyAsync(J.extra, live.data(), strokeBytes, hipMemcpyHostToDevice, ctx->stream);
			if (e == hipSuccess) { hipLaunchKernelGGL(cvxbrush::brush_count_kernel, grid, block, 0, ctx->stream, A); }
			return e;
		},
		[&](const cvxi::ColumnEditJob &J) {
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxbrush::brush_write_kernel, grid, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		outDeviceMs);
}

int cvx_world_pick_device(cvx_context *ctx, int rayCount, const cvx_pick_ray *raysDevice, cvx_pick_hit *hitsDevice, void *hipStream)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (rayCount < 0 || (rayCount > 0 && (!raysDevice || !hitsDevice))) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad rays / hits (rayCount %d)", rayCount); }
	int rc = Prepare(ctx);
	if (rc == CVX_OK && ctx->worldRepeat) { rc = cvxi::ValidateRepeat(ctx); }
	if (rc != CVX_OK) { return rc; }
	if (rayCount == 0) { return CVX_OK; }
	hipStream_t stream = hipStream ? static_cast<hipStream_t>(hipStream) : ctx->stream;
	hipLaunchKernelGGL(cvxbrush::pick_kernel, dim3(Grid((size_t)rayCount, CVX_WAVE)), dim3(CVX_WAVE), 0, stream, PickWorldOf(ctx), rayCount, raysDevice, hitsDevice);
	CVX_HIP(ctx, hipGetLastError());
	return CVX_OK;
}

int cvx_world_pick(cvx_context *ctx, int rayCount, const cvx_pick_ray *rays, cvx_pick_hit *hits)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (rayCount < 0 || (rayCount > 0 && (!rays || !hits))) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad rays / hits (rayCount %d)", rayCount); }
	int rc = Prepare(ctx);
	if (rc == CVX_OK && ctx->worldRepeat) {
		rc = cvxi::ValidateRepeat(ctx);
		for (int i = 0; i < rayCount && rc == CVX_OK; i++) {
			if (!(rays[i].maxT <= CVX_REPEAT_MAX_DISTANCE)) { rc = Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "repeating world: ray %d has maxT %g, above 2^20", i, (double)rays[i].maxT); }
		}
	}
	if (rc != CVX_OK) { return rc; }
	if (rayCount == 0) { return CVX_OK; }
	const size_t raysBytes = ((size_t)rayCount * sizeof(cvx_pick_ray) + 255) & ~(size_t)255, hitsBytes = (size_t)rayCount * sizeof(cvx_pick_hit);
	if (ctx->pickScratchBytes < raysBytes + hitsBytes) {
		cvxi::FreeBrushState(ctx);
		CVX_HIP(ctx, hipMalloc(&ctx->pickScratch, raysBytes + hitsBytes));
		ctx->pickScratchBytes = raysBytes + hitsBytes;
	}
	cvx_pick_ray *dRays = static_cast<cvx_pick_ray *>(ctx->pickScratch);
	cvx_pick_hit *dHits = reinterpret_cast<cvx_pick_hit *>(static_cast<uint8_t *>(ctx->pickScratch) + raysBytes);
	CVX_HIP(ctx, hipMemcpyAsync(dRays, rays, (size_t)rayCount * sizeof(cvx_pick_ray), hipMemcpyHostToDevice, ctx->stream));
	rc = cvx_world_pick_device(ctx, rayCount, dRays, dHits, nullptr);
	if (rc != CVX_OK) { return rc; }
	CVX_HIP(ctx, hipMemcpyAsync(hits, dHits, hitsBytes, hipMemcpyDeviceToHost, ctx->stream));
	CVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return CVX_OK;
}

} // extern "C"
