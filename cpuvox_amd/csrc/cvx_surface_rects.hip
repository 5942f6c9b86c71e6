// cvx_surface_rects.hip -- libcpuvox_gpu.so, the exposed faces of the device-resident world merged into rectangles (cvx_world_surface_rects,
// cvx_world_surface_rects_device, cvx_surface_rect_triangles).  See include/cpuvox_gpu_surface_rects.h for the contract and cvx_surface_rects.h
// for the rule.
//
// Over the (column, face) pairs of the clipped box, pair = column * 6 + face in the box's (x, then z) column order, a thread per pair in every kernel:
//   1. count   cvxb::SurfaceWalk with a counting sink -> the pair's strips; the unit faces are summed per workgroup in LDS and sent on with one atomic
//   2. scan    cvxi::ExclusiveScan gives every pair its first strip; the strip total comes to the host, which sizes the strip scratch by it
//   3. strips  the same walk with a storing sink: bottom, length, colour of every strip, 12 bytes
//   4. merge   the first pass (faces 0, 1 along z; 2 .. 5 along x): cvxb::RectsMergePair marks the pair's strips that start a chain against the pair
//              one column back and walks their chains forward; every strip gets its extent, 0 when it was merged.  The pairs of the side faces
//              count their rectangles here
//   5. rows    the same function over the rows of faces 2, 3 along z, the x extent part of a row's identity; their pairs count here
//   6. scan    every pair's first rectangle; ONE copy brings the totals to the host
//   7. write   (a thread per pair that has rectangles below the capacity): the strips whose extents are above 0, in the order they stand in
// Nothing is compacted between the passes and nothing is sorted: the rectangles in pair order, top-down inside a pair, are in the order of the
// contract.  A pass writes one word per strip of its own pair and reads only what the kernel before it wrote.  Nothing is written to the arena.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "cvx_context.h"
#include "cvx_surface_rects.h"

using cvxi::Fail;

namespace cvxrects {

using cvxi::Grid;
using cvxi::kThreads;

constexpr int kFaces = 6;

struct Totals {
	unsigned long long rects;      // the second scan's total
	unsigned long long strips;     // the first scan's total
	unsigned long long unitFaces;
	unsigned long long perFace[kFaces];
};
static_assert(sizeof(Totals) == sizeof(cvx_surface_rects_summary), "the totals are the summary");
static_assert(sizeof(cvxb::RectStrip) == 12 && sizeof(cvx_surface_rect) == 32, "the layouts of the contract");

struct RectsArgs {
	cvxb::CopyWorld W;
	cvxb::PiecesBox B;
	int pairs;                 // columns of the box * 6
	int solidOutside, flags;
	uint32_t *stripOffsets;    // pairs + 1: count, then the first strip of every pair
	uint32_t *rectOffsets;     // pairs + 1: count, then the first rectangle of every pair
	Totals *totals;
	cvxb::RectStrip *strips;
	uint32_t *along, *rows;    // per strip: its extent from the first pass, and from the row pass (faces 2, 3 only)
	cvx_surface_rect *rects;
	uint32_t limit;            // rectangles are written below this index
};

struct CountSink {
	uint32_t strips;
	unsigned long long unitFaces;
	CVX_HD void operator()(const cvx_surface_quad &q)
	{
		strips++;
		unitFaces += (unsigned long long)q.length;
	}
};

struct StoreSink {
	cvxb::RectStrip *strips;
	uint32_t at, end;
	CVX_HD void operator()(const cvx_surface_quad &q)
	{
		if (at < end) { strips[at] = cvxb::RectStrip{ q.voxel[1], q.length, q.argb }; } // (the count pass found `end - first`: the walk is the same)
		at++;
	}
};

__device__ inline void PairOf(const RectsArgs &A, long long i, int *column, int *face, int64_t *x, int64_t *z)
{
	*column = (int)(i / kFaces);
	*face = (int)(i % kFaces);
	*x = A.B.x0 + *column / A.B.SizeZ();
	*z = A.B.z0 + *column % A.B.SizeZ();
}

__global__ __launch_bounds__(256) void rects_count_kernel(RectsArgs A)
{
	__shared__ unsigned long long unitFaces;
	if (threadIdx.x == 0u) { unitFaces = 0ull; }
	__syncthreads();
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < A.pairs) {
		int column, face;
		int64_t x, z;
		PairOf(A, i, &column, &face, &x, &z);
		CountSink sink{ 0u, 0ull };
		cvxb::SurfaceWalk(A.W, A.B, x, z, face, A.solidOutside, A.flags, sink);
		A.stripOffsets[i] = sink.strips;
		if (sink.strips) { atomicAdd(&unitFaces, sink.unitFaces); }
	} else if (i == A.pairs) { // (the scans then leave the totals behind the last pair's offset)
		A.stripOffsets[i] = 0u;
		A.rectOffsets[i] = 0u;
	}
	__syncthreads();
	if (threadIdx.x == 0u && unitFaces) { atomicAdd(&A.totals->unitFaces, unitFaces); }
}

__global__ __launch_bounds__(256) void rects_strips_kernel(RectsArgs A)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.pairs) { return; }
	const uint32_t first = A.stripOffsets[i], end = A.stripOffsets[i + 1];
	if (end == first) { return; }
	int column, face;
	int64_t x, z;
	PairOf(A, i, &column, &face, &x, &z);
	StoreSink sink{ A.strips, first, end };
	cvxb::SurfaceWalk(A.W, A.B, x, z, face, A.solidOutside, A.flags, sink);
}

// kRows false: the first pass of every face.  true: the rows of faces 2, 3 along z.  The pass that is a face's last one counts its rectangles.
template <bool kRows>
__global__ __launch_bounds__(256) void rects_merge_kernel(RectsArgs A)
{
	__shared__ unsigned long long sums[kFaces];
	if (threadIdx.x < (unsigned)kFaces) { sums[threadIdx.x] = 0ull; }
	__syncthreads();
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < A.pairs) {
		const int column = (int)(i / kFaces), face = (int)(i % kFaces);
		if (!kRows || cvxb::RectsHasRowPass(face)) {
			uint32_t firsts = 0u;
			if (A.stripOffsets[i + 1] != A.stripOffsets[i]) {
				const cvxb::RectsPass P{ A.strips, A.stripOffsets, kRows ? A.along : nullptr, (A.flags & CVX_SURFACE_IGNORE_COLOUR) != 0 };
				const cvxb::RectsAxis axis = cvxb::RectsAxisOf(A.B, column, kRows || cvxb::RectsFirstPassAlongZ(face));
				firsts = cvxb::RectsMergePair(P, i, axis, kRows ? A.rows : A.along);
			}
			if (kRows || !cvxb::RectsHasRowPass(face)) {
				A.rectOffsets[i] = firsts;
				if (firsts) { atomicAdd(&sums[face], (unsigned long long)firsts); }
			}
		}
	}
	__syncthreads();
	if (threadIdx.x < (unsigned)kFaces && sums[threadIdx.x]) { atomicAdd(&A.totals->perFace[threadIdx.x], sums[threadIdx.x]); }
}

__global__ __launch_bounds__(256) void rects_write_kernel(RectsArgs A)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.pairs) { return; }
	uint32_t at = A.rectOffsets[i];
	const uint32_t end = A.rectOffsets[i + 1] < A.limit ? A.rectOffsets[i + 1] : A.limit;
	if (at >= end) { return; }
	int column, face;
	int64_t x, z;
	PairOf(A, i, &column, &face, &x, &z);
	const bool rowPass = cvxb::RectsHasRowPass(face);
	const uint32_t stripEnd = A.stripOffsets[i + 1];
	for (uint32_t k = A.stripOffsets[i]; at < end && k < stripEnd; k++) { // (the passes counted the pair's strips with extents above 0)
		const uint32_t along = A.along[k], rows = rowPass ? A.rows[k] : 1u;
		if (along == 0u || rows == 0u) { continue; }
		A.rects[at++] = cvxb::RectOf(A.strips[k], (int32_t)x, (int32_t)z, face, along, rows);
	}
}

// Both calls: `device` says where `rects` lives.
static int Rects(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags, cvx_surface_rect *rects,
                 bool device, int64_t rectCapacity, cvx_surface_rects_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!boxMin || !boxMax) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: a NULL box", call); }
	char bad[cvxb::kBoxMessage];
	if (cvxb::BoxCheck(boxMin, boxMax, 0, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", bad); }
	if (solidOutside & ~0x3F) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown solidOutside bits 0x%x", (unsigned)solidOutside); }
	if (flags & ~CVX_SURFACE_IGNORE_COLOUR) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown flags bits 0x%x", (unsigned)flags); }
	if (rectCapacity < 0 || (rectCapacity > 0 && !rects)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "rectCapacity %lld with %s list", (long long)rectCapacity, rects ? "a" : "no");
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	RectsArgs A{};
	if (!cvxb::PiecesClipBox(boxMin, boxMax, ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ, &A.B)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box lies outside the world");
	}
	if (A.B.Columns() * kFaces >= ((int64_t)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "a box of %lld columns", (long long)A.B.Columns()); }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	const int pairs = (int)(A.B.Columns() * kFaces);
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr, *stripScratch = nullptr;
	cvxi::ScratchLayout carve;
	const size_t chunks = ((size_t)pairs + 1 + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
	const size_t oTotals = carve(sizeof(Totals)), oStripOffsets = carve(((size_t)pairs + 1) * 4), oRectOffsets = carve(((size_t)pairs + 1) * 4);
	const size_t oChunks = carve(chunks * 8), oChunks2 = carve(chunks * 8);
	Totals host{};
	hipError_t e = D.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = hipMemsetAsync(scratch + oTotals, 0, sizeof(Totals), ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.pairs = pairs;
		A.solidOutside = solidOutside;
		A.flags = flags;
		A.totals = reinterpret_cast<Totals *>(scratch + oTotals);
		A.stripOffsets = reinterpret_cast<uint32_t *>(scratch + oStripOffsets);
		A.rectOffsets = reinterpret_cast<uint32_t *>(scratch + oRectOffsets);
		hipLaunchKernelGGL(rects_count_kernel, dim3(Grid((size_t)pairs + 1)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.stripOffsets, pairs + 1, reinterpret_cast<unsigned long long *>(scratch + oChunks), &A.totals->strips);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host.strips, &A.totals->strips, sizeof host.strips, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) { return D.Fail(e); }
	if (host.strips >= ((unsigned long long)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "the box holds %llu strips", host.strips); }
	const size_t strips = (size_t)host.strips;
	if (strips) {
		carve.bytes = 0;
		const size_t oStrips = carve(strips * sizeof(cvxb::RectStrip)), oAlong = carve(strips * 4), oRows = carve(strips * 4);
		e = D.Allocate(&stripScratch, carve.bytes);
		if (e == hipSuccess) {
			A.strips = reinterpret_cast<cvxb::RectStrip *>(stripScratch + oStrips);
			A.along = reinterpret_cast<uint32_t *>(stripScratch + oAlong);
			A.rows = reinterpret_cast<uint32_t *>(stripScratch + oRows);
			hipLaunchKernelGGL(rects_strips_kernel, dim3(Grid((size_t)pairs)), dim3(kThreads), 0, ctx->stream, A);
			hipLaunchKernelGGL(rects_merge_kernel<false>, dim3(Grid((size_t)pairs)), dim3(kThreads), 0, ctx->stream, A);
			hipLaunchKernelGGL(rects_merge_kernel<true>, dim3(Grid((size_t)pairs)), dim3(kThreads), 0, ctx->stream, A);
			cvxi::ExclusiveScan(ctx->stream, A.rectOffsets, pairs + 1, reinterpret_cast<unsigned long long *>(scratch + oChunks2), &A.totals->rects);
			e = hipGetLastError();
		}
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(&host, A.totals, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	const cvxi::ListCall list{ sizeof(cvx_surface_rect), host.rects, rectCapacity, rects, device };
	const int rc = cvxi::FinishList(ctx, D, list, [&](const cvxi::ListJob &J) {
		A.rects = static_cast<cvx_surface_rect *>(J.into);
		A.limit = J.limit;
		hipLaunchKernelGGL(rects_write_kernel, dim3(Grid((size_t)pairs)), dim3(kThreads), 0, ctx->stream, A);
		return hipSuccess;
	});
	if (rc != CVX_OK) { return rc; }
	if (summary) { std::memcpy(summary, &host, sizeof *summary); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxrects

extern "C" {

int cvx_world_surface_rects(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags, cvx_surface_rect *rects,
                            int64_t rectCapacity, cvx_surface_rects_summary *summary, float *outDeviceMs)
{
	return cvxrects::Rects(ctx, "cvx_world_surface_rects", boxMin, boxMax, solidOutside, flags, rects, false, rectCapacity, summary, outDeviceMs);
}

int cvx_world_surface_rects_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags, cvx_surface_rect *rectsDevice,
                                   int64_t rectCapacity, cvx_surface_rects_summary *summary, float *outDeviceMs)
{
	return cvxrects::Rects(ctx, "cvx_world_surface_rects_device", boxMin, boxMax, solidOutside, flags, rectsDevice, true, rectCapacity, summary, outDeviceMs);
}

int cvx_surface_rect_triangles(const cvx_surface_rect *rects, int64_t rectCount, cvx_mesh_vertex *vertices, int32_t *indices)
{
	if (rectCount < 0 || rectCount >= ((int64_t)1 << 29)) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_rect_triangles: rectCount %lld", (long long)rectCount); }
	if (rectCount > 0 && (!rects || !vertices || !indices)) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_rect_triangles: a NULL pointer"); }
	for (int64_t k = 0; k < rectCount; k++) {
		const cvx_surface_rect &r = rects[k];
		if (r.face < 0 || r.face > 5) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_rect_triangles: rectangle %lld has face %d", (long long)k, r.face); }
		if (r.size[0] < 1 || r.size[1] < 1 || r.size[2] < 1 || r.size[r.face >> 1] != 1) {
			return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_rect_triangles: rectangle %lld of face %d has size %d x %d x %d", (long long)k, r.face, r.size[0],
			            r.size[1], r.size[2]);
		}
	}
	static const int32_t order[6] = { 0, 1, 2, 0, 2, 3 };
	for (int64_t k = 0; k < rectCount; k++) {
		float corners[4][3];
		cvxb::RectCorners(rects[k], corners);
		for (int c = 0; c < 4; c++) {
			cvx_mesh_vertex &v = vertices[4 * k + c];
			for (int a = 0; a < 3; a++) { v.position[a] = corners[c][a]; }
			cvxb::SurfaceVertexRgba(rects[k].argb, v.rgba);
			v.uv[0] = v.uv[1] = 0.f;
			v.material = -1;
		}
		for (int t = 0; t < 6; t++) { indices[6 * k + t] = (int32_t)(4 * k) + order[t]; }
	}
	return CVX_OK;
}

} // extern "C"
