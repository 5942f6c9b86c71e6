// cvx_surface.hip -- libcpuvox_gpu.so, the exposed faces of the device-resident world as coloured quads (cvx_world_surface,
// cvx_world_surface_device, cvx_surface_triangles).  See include/cpuvox_gpu.h for the contract and cvx_surface.h for the rule.
//
// Count, scan, write over the (column, face) pairs of the clipped box, pair = column * 6 + face in the box's (x, then z) column order:
//   1. count  (a thread per pair): cvxb::SurfaceWalk with a counting sink -> the pair's quads; the unit faces and the quads per face are summed
//             per workgroup in LDS and sent on with one atomic each (integer sums: no schedule shows in them)
//   2. scan   cvxi::ExclusiveScan gives every pair its first quad; ONE copy brings the totals to the host
//   3. write  (a thread per pair that has quads below the capacity): the same walk with a storing sink.  The order of the contract is the pair
//             order with the walk's top-down order inside a pair: nothing is sorted.
// A column's cost is spread over six lanes, and a side pair reads two records (its own and one neighbour's), not five.  Nothing is written to
// the arena.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "cvx_context.h"
#include "cvx_surface.h"

using cvxi::Fail;

namespace cvxsurface {

using cvxi::Grid;
using cvxi::kThreads;

constexpr int kFaces = 6;

struct Totals {
	unsigned long long quads;        // the scan's total
	unsigned long long unitFaces;
	unsigned long long perFace[kFaces];
};
static_assert(sizeof(Totals) == sizeof(cvx_surface_summary), "the totals are the summary");

struct SurfaceArgs {
	cvxb::CopyWorld W;
	cvxb::PiecesBox B;
	int pairs;                 // columns of the box * 6
	int solidOutside, flags;
	uint32_t *offsets;         // pairs + 1: count, then the first quad of every pair
	Totals *totals;
	cvx_surface_quad *quads;
	uint32_t limit;            // quads are written below this index
};

struct CountSink {
	uint32_t quads;
	unsigned long long unitFaces;
	CVX_HD void operator()(const cvx_surface_quad &q)
	{
		quads++;
		unitFaces += (unsigned long long)q.length;
	}
};

struct StoreSink {
	cvx_surface_quad *quads;
	uint32_t at, limit;
	CVX_HD void operator()(const cvx_surface_quad &q)
	{
		if (at < limit) { quads[at] = q; }
		at++;
	}
};

__global__ __launch_bounds__(256) void surface_count_kernel(SurfaceArgs A)
{
	__shared__ unsigned long long sums[kFaces + 1];
	if (threadIdx.x <= (unsigned)kFaces) { sums[threadIdx.x] = 0ull; }
	__syncthreads();
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < A.pairs) {
		const int column = (int)(i / kFaces), face = (int)(i % kFaces);
		const int64_t x = A.B.x0 + column / A.B.SizeZ(), z = A.B.z0 + column % A.B.SizeZ();
		CountSink sink{ 0u, 0ull };
		cvxb::SurfaceWalk(A.W, A.B, x, z, face, A.solidOutside, A.flags, sink);
		A.offsets[i] = sink.quads;
		if (sink.quads) {
			atomicAdd(&sums[face], (unsigned long long)sink.quads);
			atomicAdd(&sums[kFaces], sink.unitFaces);
		}
	} else if (i == A.pairs) { // (the scan then leaves the quad total behind the last pair's offset)
		A.offsets[i] = 0u;
	}
	__syncthreads();
	if (threadIdx.x <= (unsigned)kFaces && sums[threadIdx.x]) {
		atomicAdd(threadIdx.x == (unsigned)kFaces ? &A.totals->unitFaces : &A.totals->perFace[threadIdx.x], sums[threadIdx.x]);
	}
}

__global__ __launch_bounds__(256) void surface_write_kernel(SurfaceArgs A)
{
	const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.pairs) { return; }
	const uint32_t first = A.offsets[i];
	if (first >= A.limit || A.offsets[i + 1] == first) { return; }
	const int column = (int)(i / kFaces), face = (int)(i % kFaces);
	const int64_t x = A.B.x0 + column / A.B.SizeZ(), z = A.B.z0 + column % A.B.SizeZ();
	StoreSink sink{ A.quads, first, A.limit };
	cvxb::SurfaceWalk(A.W, A.B, x, z, face, A.solidOutside, A.flags, sink);
}

// Both calls: `device` says where `quads` lives.
static int Surface(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags, cvx_surface_quad *quads,
                   bool device, int64_t quadCapacity, cvx_surface_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!boxMin || !boxMax) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: a NULL box", call); }
	char bad[cvxb::kBoxMessage];
	if (cvxb::BoxCheck(boxMin, boxMax, 0, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", bad); }
	if (solidOutside & ~0x3F) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown solidOutside bits 0x%x", (unsigned)solidOutside); }
	if (flags & ~CVX_SURFACE_IGNORE_COLOUR) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown flags bits 0x%x", (unsigned)flags); }
	if (quadCapacity < 0 || (quadCapacity > 0 && !quads)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "quadCapacity %lld with %s list", (long long)quadCapacity, quads ? "a" : "no");
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int dim[3] = { ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ };
	SurfaceArgs A{};
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dim[0], dim[1], dim[2], &A.B)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box lies outside the world"); }
	if (A.B.Columns() * kFaces >= ((int64_t)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "a box of %lld columns", (long long)A.B.Columns()); }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	const int pairs = (int)(A.B.Columns() * kFaces);
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	cvxi::ScratchLayout carve;
	const size_t chunks = ((size_t)pairs + 1 + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
	const size_t oTotals = carve(sizeof(Totals)), oOffsets = carve(((size_t)pairs + 1) * 4), oChunks = carve(chunks * 8);
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
		A.offsets = reinterpret_cast<uint32_t *>(scratch + oOffsets);
		hipLaunchKernelGGL(surface_count_kernel, dim3(Grid((size_t)pairs + 1)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.offsets, pairs + 1, reinterpret_cast<unsigned long long *>(scratch + oChunks), &A.totals->quads);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host, A.totals, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) { return D.Fail(e); }
	if (host.quads >= ((unsigned long long)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "the box holds %llu quads", host.quads); }
	const cvxi::ListCall list{ sizeof(cvx_surface_quad), host.quads, quadCapacity, quads, device };
	const int rc = cvxi::FinishList(ctx, D, list, [&](const cvxi::ListJob &J) {
		A.quads = static_cast<cvx_surface_quad *>(J.into);
		A.limit = J.limit;
		hipLaunchKernelGGL(surface_write_kernel, dim3(Grid((size_t)pairs)), dim3(kThreads), 0, ctx->stream, A);
		return hipSuccess;
	});
	if (rc != CVX_OK) { return rc; }
	if (summary) { std::memcpy(summary, &host, sizeof *summary); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace cvxsurface

extern "C" {

int cvx_world_surface(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags, cvx_surface_quad *quads,
                      int64_t quadCapacity, cvx_surface_summary *summary, float *outDeviceMs)
{
	return cvxsurface::Surface(ctx, "cvx_world_surface", boxMin, boxMax, solidOutside, flags, quads, false, quadCapacity, summary, outDeviceMs);
}

int cvx_world_surface_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags, cvx_surface_quad *quadsDevice,
                             int64_t quadCapacity, cvx_surface_summary *summary, float *outDeviceMs)
{
	return cvxsurface::Surface(ctx, "cvx_world_surface_device", boxMin, boxMax, solidOutside, flags, quadsDevice, true, quadCapacity, summary, outDeviceMs);
}

int cvx_surface_triangles(const cvx_surface_quad *quads, int64_t quadCount, cvx_mesh_vertex *vertices, int32_t *indices)
{
	if (quadCount < 0 || quadCount >= ((int64_t)1 << 29)) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_triangles: quadCount %lld", (long long)quadCount); }
	if (quadCount > 0 && (!quads || !vertices || !indices)) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_triangles: a NULL pointer"); }
	for (int64_t k = 0; k < quadCount; k++) {
		if (quads[k].face < 0 || quads[k].face > 5) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_surface_triangles: quad %lld has face %d", (long long)k, quads[k].face); }
	}
	static const int32_t order[6] = { 0, 1, 2, 0, 2, 3 };
	for (int64_t k = 0; k < quadCount; k++) {
		float corners[4][3];
		cvxb::SurfaceCorners(quads[k], corners);
		for (int c = 0; c < 4; c++) {
			cvx_mesh_vertex &v = vertices[4 * k + c];
			for (int a = 0; a < 3; a++) { v.position[a] = corners[c][a]; }
			cvxb::SurfaceVertexRgba(quads[k].argb, v.rgba);
			v.uv[0] = v.uv[1] = 0.f;
			v.material = -1;
		}
		for (int t = 0; t < 6; t++) { indices[6 * k + t] = (int32_t)(4 * k) + order[t]; }
	}
	return CVX_OK;
}

} // extern "C"
