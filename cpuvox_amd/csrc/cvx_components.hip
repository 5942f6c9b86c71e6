// cvx_components.hip -- libcpuvox_gpu.so, the component-labelling engine of cvx_world_pieces, cvx_world_settle and cvx_world_cavities: the
// kernels that depend on no rule and the host driver.  See cvx_components.h for the steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cvx_components.h"

using cvxi::Fail;
using cvxi::Grid;
using cvxi::kThreads;

namespace cvxcomp {

__global__ __launch_bounds__(256) void flatten_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	const uint32_t r = Find(A.parent, i);
	if (r != i) { atomicMin(A.parent + i, r); }
}

__global__ __launch_bounds__(256) void list_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes || !(A.parent[i] == i && (A.bits[i] & kSelected)) || A.rank[i] >= (uint32_t)A.capacity) { return; }
	const int32_t *b = A.bounds + 6 * (size_t)i;
	const uint32_t c = A.column[i];
	cvx_piece p;
	for (int a = 0; a < 3; a++) {
		p.min[a] = b[a];
		p.max[a] = b[3 + a];
	}
	p.seed[0] = A.B.x0 + (int)(c / (uint32_t)A.B.SizeZ());
	p.seed[1] = (int32_t)A.lohi[2 * (size_t)i + 1] - 1;
	p.seed[2] = A.B.z0 + (int)(c % (uint32_t)A.B.SizeZ());
	p.pad_ = 0;
	p.voxels = (int64_t)A.voxels[i];
	A.list[A.rank[i]] = p;
}

__global__ __launch_bounds__(256) void mark_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	A.rank[i] = (A.bits[A.parent[i]] & kSelected) ? 1u : 0u;
}

void MarkSelected(hipStream_t stream, const NodeArgs &A) { hipLaunchKernelGGL(mark_kernel, dim3(Grid(A.nodes)), dim3(kThreads), 0, stream, A); }

constexpr size_t kHead = 256; // components that come to the host with the totals, in one copy

int Analyse(cvx_context *ctx, const Call &call, const int32_t boxMin[3], const int32_t boxMax[3], SelectLauncher select, void *hostTotals, Analysis *R)
{
	NodeArgs &A = R->A;
	A = NodeArgs{};
	if (!cvxb::PiecesClipBox(boxMin, boxMax, ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ, &A.B)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box lies outside the world");
	}
	if (A.B.Columns() >= ((int64_t)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "a box of %lld columns", (long long)A.B.Columns()); }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	const int n = (int)A.B.Columns();
	const RuleKernels &K = call.kernels;
	const size_t totalsBytes = call.totalsBytes;
	TotalsHead &host = *static_cast<TotalsHead *>(hostTotals);
	cvxi::DeviceCall &D = R->device;
	uint8_t *columnScratch = nullptr, *nodeScratch = nullptr;
	auto chunksOf = [](size_t count) { return (count + cvxi::ScanChunk() - 1) / cvxi::ScanChunk(); };

	// 1. the nodes of every column, their offsets, the total
	cvxi::ScratchLayout columns;
	const size_t oTotals = columns(totalsBytes), oOffsets = columns(((size_t)n + 1) * 4), oChunks = columns(chunksOf((size_t)n + 1) * 8);
	hipError_t e = D.Allocate(&columnScratch, columns.bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = hipMemcpyAsync(columnScratch + oTotals, hostTotals, totalsBytes, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.n = n;
		A.faceMask = call.faceMask;
		A.totals = reinterpret_cast<TotalsHead *>(columnScratch + oTotals);
		A.offsets = reinterpret_cast<uint32_t *>(columnScratch + oOffsets);
		hipLaunchKernelGGL(K.count, dim3(Grid((size_t)n + 1)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.offsets, n + 1, reinterpret_cast<unsigned long long *>(columnScratch + oChunks), &A.totals->nodes);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host.nodes, &A.totals->nodes, sizeof host.nodes, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) { return D.Fail(e); }
	if (host.nodes >= ((unsigned long long)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "the box holds %llu %s", host.nodes, call.nodeNoun); }
	const size_t nodes = (size_t)host.nodes;
	R->nodes = nodes;
	A.nodes = (uint32_t)nodes;
	A.capacity = call.capacity;
	const size_t listed = std::min<size_t>((size_t)call.capacity, nodes);

	// 2 .. 5. the node table, the components, the totals, the list
	cvxi::ScratchLayout table;
	const size_t oHead = table(totalsBytes), oList = table(listed * sizeof(cvx_piece)), oLohi = table(nodes * 8), oColumn = table(nodes * 4), oParent = table(nodes * 4),
	             oVoxels = table(nodes * 8), oBounds = table(nodes * 24), oBits = table(nodes * 4), oRank = table(nodes * 4), oRankChunks = table(chunksOf(nodes) * 8);
	std::vector<uint8_t> back(totalsBytes + std::min(listed, kHead) * sizeof(cvx_piece));
	if (nodes) {
		e = D.Allocate(&nodeScratch, table.bytes);
		if (e != hipSuccess) { return D.Fail(e); }
		A.list = reinterpret_cast<cvx_piece *>(nodeScratch + oList);
		A.lohi = reinterpret_cast<uint32_t *>(nodeScratch + oLohi);
		A.column = reinterpret_cast<uint32_t *>(nodeScratch + oColumn);
		A.parent = reinterpret_cast<uint32_t *>(nodeScratch + oParent);
		A.voxels = reinterpret_cast<unsigned long long *>(nodeScratch + oVoxels);
		A.bounds = reinterpret_cast<int32_t *>(nodeScratch + oBounds);
		A.bits = reinterpret_cast<uint32_t *>(nodeScratch + oBits);
		A.rank = reinterpret_cast<uint32_t *>(nodeScratch + oRank);
		const dim3 grid(Grid(nodes)), block(kThreads);
		hipLaunchKernelGGL(K.nodes, dim3(Grid((size_t)n)), block, 0, ctx->stream, A);
		for (;;) { // until a pass hooks nothing
			e = hipMemsetAsync(&A.totals->changed, 0, sizeof(unsigned int), ctx->stream);
			if (e != hipSuccess) { break; }
			hipLaunchKernelGGL(K.hook, grid, block, 0, ctx->stream, A);
			hipLaunchKernelGGL(flatten_kernel, grid, block, 0, ctx->stream, A);
			R->rounds++;
			e = hipGetLastError();
			if (e == hipSuccess) { e = hipMemcpyAsync(&host.changed, &A.totals->changed, sizeof host.changed, hipMemcpyDeviceToHost, ctx->stream); }
			if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
			if (e != hipSuccess || !host.changed) { break; }
		}
		if (e == hipSuccess) {
			hipLaunchKernelGGL(K.stats, grid, block, 0, ctx->stream, A);
			e = select(A);
			cvxi::ExclusiveScan(ctx->stream, A.rank, (int)nodes, reinterpret_cast<unsigned long long *>(nodeScratch + oRankChunks), &A.totals->listed);
			if (listed) { hipLaunchKernelGGL(list_kernel, grid, block, 0, ctx->stream, A); }
			if (e == hipSuccess) { e = hipGetLastError(); }
			// the totals go in front of the list, so that ONE copy brings them and the list's head
			if (e == hipSuccess) { e = hipMemcpyAsync(nodeScratch + oHead, A.totals, totalsBytes, hipMemcpyDeviceToDevice, ctx->stream); }
			if (e == hipSuccess) { e = hipMemcpyAsync(back.data(), nodeScratch + oHead, back.size(), hipMemcpyDeviceToHost, ctx->stream); }
		}
	}
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (nodes) { std::memcpy(hostTotals, back.data(), totalsBytes); }
	const size_t wanted = std::min<size_t>((size_t)host.listed, (size_t)call.capacity);
	R->list.assign(wanted, cvx_piece{});
	if (wanted) {
		const size_t head = std::min(wanted, kHead);
		std::memcpy(R->list.data(), back.data() + totalsBytes, head * sizeof(cvx_piece));
		if (wanted > head) {
			e = hipMemcpy(R->list.data() + head, A.list + head, (wanted - head) * sizeof(cvx_piece), hipMemcpyDeviceToHost);
			if (e != hipSuccess) { return D.Fail(e); }
		}
	}
	R->ms = D.Ms();
	return CVX_OK;
}

} // namespace cvxcomp
