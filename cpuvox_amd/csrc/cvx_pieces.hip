// cvx_pieces.hip -- libcpuvox_gpu.so, the floating pieces of the device-resident world (cvx_world_pieces).  See include/cpuvox_gpu.h for the
// contract and cvx_pieces.h for the rules.
//
// Connected components over the solid RUNS of LOD 0 inside the box, not over its voxels: a node is one solid run of one column clipped to the
// box's y range, an edge joins nodes of face-neighbouring columns whose y intervals overlap (and the two halves of a split run).
//   1. count  (a thread per column of the box): its nodes; cvxi::ExclusiveScan gives the node offsets; ONE copy brings the total to the host
//   2. nodes  (a thread per column): interval, column and label (= its own index) of every node, in column order and top-down inside a column,
//             so that the smallest node index of a piece is its seed
//   3. hook   (a thread per node): the node's interval against the sorted node lists of the +X and +Z neighbour columns and the node below it;
//             every edge is a lock-free union, the root with the larger index hooked under the smaller one with atomicMin, retried until both
//             ends have one root; then a flatten pass points every node at its root.  The two are repeated until a hook pass changes no label
//             (the first pass does all the work, the second confirms it: no round limit decides the result)
//   4. stats  (a thread per node, reduced per wave where a wave has one root): voxels, bounding box and anchor bits of every root; the largest
//             piece by two reductions; floating roots flagged, totalled and ranked by a scan in index order = the order of the contract
//   5. list   the first pieceCapacity floating pieces, copied to the host behind the totals
//   6. REMOVE cvxi::ColumnEdit (cvx_edit.hip) over the floating pieces' rectangle: count and write of the sub-world blob are
//             cvxb::PiecesRemoveColumn.  Nothing in the arena is written before its last step.
// Steps 1 .. 5 are cvxpieces::Analyse (cvx_pieces_nodes.h), which leaves the node tables on the device: cvx_world_settle (cvx_settle.hip) goes on from them too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_pieces.h"
#include "cvx_pieces_nodes.h"

using cvxi::Fail;

namespace cvxpieces {

__global__ __launch_bounds__(256) void pieces_count_kernel(PiecesArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > A.n) { return; }
	if (i == A.n) { // (the scan then leaves the node total behind the last column's offset)
		A.offsets[i] = 0u;
		return;
	}
	const int64_t x = A.B.x0 + i / A.B.SizeZ(), z = A.B.z0 + i % A.B.SizeZ();
	A.offsets[i] = cvxb::PiecesRunCount(cvxb::CopyColumnAt(A.W, x, z), A.B.y0, A.B.y1);
}

__global__ __launch_bounds__(256) void pieces_nodes_kernel(PiecesArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t first = A.offsets[i], count = A.offsets[i + 1] - first;
	if (count == 0u) { return; }
	const int64_t x = A.B.x0 + i / A.B.SizeZ(), z = A.B.z0 + i % A.B.SizeZ();
	cvxb::PiecesClippedRuns(cvxb::CopyColumnAt(A.W, x, z), A.B.y0, A.B.y1, A.lohi + 2 * (size_t)first);
	for (uint32_t j = first; j < first + count; j++) {
		A.column[j] = (uint32_t)i;
		A.parent[j] = j;
		A.voxels[j] = 0ull;
		A.bits[j] = 0u;
		int32_t *b = A.bounds + 6 * (size_t)j;
		b[0] = b[1] = b[2] = INT_MAX;
		b[3] = b[4] = b[5] = INT_MIN;
	}
}

// node i against the nodes of column c2 (sorted top-down: lo and hi fall with the index)
__device__ inline bool HookColumn(const PiecesArgs &A, uint32_t i, uint32_t lo, uint32_t hi, uint32_t c2)
{
	uint32_t s = A.offsets[c2];
	const uint32_t e = A.offsets[c2 + 1];
	uint32_t a = s, b = e; // the first node whose lo is below hi
	while (a < b) {
		const uint32_t mid = (a + b) >> 1;
		if (A.lohi[2 * (size_t)mid] >= hi) { a = mid + 1u; } else { b = mid; }
	}
	bool changed = false;
	for (s = a; s < e && cvxb::PiecesTouch(lo, hi, A.lohi[2 * (size_t)s], A.lohi[2 * (size_t)s + 1]); s++) { changed = Unite(A.parent, i, s) || changed; }
	return changed;
}

__global__ __launch_bounds__(256) void pieces_hook_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	const uint32_t lo = A.lohi[2 * (size_t)i], hi = A.lohi[2 * (size_t)i + 1], c = A.column[i];
	const int sizeZ = A.B.SizeZ();
	bool changed = false;
	if (i + 1u < A.offsets[c + 1] && cvxb::PiecesStacked(lo, A.lohi[2 * (size_t)(i + 1u) + 1])) { changed = Unite(A.parent, i, i + 1u); }
	if ((int)(c / (uint32_t)sizeZ) + 1 < A.B.SizeX()) { changed = HookColumn(A, i, lo, hi, c + (uint32_t)sizeZ) || changed; }
	if ((int)(c % (uint32_t)sizeZ) + 1 < sizeZ) { changed = HookColumn(A, i, lo, hi, c + 1u) || changed; }
	if (changed) { atomicOr(&A.totals->changed, 1u); }
}

__global__ __launch_bounds__(256) void pieces_flatten_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	const uint32_t r = Find(A.parent, i);
	if (r != i) { atomicMin(A.parent + i, r); }
}

// Totals of the roots.  Neighbouring nodes mostly belong to one piece: a wave whose nodes have one root reduces first and sends one set of atomics.
__global__ __launch_bounds__(256) void pieces_stats_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = i < A.nodes;
	uint32_t root = 0xFFFFFFFFu;
	unsigned long long voxels = 0ull;
	int mn[3] = { INT_MAX, INT_MAX, INT_MAX }, mx[3] = { INT_MIN, INT_MIN, INT_MIN };
	uint32_t bits = 0u;
	if (live) {
		root = A.parent[i];
		const uint32_t lo = A.lohi[2 * (size_t)i], hi = A.lohi[2 * (size_t)i + 1], c = A.column[i];
		const int x = A.B.x0 + (int)(c / (uint32_t)A.B.SizeZ()), z = A.B.z0 + (int)(c % (uint32_t)A.B.SizeZ());
		voxels = hi - lo;
		mn[0] = x; mn[1] = (int)lo; mn[2] = z;
		mx[0] = x + 1; mx[1] = (int)hi; mx[2] = z + 1;
		bits = (uint32_t)(cvxb::PiecesNodeAnchors(A.W, A.B, x, z, lo, hi) & A.anchors);
	}
	const uint32_t first = __shfl(root, 0, 64); // (lane 0 is live in every wave that has a live lane)
	if (__all(!live || root == first)) {
		voxels = WaveReduce(voxels, [](unsigned long long a, unsigned long long b) { return a + b; });
		bits = WaveReduce(bits, [](uint32_t a, uint32_t b) { return a | b; });
		for (int a = 0; a < 3; a++) {
			mn[a] = WaveReduce(mn[a], [](int p, int q) { return p < q ? p : q; });
			mx[a] = WaveReduce(mx[a], [](int p, int q) { return p > q ? p : q; });
		}
		if ((threadIdx.x & 63u) != 0u) { return; }
	}
	if (!live) { return; }
	atomicAdd(A.voxels + root, voxels);
	if (bits) { atomicOr(A.bits + root, bits); }
	int32_t *b = A.bounds + 6 * (size_t)root;
	for (int a = 0; a < 3; a++) {
		atomicMin(b + a, mn[a]);
		atomicMax(b + 3 + a, mx[a]);
	}
}

// CVX_ANCHOR_LARGEST: the most voxels, then the smallest root among the pieces that have them
__global__ __launch_bounds__(256) void pieces_most_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long v = i < A.nodes && A.parent[i] == i ? A.voxels[i] : 0ull;
	v = WaveReduce(v, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; });
	if ((threadIdx.x & 63u) == 0u && v) { atomicMax(&A.totals->mostVoxels, v); }
}

__global__ __launch_bounds__(256) void pieces_largest_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t r = i < A.nodes && A.parent[i] == i && A.voxels[i] == A.totals->mostVoxels ? i : 0xFFFFFFFFu;
	r = WaveReduce(r, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
	if ((threadIdx.x & 63u) == 0u && r != 0xFFFFFFFFu) { atomicMin(&A.totals->largest, r); }
}

// roots: anchored or floating; rank = 1 for a floating root (-> its place in the list after the scan); the four totals and the floating pieces' XZ box
__global__ __launch_bounds__(256) void pieces_flag_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool root = i < A.nodes && A.parent[i] == i;
	bool floats = false;
	unsigned long long voxels = 0ull;
	int x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	if (root) {
		const bool anchored = A.bits[i] != 0u || ((A.anchors & CVX_ANCHOR_LARGEST) && A.totals->largest == i);
		floats = !anchored;
		voxels = A.voxels[i];
		if (floats) {
			const int32_t *b = A.bounds + 6 * (size_t)i;
			A.bits[i] |= kFloats;
			x0 = b[0]; z0 = b[2]; x1 = b[3]; z1 = b[5];
		}
	}
	if (i < A.nodes) { A.rank[i] = floats ? 1u : 0u; }
	auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
	const unsigned long long fp = WaveReduce<unsigned long long>(floats ? 1ull : 0ull, add), fv = WaveReduce<unsigned long long>(floats ? voxels : 0ull, add);
	const unsigned long long ap = WaveReduce<unsigned long long>(root && !floats ? 1ull : 0ull, add), av = WaveReduce<unsigned long long>(root && !floats ? voxels : 0ull, add);
	x0 = WaveReduce(x0, [](int p, int q) { return p < q ? p : q; });
	z0 = WaveReduce(z0, [](int p, int q) { return p < q ? p : q; });
	x1 = WaveReduce(x1, [](int p, int q) { return p > q ? p : q; });
	z1 = WaveReduce(z1, [](int p, int q) { return p > q ? p : q; });
	if ((threadIdx.x & 63u) != 0u) { return; }
	Totals *T = A.totals;
	if (fp) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.floatingPieces), fp);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.floatingVoxels), fv);
		atomicMin(&T->x0, x0);
		atomicMin(&T->z0, z0);
		atomicMax(&T->x1, x1);
		atomicMax(&T->z1, z1);
	}
	if (ap) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.anchoredPieces), ap);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.anchoredVoxels), av);
	}
}

__global__ __launch_bounds__(256) void pieces_list_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes || !(A.parent[i] == i && (A.bits[i] & kFloats)) || A.rank[i] >= (uint32_t)A.capacity) { return; }
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

// REMOVE: rank[i] = node i belongs to a floating piece
__global__ __launch_bounds__(256) void pieces_mark_kernel(PiecesArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	A.rank[i] = (A.bits[A.parent[i]] & kFloats) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void pieces_remove_count_kernel(PiecesArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.rn) { return; }
	const int cx = A.rx0 + i / A.rSizeZ, cz = A.rz0 + i % A.rSizeZ;
	uint32_t nodes;
	const uint32_t *floating = ColumnNodes(A, A.rank, cx, cz, &nodes);
	const cvxb::BrushResult r = cvxb::PiecesRemoveColumn(A.W, cx, cz, A.B.y0, A.B.y1, floating, nodes, nullptr, nullptr);
	if (r.overLimit) { atomicOr(&A.totals->overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void pieces_remove_write_kernel(PiecesArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.rn) { return; }
	const int cx = A.rx0 + i / A.rSizeZ, cz = A.rz0 + i % A.rSizeZ;
	uint32_t nodes;
	const uint32_t *floating = ColumnNodes(A, A.rank, cx, cz, &nodes);
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	const cvxb::BrushResult r = cvxb::PiecesRemoveColumn(A.W, cx, cz, A.B.y0, A.B.y1, floating, nodes, nullptr, nullptr);
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::PiecesRemoveColumn(A.W, cx, cz, A.B.y0, A.B.y1, floating, nodes, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

constexpr size_t kHead = 256; // pieces that come to the host with the totals, in one copy

int FailHip(cvx_context *ctx, const char *call, hipError_t e)
{
	if (e == hipErrorOutOfMemory) {
		(void)hipGetLastError();
		return Fail(ctx, CVX_ERR_CAPACITY, "the scratch of %s does not fit in device memory", call);
	}
	return Fail(ctx, CVX_ERR_HIP, "%s failed: %s", call, hipGetErrorString(e));
}

void Analysis::Release()
{
	for (uint8_t *p : { columnScratch, nodeScratch }) { if (p) { (void)hipFree(p); } }
	for (hipEvent_t e : ev) { if (e) { (void)hipEventDestroy(e); } }
	columnScratch = nodeScratch = nullptr;
	ev[0] = ev[1] = nullptr;
}

int Analyse(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, const char *extraError, int levelCount,
            const cvx_piece *pieces, int pieceCapacity, Analysis *R)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!boxMin || !boxMax) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box is NULL"); }
	for (int a = 0; a < 3; a++) {
		if (boxMin[a] >= boxMax[a]) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box [%d, %d) on axis %d is empty", boxMin[a], boxMax[a], a); }
	}
	if (anchors & ~(CVX_ANCHOR_GROUND | CVX_ANCHOR_OUTSIDE | CVX_ANCHOR_LARGEST)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown anchors bits 0x%x", (unsigned)anchors); }
	if (extraError) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", extraError); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (pieceCapacity < 0 || (pieceCapacity > 0 && !pieces)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "pieceCapacity %d with %s list", pieceCapacity, pieces ? "a" : "no"); }
	if (!ctx->levelSet[0]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD 0 has not been uploaded"); }
	int *dim = R->dim;
	dim[0] = ctx->hostWorld.dimX;
	dim[1] = ctx->hostWorld.dimY;
	dim[2] = ctx->hostWorld.dimZ;
	PiecesArgs &A = R->A;
	A = PiecesArgs{};
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dim[0], dim[1], dim[2], &A.B)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box lies outside the world"); }
	if (A.B.Columns() >= ((int64_t)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "a box of %lld columns", (long long)A.B.Columns()); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	int rc = cvxi::SyncWorld(ctx);
	if (rc != CVX_OK) { return rc; }

	const int n = (int)A.B.Columns();
	hipEvent_t *ev = R->ev;
	auto release = [&]() { R->Release(); };
	size_t bytes = 0;
	auto carve = [&](size_t b) { const size_t at = bytes; bytes = (bytes + b + 15) & ~(size_t)15; return at; };
	auto chunksOf = [](size_t count) { return (count + cvxi::ScanChunk() - 1) / cvxi::ScanChunk(); };

	// 1. the nodes of every column, their offsets, the total
	const size_t oTotals = carve(sizeof(Totals)), oOffsets = carve(((size_t)n + 1) * 4), oChunks = carve(chunksOf((size_t)n + 1) * 8);
	Totals &host = R->host;
	host = Totals{};
	host.largest = 0xFFFFFFFFu;
	host.x0 = host.z0 = INT_MAX;
	host.x1 = host.z1 = INT_MIN;
	uint8_t *&columnScratch = R->columnScratch, *&nodeScratch = R->nodeScratch;
	hipError_t e = hipEventCreate(&ev[0]);
	if (e == hipSuccess) { e = hipEventCreate(&ev[1]); }
	if (e == hipSuccess) { e = hipMalloc((void **)&columnScratch, bytes); }
	if (e == hipSuccess) { e = hipEventRecord(ev[0], ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(columnScratch + oTotals, &host, sizeof host, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.n = n;
		A.anchors = anchors;
		A.totals = reinterpret_cast<Totals *>(columnScratch + oTotals);
		A.offsets = reinterpret_cast<uint32_t *>(columnScratch + oOffsets);
		hipLaunchKernelGGL(pieces_count_kernel, dim3(Grid((size_t)n + 1)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.offsets, n + 1, reinterpret_cast<unsigned long long *>(columnScratch + oChunks), &A.totals->nodes);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host.nodes, &A.totals->nodes, sizeof host.nodes, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) {
		release();
		return FailHip(ctx, call, e);
	}
	if (host.nodes >= ((unsigned long long)1 << 31) - 1) {
		release();
		return Fail(ctx, CVX_ERR_CAPACITY, "the box holds %llu solid runs", host.nodes);
	}
	const size_t nodes = (size_t)host.nodes;
	R->nodes = nodes;
	A.nodes = (uint32_t)nodes;
	A.capacity = pieceCapacity;
	const size_t listed = std::min<size_t>((size_t)pieceCapacity, nodes);

	// 2 .. 5. the node table, the components, the totals, the list
	bytes = 0;
	const size_t oHead = carve(sizeof(Totals)), oList = carve(listed * sizeof(cvx_piece)), oLohi = carve(nodes * 8), oColumn = carve(nodes * 4), oParent = carve(nodes * 4),
	             oVoxels = carve(nodes * 8), oBounds = carve(nodes * 24), oBits = carve(nodes * 4), oRank = carve(nodes * 4), oRankChunks = carve(chunksOf(nodes) * 8);
	static_assert(sizeof(Totals) % 16 == 0, "the list follows the totals");
	std::vector<uint8_t> back(sizeof(Totals) + std::min(listed, kHead) * sizeof(cvx_piece));
	if (nodes) {
		e = hipMalloc((void **)&nodeScratch, bytes);
		if (e != hipSuccess) {
			release();
			return FailHip(ctx, call, e);
		}
		A.list = reinterpret_cast<cvx_piece *>(nodeScratch + oList);
		A.lohi = reinterpret_cast<uint32_t *>(nodeScratch + oLohi);
		A.column = reinterpret_cast<uint32_t *>(nodeScratch + oColumn);
		A.parent = reinterpret_cast<uint32_t *>(nodeScratch + oParent);
		A.voxels = reinterpret_cast<unsigned long long *>(nodeScratch + oVoxels);
		A.bounds = reinterpret_cast<int32_t *>(nodeScratch + oBounds);
		A.bits = reinterpret_cast<uint32_t *>(nodeScratch + oBits);
		A.rank = reinterpret_cast<uint32_t *>(nodeScratch + oRank);
		const dim3 grid(Grid(nodes)), block(kThreads);
		hipLaunchKernelGGL(pieces_nodes_kernel, dim3(Grid((size_t)n)), block, 0, ctx->stream, A);
		for (;;) { // until a pass hooks nothing
			e = hipMemsetAsync(&A.totals->changed, 0, sizeof(unsigned int), ctx->stream);
			if (e != hipSuccess) { break; }
			hipLaunchKernelGGL(pieces_hook_kernel, grid, block, 0, ctx->stream, A);
			hipLaunchKernelGGL(pieces_flatten_kernel, grid, block, 0, ctx->stream, A);
			e = hipGetLastError();
			if (e == hipSuccess) { e = hipMemcpyAsync(&host.changed, &A.totals->changed, sizeof host.changed, hipMemcpyDeviceToHost, ctx->stream); }
			if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
			if (e != hipSuccess || !host.changed) { break; }
		}
		if (e == hipSuccess) {
			hipLaunchKernelGGL(pieces_stats_kernel, grid, block, 0, ctx->stream, A);
			if (anchors & CVX_ANCHOR_LARGEST) {
				hipLaunchKernelGGL(pieces_most_kernel, grid, block, 0, ctx->stream, A);
				hipLaunchKernelGGL(pieces_largest_kernel, grid, block, 0, ctx->stream, A);
			}
			hipLaunchKernelGGL(pieces_flag_kernel, grid, block, 0, ctx->stream, A);
			cvxi::ExclusiveScan(ctx->stream, A.rank, (int)nodes, reinterpret_cast<unsigned long long *>(nodeScratch + oRankChunks), &A.totals->floating);
			if (listed) { hipLaunchKernelGGL(pieces_list_kernel, grid, block, 0, ctx->stream, A); }
			e = hipGetLastError();
			// the totals go in front of the list, so that ONE copy brings them and the list's head
			if (e == hipSuccess) { e = hipMemcpyAsync(nodeScratch + oHead, A.totals, sizeof(Totals), hipMemcpyDeviceToDevice, ctx->stream); }
			if (e == hipSuccess) { e = hipMemcpyAsync(back.data(), nodeScratch + oHead, back.size(), hipMemcpyDeviceToHost, ctx->stream); }
		}
		if (e == hipSuccess) { e = hipEventRecord(ev[1], ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) {
			release();
			return FailHip(ctx, call, e);
		}
		std::memcpy(&host, back.data(), sizeof host);
	} else {
		e = hipEventRecord(ev[1], ctx->stream);
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) {
			release();
			return FailHip(ctx, call, e);
		}
	}
	const size_t floating = (size_t)host.summary.floatingPieces, wanted = std::min<size_t>(floating, (size_t)pieceCapacity);
	R->list.assign(wanted, cvx_piece{});
	if (wanted) {
		const size_t head = std::min(wanted, kHead);
		std::memcpy(R->list.data(), back.data() + sizeof(Totals), head * sizeof(cvx_piece));
		if (wanted > head) {
			e = hipMemcpy(R->list.data() + head, A.list + head, (wanted - head) * sizeof(cvx_piece), hipMemcpyDeviceToHost);
			if (e != hipSuccess) {
				release();
				return FailHip(ctx, call, e);
			}
		}
	}
	R->ms = 0.f;
	(void)hipEventElapsedTime(&R->ms, ev[0], ev[1]);
	return CVX_OK;
}

} // namespace cvxpieces

extern "C" {

int cvx_world_pieces(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount, cvx_piece *pieces,
                     int pieceCapacity, cvx_pieces_summary *summary, float *outDeviceMs)
{
	using namespace cvxpieces;
	static const char *const call = "cvx_world_pieces";
	char bad[32];
	std::snprintf(bad, sizeof bad, "bad op %d", op);
	Analysis R;
	int rc = Analyse(ctx, call, boxMin, boxMax, anchors, op != CVX_PIECES_REPORT && op != CVX_PIECES_REMOVE ? bad : nullptr, levelCount, pieces, pieceCapacity, &R);
	if (rc != CVX_OK) { return rc; }
	PiecesArgs &A = R.A;
	Totals &host = R.host;
	const size_t nodes = R.nodes, floating = (size_t)host.summary.floatingPieces;
	float ms = R.ms;
	struct Held { // (Analyse left its tables to this call)
		Analysis &R;
		~Held() { R.Release(); }
	} held{ R };

	// 6. REMOVE: the floating pieces' rectangle without them, through cvx_world_edit's machinery (cvxi::ColumnEdit)
	if (op == CVX_PIECES_REMOVE && floating) {
		cvxi::EditRectangle E;
		rc = cvxi::RoundEditRectangle(ctx, host.x0, host.x1, host.z0, host.z1, levelCount, "a removal over", &E);
		if (rc != CVX_OK) { return rc; }
		A.rx0 = E.x0;
		A.rz0 = E.z0;
		A.rSizeZ = E.sizeZ;
		A.rn = E.n;
		const cvxi::ColumnEditTotals totals{ A.totals, &host, sizeof host, offsetof(Totals, elements), offsetof(Totals, overLimit) };
		cvxi::ColumnEditCall edit{ call, FailHip, "a column without its floating runs", "the columns of the removal" };
		edit.totals = &totals;
		edit.done = R.ev[1];
		rc = cvxi::ColumnEdit(
			ctx, E, levelCount, edit,
			[&](const cvxi::ColumnEditJob &J) {
				A.counts = J.counts;
				hipLaunchKernelGGL(pieces_mark_kernel, dim3(Grid(nodes)), dim3(kThreads), 0, ctx->stream, A);
				hipLaunchKernelGGL(pieces_remove_count_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			[&](const cvxi::ColumnEditJob &J) {
				A.headers = J.headers;
				A.elements = J.elements;
				hipLaunchKernelGGL(pieces_remove_write_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			nullptr);
		if (rc != CVX_OK) { return rc; }
		(void)hipEventElapsedTime(&ms, R.ev[0], R.ev[1]);
	}
	// (nothing is handed out before the call can no longer fail)
	if (!R.list.empty()) { std::memcpy(pieces, R.list.data(), R.list.size() * sizeof(cvx_piece)); }
	if (summary) { *summary = host.summary; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // extern "C"
