// cvx_cavity.hip -- libcpuvox_gpu.so, the enclosed cavities of the device-resident world (cvx_world_cavities).  See include/cpuvox_gpu.h for the
// contract and cvx_cavity.h for the rules.
//
// Connected components over the AIR intervals of LOD 0 inside the box, not over its voxels: a node is one maximal air interval of one column
// inside the box's y range, an edge joins nodes of face-neighbouring columns whose y intervals overlap.  cvx_pieces.hip's steps on other nodes:
//   1. count  (a thread per column of the box): its nodes; cvxi::ExclusiveScan gives the node offsets; ONE copy brings the total to the host
//   2. nodes  (a thread per column): interval, column and label (= its own index) of every node, in column order and top-down inside a column,
//             so that the smallest node index of a region is its seed
//   3. hook   (a thread per node): the node's interval against the sorted node lists of the +X and +Z neighbour columns; every edge is a
//             lock-free union (cvx_pieces_nodes.h); then a flatten pass points every node at its root.  The two are repeated until a hook pass
//             changes no label: no round limit decides the result
//   4. stats  (a thread per node, reduced per wave where a wave has one root -- the sky is one region with a node in every column): voxels,
//             bounding box and open bits of every root; then the roots are flagged open / enclosed / selected (maxVoxels), totalled, and the
//             selected ones ranked by a scan in index order = the order of the contract
//   5. list   the first cavityCapacity selected cavities, copied to the host behind the totals
//   6. FILL   cvxi::ColumnEdit (cvx_edit.hip) over the selected cavities' rectangle: count and write of the sub-world blob are
//             cvxb::CavityFillColumn.  Nothing in the arena is written before its last step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvx_cavity.h"
#include "cvx_context.h"
#include "cvx_pieces_nodes.h"

using cvxi::Fail;

namespace cvxcavity {

using cvxpieces::FailHip;
using cvxpieces::Grid;
using cvxpieces::kThreads;
using cvxpieces::WaveReduce;

constexpr uint32_t kSelected = 0x100u; // in a root's bits, besides the six open bits

struct Totals {
	unsigned long long nodes;    // the count scan's total
	unsigned long long listed;   // the rank scan's total
	unsigned long long elements; // FILL: the blob's element count
	unsigned int changed;        // a hook pass hooked something
	unsigned int overLimit;      // FILL
	int x0, x1, z0, z1;          // XZ bounding box of the selected cavities
	unsigned int pad[4];
	cvx_cavities_summary summary;
};
static_assert(sizeof(Totals) % 16 == 0, "the list follows the totals");

struct CavityArgs {
	cvxb::CopyWorld W;
	cvxb::PiecesBox B;
	int n;                      // columns of the box
	uint32_t nodes;
	int openFaces;
	unsigned long long maxVoxels;
	uint32_t argb;
	uint32_t *offsets;          // n + 1: the first node of every column
	uint32_t *lohi;             // per node: lo, hi
	uint32_t *column;           // per node: its column in the box
	uint32_t *parent;           // per node: the label; after the analysis: its root
	unsigned long long *voxels; // per root
	int32_t *bounds;            // per root: min x, y, z, max x, y, z
	uint32_t *bits;             // per root: open bits | kSelected
	uint32_t *rank;             // per node: selected root -> its place in the list; FILL later: the node is filled
	Totals *totals;
	cvx_piece *list;
	int capacity;
	// FILL: the rectangle and its blob
	int rx0, rz0, rSizeZ, rn;
	uint32_t *counts;
	uint32_t *headers;
	uint32_t *elements;
};

__global__ __launch_bounds__(256) void cavity_count_kernel(CavityArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > A.n) { return; }
	if (i == A.n) { // (the scan then leaves the node total behind the last column's offset)
		A.offsets[i] = 0u;
		return;
	}
	const int64_t x = A.B.x0 + i / A.B.SizeZ(), z = A.B.z0 + i % A.B.SizeZ();
	A.offsets[i] = cvxb::CavityNodeCount(cvxb::CopyColumnAt(A.W, x, z), A.B.y0, A.B.y1);
}

__global__ __launch_bounds__(256) void cavity_nodes_kernel(CavityArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t first = A.offsets[i], count = A.offsets[i + 1] - first;
	if (count == 0u) { return; }
	const int64_t x = A.B.x0 + i / A.B.SizeZ(), z = A.B.z0 + i % A.B.SizeZ();
	const cvxb::ArenaColumn col = cvxb::CopyColumnAt(A.W, x, z);
	cvxb::CavityWalk w = cvxb::CavityWalkFrom(col, A.B.y1);
	for (uint32_t j = first; j < first + count; j++) { // (bounded by the count of step 1 whatever the walk gives)
		uint32_t lo = 0u, hi = 0u;
		(void)cvxb::CavityNextNode(col, A.B.y0, &w, &lo, &hi);
		A.lohi[2 * (size_t)j] = lo;
		A.lohi[2 * (size_t)j + 1] = hi;
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
__device__ inline bool HookColumn(const CavityArgs &A, uint32_t i, uint32_t lo, uint32_t hi, uint32_t c2)
{
	const uint32_t e = A.offsets[c2 + 1];
	uint32_t a = A.offsets[c2], b = e; // the first node whose lo is below hi
	while (a < b) {
		const uint32_t mid = (a + b) >> 1;
		if (A.lohi[2 * (size_t)mid] >= hi) { a = mid + 1u; } else { b = mid; }
	}
	bool changed = false;
	for (uint32_t s = a; s < e && cvxb::PiecesTouch(lo, hi, A.lohi[2 * (size_t)s], A.lohi[2 * (size_t)s + 1]); s++) {
		changed = cvxpieces::Unite(A.parent, i, s) || changed;
	}
	return changed;
}

__global__ __launch_bounds__(256) void cavity_hook_kernel(CavityArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	const uint32_t lo = A.lohi[2 * (size_t)i], hi = A.lohi[2 * (size_t)i + 1], c = A.column[i];
	const int sizeZ = A.B.SizeZ();
	bool changed = false;
	if ((int)(c / (uint32_t)sizeZ) + 1 < A.B.SizeX()) { changed = HookColumn(A, i, lo, hi, c + (uint32_t)sizeZ); }
	if ((int)(c % (uint32_t)sizeZ) + 1 < sizeZ) { changed = HookColumn(A, i, lo, hi, c + 1u) || changed; }
	if (changed) { atomicOr(&A.totals->changed, 1u); }
}

__global__ __launch_bounds__(256) void cavity_flatten_kernel(CavityArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	const uint32_t r = cvxpieces::Find(A.parent, i);
	if (r != i) { atomicMin(A.parent + i, r); }
}

// Totals of the roots.  Neighbouring nodes mostly belong to one region (the sky): a wave whose nodes have one root reduces first and sends one
// set of atomics.
__global__ __launch_bounds__(256) void cavity_stats_kernel(CavityArgs A)
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
		bits = (uint32_t)(cvxb::CavityNodeOpen(A.W, A.B, x, z, lo, hi) & A.openFaces);
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

// roots: open, enclosed, or enclosed and selected; rank = 1 for a selected root (-> its place in the list after the scan); the six totals and the
// selected cavities' XZ box
__global__ __launch_bounds__(256) void cavity_flag_kernel(CavityArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool root = i < A.nodes && A.parent[i] == i;
	bool open = false, selected = false;
	unsigned long long voxels = 0ull;
	int x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	if (root) {
		open = A.bits[i] != 0u;
		voxels = A.voxels[i];
		selected = !open && (A.maxVoxels == 0ull || voxels <= A.maxVoxels);
		if (selected) {
			const int32_t *b = A.bounds + 6 * (size_t)i;
			A.bits[i] = kSelected;
			x0 = b[0]; z0 = b[2]; x1 = b[3]; z1 = b[5];
		}
	}
	if (i < A.nodes) { A.rank[i] = selected ? 1u : 0u; }
	auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
	const bool enclosed = root && !open;
	const unsigned long long ec = WaveReduce<unsigned long long>(enclosed ? 1ull : 0ull, add), ev = WaveReduce<unsigned long long>(enclosed ? voxels : 0ull, add);
	const unsigned long long sc = WaveReduce<unsigned long long>(selected ? 1ull : 0ull, add), sv = WaveReduce<unsigned long long>(selected ? voxels : 0ull, add);
	const unsigned long long oc = WaveReduce<unsigned long long>(open ? 1ull : 0ull, add), ov = WaveReduce<unsigned long long>(open ? voxels : 0ull, add);
	x0 = WaveReduce(x0, [](int p, int q) { return p < q ? p : q; });
	z0 = WaveReduce(z0, [](int p, int q) { return p < q ? p : q; });
	x1 = WaveReduce(x1, [](int p, int q) { return p > q ? p : q; });
	z1 = WaveReduce(z1, [](int p, int q) { return p > q ? p : q; });
	if ((threadIdx.x & 63u) != 0u) { return; }
	Totals *T = A.totals;
	if (ec) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.enclosedCavities), ec);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.enclosedVoxels), ev);
	}
	if (sc) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.selectedCavities), sc);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.selectedVoxels), sv);
		atomicMin(&T->x0, x0);
		atomicMin(&T->z0, z0);
		atomicMax(&T->x1, x1);
		atomicMax(&T->z1, z1);
	}
	if (oc) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.openRegions), oc);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.openVoxels), ov);
	}
}

__global__ __launch_bounds__(256) void cavity_list_kernel(CavityArgs A)
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

// FILL: rank[i] = node i belongs to a selected cavity
__global__ __launch_bounds__(256) void cavity_mark_kernel(CavityArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	A.rank[i] = (A.bits[A.parent[i]] & kSelected) ? 1u : 0u;
}

// the per-node table of column (cx, cz) of the rectangle: null outside the box
__device__ inline const uint32_t *ColumnNodes(const CavityArgs &A, int cx, int cz)
{
	return A.B.Holds(cx, cz) ? A.rank + A.offsets[A.B.Column(cx, cz)] : nullptr;
}

__global__ __launch_bounds__(256) void cavity_fill_count_kernel(CavityArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.rn) { return; }
	const int cx = A.rx0 + i / A.rSizeZ, cz = A.rz0 + i % A.rSizeZ;
	const cvxb::BrushResult r = cvxb::CavityFillColumn(A.W, cx, cz, A.B.y0, A.B.y1, ColumnNodes(A, cx, cz), A.argb, nullptr, nullptr);
	if (r.overLimit) { atomicOr(&A.totals->overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void cavity_fill_write_kernel(CavityArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.rn) { return; }
	const int cx = A.rx0 + i / A.rSizeZ, cz = A.rz0 + i % A.rSizeZ;
	const uint32_t *selected = ColumnNodes(A, cx, cz);
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	const cvxb::BrushResult r = cvxb::CavityFillColumn(A.W, cx, cz, A.B.y0, A.B.y1, selected, A.argb, nullptr, nullptr);
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::CavityFillColumn(A.W, cx, cz, A.B.y0, A.B.y1, selected, A.argb, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

constexpr size_t kHead = 256; // cavities that come to the host with the totals, in one copy

#if defined(CVX_EXPERIMENTS) || defined(CVX_PROFILE_SECTIONS) /* include/cpuvox_gpu_diag.h: cvx_debug_cavities */
#define CVX_CAVITY_DIAG 1
static float g_lastMs[2] = { 0.f, 0.f };
static int64_t g_lastCounts[2] = { -1, 0 };
#endif

} // namespace cvxcavity

extern "C" {

int cvx_world_cavities(cvx_context *ctx, const cvx_cavity_params *params, int levelCount, cvx_piece *cavities, int cavityCapacity,
                       cvx_cavities_summary *summary, float *outDeviceMs)
{
	using namespace cvxcavity;
	static const char *const call = "cvx_world_cavities";
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!params) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "params is NULL"); }
	const cvx_cavity_params P = *params;
	for (int a = 0; a < 3; a++) {
		if (P.boxMin[a] >= P.boxMax[a]) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box [%d, %d) on axis %d is empty", P.boxMin[a], P.boxMax[a], a); }
	}
	if (P.openFaces & ~0x3F) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown openFaces bits 0x%x", (unsigned)P.openFaces); }
	if (P.op != CVX_CAVITIES_REPORT && P.op != CVX_CAVITIES_FILL) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad op %d", P.op); }
	if (P.maxVoxels < 0) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "maxVoxels %lld is negative", (long long)P.maxVoxels); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (cavityCapacity < 0 || (cavityCapacity > 0 && !cavities)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "cavityCapacity %d with %s list", cavityCapacity, cavities ? "a" : "no");
	}
	if (!ctx->levelSet[0]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD 0 has not been uploaded"); }
	const int dim[3] = { ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ };
	CavityArgs A{};
	if (!cvxb::PiecesClipBox(P.boxMin, P.boxMax, dim[0], dim[1], dim[2], &A.B)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box lies outside the world"); }
	if (A.B.Columns() >= ((int64_t)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "a box of %lld columns", (long long)A.B.Columns()); }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	int rc = cvxi::SyncWorld(ctx);
	if (rc != CVX_OK) { return rc; }

	const int n = (int)A.B.Columns();
	hipEvent_t ev[3] = { nullptr, nullptr, nullptr }; // start, the analysis, the edit
	uint8_t *columnScratch = nullptr, *nodeScratch = nullptr;
	auto release = [&]() {
		for (uint8_t *p : { columnScratch, nodeScratch }) { if (p) { (void)hipFree(p); } }
		for (hipEvent_t e : ev) { if (e) { (void)hipEventDestroy(e); } }
	};
	size_t bytes = 0;
	auto carve = [&](size_t b) { const size_t at = bytes; bytes = (bytes + b + 15) & ~(size_t)15; return at; };
	auto chunksOf = [](size_t count) { return (count + cvxi::ScanChunk() - 1) / cvxi::ScanChunk(); };

	// 1. the nodes of every column, their offsets, the total
	const size_t oTotals = carve(sizeof(Totals)), oOffsets = carve(((size_t)n + 1) * 4), oChunks = carve(chunksOf((size_t)n + 1) * 8);
	Totals host{};
	host.x0 = host.z0 = INT_MAX;
	host.x1 = host.z1 = INT_MIN;
	hipError_t e = hipSuccess;
	for (hipEvent_t &event : ev) { if (e == hipSuccess) { e = hipEventCreate(&event); } }
	if (e == hipSuccess) { e = hipMalloc((void **)&columnScratch, bytes); }
	if (e == hipSuccess) { e = hipEventRecord(ev[0], ctx->stream); }
	if (e == hipSuccess) { e = hipMemcpyAsync(columnScratch + oTotals, &host, sizeof host, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.n = n;
		A.openFaces = P.openFaces;
		A.maxVoxels = (unsigned long long)P.maxVoxels;
		A.argb = P.argb;
		A.totals = reinterpret_cast<Totals *>(columnScratch + oTotals);
		A.offsets = reinterpret_cast<uint32_t *>(columnScratch + oOffsets);
		hipLaunchKernelGGL(cavity_count_kernel, dim3(Grid((size_t)n + 1)), dim3(kThreads), 0, ctx->stream, A);
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
		return Fail(ctx, CVX_ERR_CAPACITY, "the box holds %llu air intervals", host.nodes);
	}
	const size_t nodes = (size_t)host.nodes;
	A.nodes = (uint32_t)nodes;
	A.capacity = cavityCapacity;
	const size_t listed = std::min<size_t>((size_t)cavityCapacity, nodes);

	// 2 .. 5. the node table, the components, the totals, the list
	bytes = 0;
	const size_t oHead = carve(sizeof(Totals)), oList = carve(listed * sizeof(cvx_piece)), oLohi = carve(nodes * 8), oColumn = carve(nodes * 4), oParent = carve(nodes * 4),
	             oVoxels = carve(nodes * 8), oBounds = carve(nodes * 24), oBits = carve(nodes * 4), oRank = carve(nodes * 4), oRankChunks = carve(chunksOf(nodes) * 8);
	std::vector<uint8_t> back(sizeof(Totals) + std::min(listed, kHead) * sizeof(cvx_piece));
	int64_t rounds = 0;
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
		hipLaunchKernelGGL(cavity_nodes_kernel, dim3(Grid((size_t)n)), block, 0, ctx->stream, A);
		for (;;) { // until a pass hooks nothing
			e = hipMemsetAsync(&A.totals->changed, 0, sizeof(unsigned int), ctx->stream);
			if (e != hipSuccess) { break; }
			hipLaunchKernelGGL(cavity_hook_kernel, grid, block, 0, ctx->stream, A);
			hipLaunchKernelGGL(cavity_flatten_kernel, grid, block, 0, ctx->stream, A);
			rounds++;
			e = hipGetLastError();
			if (e == hipSuccess) { e = hipMemcpyAsync(&host.changed, &A.totals->changed, sizeof host.changed, hipMemcpyDeviceToHost, ctx->stream); }
			if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
			if (e != hipSuccess || !host.changed) { break; }
		}
		if (e == hipSuccess) {
			hipLaunchKernelGGL(cavity_stats_kernel, grid, block, 0, ctx->stream, A);
			hipLaunchKernelGGL(cavity_flag_kernel, grid, block, 0, ctx->stream, A);
			cvxi::ExclusiveScan(ctx->stream, A.rank, (int)nodes, reinterpret_cast<unsigned long long *>(nodeScratch + oRankChunks), &A.totals->listed);
			if (listed) { hipLaunchKernelGGL(cavity_list_kernel, grid, block, 0, ctx->stream, A); }
			e = hipGetLastError();
			// the totals go in front of the list, so that ONE copy brings them and the list's head
			if (e == hipSuccess) { e = hipMemcpyAsync(nodeScratch + oHead, A.totals, sizeof(Totals), hipMemcpyDeviceToDevice, ctx->stream); }
			if (e == hipSuccess) { e = hipMemcpyAsync(back.data(), nodeScratch + oHead, back.size(), hipMemcpyDeviceToHost, ctx->stream); }
		}
	}
	if (e == hipSuccess) { e = hipEventRecord(ev[1], ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) {
		release();
		return FailHip(ctx, call, e);
	}
	if (nodes) { std::memcpy(&host, back.data(), sizeof host); }
	const size_t selected = (size_t)host.summary.selectedCavities, wanted = std::min<size_t>(selected, (size_t)cavityCapacity);
	std::vector<cvx_piece> list(wanted, cvx_piece{});
	if (wanted) {
		const size_t head = std::min(wanted, kHead);
		std::memcpy(list.data(), back.data() + sizeof(Totals), head * sizeof(cvx_piece));
		if (wanted > head) {
			e = hipMemcpy(list.data() + head, A.list + head, (wanted - head) * sizeof(cvx_piece), hipMemcpyDeviceToHost);
			if (e != hipSuccess) {
				release();
				return FailHip(ctx, call, e);
			}
		}
	}
	float ms = 0.f, editMs = 0.f;
	(void)hipEventElapsedTime(&ms, ev[0], ev[1]);
	const float analysisMs = ms;

	// 6. FILL: the selected cavities' rectangle with them solid, through cvx_world_edit's machinery (cvxi::ColumnEdit)
	if (P.op == CVX_CAVITIES_FILL && selected) {
		cvxi::EditRectangle E;
		rc = cvxi::RoundEditRectangle(ctx, host.x0, host.x1, host.z0, host.z1, levelCount, "a fill over", &E);
		if (rc != CVX_OK) {
			release();
			return rc;
		}
		A.rx0 = E.x0;
		A.rz0 = E.z0;
		A.rSizeZ = E.sizeZ;
		A.rn = E.n;
		const cvxi::ColumnEditTotals totals{ A.totals, &host, sizeof host, offsetof(Totals, elements), offsetof(Totals, overLimit) };
		cvxi::ColumnEditCall edit{ call, FailHip, "a filled column", "the columns of the fill", " (one colour per voxel)" };
		edit.totals = &totals;
		edit.done = ev[2];
		rc = cvxi::ColumnEdit(
			ctx, E, levelCount, edit,
			[&](const cvxi::ColumnEditJob &J) {
				A.counts = J.counts;
				hipLaunchKernelGGL(cavity_mark_kernel, dim3(Grid(nodes)), dim3(kThreads), 0, ctx->stream, A);
				hipLaunchKernelGGL(cavity_fill_count_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			[&](const cvxi::ColumnEditJob &J) {
				A.headers = J.headers;
				A.elements = J.elements;
				hipLaunchKernelGGL(cavity_fill_write_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			nullptr);
		if (rc != CVX_OK) {
			release();
			return rc;
		}
		(void)hipEventElapsedTime(&ms, ev[0], ev[2]);
		(void)hipEventElapsedTime(&editMs, ev[1], ev[2]);
	}
#ifdef CVX_CAVITY_DIAG
	g_lastMs[0] = analysisMs;
	g_lastMs[1] = editMs;
	g_lastCounts[0] = (int64_t)nodes;
	g_lastCounts[1] = rounds;
#else
	(void)analysisMs;
	(void)editMs;
	(void)rounds;
#endif
	// (nothing is handed out before the call can no longer fail)
	if (!list.empty()) { std::memcpy(cavities, list.data(), list.size() * sizeof(cvx_piece)); }
	if (summary) { *summary = host.summary; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	release();
	return CVX_OK;
}

#ifdef CVX_CAVITY_DIAG
int cvx_debug_cavities(cvx_context *ctx, float outMs[2], int64_t outCounts[2])
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (outMs) { std::memcpy(outMs, cvxcavity::g_lastMs, sizeof cvxcavity::g_lastMs); }
	if (outCounts) { std::memcpy(outCounts, cvxcavity::g_lastCounts, sizeof cvxcavity::g_lastCounts); }
	return CVX_OK;
}
#endif

} // extern "C"
