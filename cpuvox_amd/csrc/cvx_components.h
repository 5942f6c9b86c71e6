// cvx_components.h -- connected components over the column intervals of a box of the device-resident world: the engine under cvx_world_pieces,
// cvx_world_settle (solid runs, cvx_pieces.hip) and cvx_world_cavities (air intervals, cvx_cavity.hip).
//
// A node is one interval [lo, hi) of one column inside the box's y range, an edge joins nodes of face-neighbouring columns whose intervals overlap
// (cvxb::PiecesTouch) and, where the caller's rule says so, consecutive nodes of one column.  A RULE is a struct of statics (PiecesRule, CavityRule):
//   CVX_HD static uint32_t Count(const cvxb::ArenaColumn &col, int64_t y0, int64_t y1)                      the nodes of a column
//   CVX_HD static void Intervals(const cvxb::ArenaColumn &col, int64_t y0, int64_t y1, uint32_t count, uint32_t *lohi)
//                                                            their lo, hi from the top; `count` is what Count gave, no more than that is written
//   CVX_HD static bool Stacked(uint32_t lo, uint32_t hiBelow)                                               node j and node j + 1 of one column are joined
//   CVX_HD static int Bits(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int64_t x, int64_t z, uint32_t lo, uint32_t hi)
//                                                            what a node gives its component, masked with NodeArgs::faceMask
// cvxcomp::Analyse (cvx_components.hip) runs on ctx->stream:
//   1. count  (a thread per column of the box): its nodes; cvxi::ExclusiveScan gives the node offsets; ONE copy brings the total to the host
//   2. nodes  (a thread per column): interval, column and label (= its own index) of every node, in column order and top-down inside a column,
//             so that the smallest node index of a component is its seed
//   3. hook   (a thread per node): the node's interval against the sorted node lists of the +X and +Z neighbour columns and the node below it;
//             every edge is a lock-free union, the root with the larger index hooked under the smaller one with atomicMin, retried until both
//             ends have one root; then a flatten pass points every node at its root.  The two are repeated until a hook pass changes no label
//             (the first pass does all the work, the second confirms it: no round limit decides the result)
//   4. stats  (a thread per node, reduced per wave where a wave has one root): voxels, bounding box and bits of every root; then the caller's
//             select launcher flags the roots it wants with kSelected and rank = 1 and totals what it reports; a scan of the ranks in index
//             order = the order of the contract
//   5. list   the first `capacity` selected components, copied to the host behind the totals
// and leaves the node tables on the device for the call's edit (REMOVE, settle, FILL).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "cvx_context.h"
#include "cvx_pieces.h" // cvxb::PiecesBox, PiecesClipBox, PiecesTouch

namespace cvxcomp {

constexpr uint32_t kSelected = 0x100u; // in a root's bits, besides the rule's: the call's select kernel chose the component

// What every call's totals begin with; the call's own struct (a multiple of 16 bytes: the list follows it) has this as its first member.
struct TotalsHead {
	unsigned long long nodes = 0;    // the count scan's total
	unsigned long long listed = 0;   // the rank scan's total: the selected components
	unsigned long long elements = 0; // the call's edit: the blob's element count
	unsigned int changed = 0;        // a hook pass hooked something
	unsigned int overLimit = 0;      // the call's edit
	int x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN; // XZ bounding box of the selected components
};

struct NodeArgs {
	cvxb::CopyWorld W;
	cvxb::PiecesBox B;
	int n;                      // columns of the box
	uint32_t nodes;
	int faceMask;               // the bits of the rule that count: anchors / openFaces
	uint32_t *offsets;          // n + 1: the first node of every column
	uint32_t *lohi;             // per node: lo, hi
	uint32_t *column;           // per node: its column in the box
	uint32_t *parent;           // per node: the label; after the analysis: its root
	unsigned long long *voxels; // per root
	int32_t *bounds;            // per root: min x, y, z, max x, y, z
	uint32_t *bits;             // per root: the rule's bits | kSelected
	uint32_t *rank;             // per node: selected root -> its place in the list; after MarkSelected: the node belongs to a selected component
	TotalsHead *totals;         // the call's totals struct
	cvx_piece *list;
	int capacity;
	// the call's edit: the rectangle and its blob
	int rx0, rz0, rSizeZ, rn;
	uint32_t *counts;
	uint32_t *headers;
	uint32_t *elements;
};

// The rule's four kernels (KernelsOf<Rule>() below); flatten, list and mark depend on no rule and live in cvx_components.hip.
struct RuleKernels {
	void (*count)(NodeArgs);
	void (*nodes)(NodeArgs);
	void (*hook)(NodeArgs);
	void (*stats)(NodeArgs);
};

struct Call {
	const char *call;     // the entry point's name for messages
	const char *nodeNoun; // "the box holds %llu <solid runs>"
	RuleKernels kernels;
	int faceMask;
	int capacity;         // of the caller's list
	size_t totalsBytes;   // of the call's totals struct
};

// The call's select kernels behind the stats kernel: they see every root's voxels, bounds and bits, set kSelected and rank = 1 for the roots the
// call lists (rank = 0 for every other node) and total what the call reports, the selected components' XZ box among it.
using SelectLauncher = cvxi::Launcher<NodeArgs>;

// What Analyse leaves behind.  `device` holds the analysis' events and its scratch until the struct goes: A.offsets / A.totals live in its first
// block, the node tables in its second (none when the box holds no node).  A call that goes on to cvxi::ColumnEdit hands it device.Event(1) as
// `done`; device.Ms() then spans the analysis and the edit.
struct Analysis {
	NodeArgs A{};
	size_t nodes = 0;
	int64_t rounds = 0;          // hook / flatten passes
	std::vector<cvx_piece> list; // the first min(capacity, selected) selected components
	float ms = 0.f;              // device time of the analysis alone
	cvxi::DeviceCall device;

	Analysis(cvx_context *ctx, const char *call) : device(ctx, call) {}
};

// Clips the box (CVX_ERR_INVALID_ARGUMENT when nothing of it is inside the world), lays the world out (cvxi::SyncWorld) and runs steps 1 .. 5.
// hostTotals: the call's totals struct with its initial value; it goes to the device as it is and comes back with the analysis' results.
int Analyse(cvx_context *ctx, const Call &call, const int32_t boxMin[3], const int32_t boxMax[3], SelectLauncher select, void *hostTotals, Analysis *R);
// The call's edit: rank[i] = node i belongs to a selected component (enqueued on `stream`)
void MarkSelected(hipStream_t stream, const NodeArgs &A);

#ifdef __HIPCC__
// The root of i; every node on the way is pointed at its grandparent (labels only ever fall, so a late or lost update is harmless).
__device__ inline uint32_t Find(uint32_t *parent, uint32_t i)
{
	for (;;) {
		const uint32_t p = cvxi::Load(parent + i);
		if (p == i) { return i; }
		const uint32_t g = cvxi::Load(parent + p);
		if (g != p) { atomicMin(parent + i, g); }
		i = g;
	}
}

// Joins the components of a and b: the larger root goes under the smaller one.  atomicMin returns what the larger one pointed at: itself -> hooked;
// anything else -> somebody hooked it first, and whichever of the two labels it keeps now, the other one still has to be joined with it.
__device__ inline bool Unite(uint32_t *parent, uint32_t a, uint32_t b)
{
	bool changed = false;
	for (;;) {
		a = Find(parent, a);
		b = Find(parent, b);
		if (a == b) { return changed; }
		const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
		const uint32_t old = atomicMin(parent + hi, lo);
		changed = true;
		if (old == hi) { return true; }
		a = old;
		b = lo;
	}
}

// the nodes of column (cx, cz) of the rectangle in a per-node table: none outside the box
__device__ inline const uint32_t *ColumnNodes(const NodeArgs &A, const uint32_t *perNode, int cx, int cz, uint32_t *count)
{
	*count = 0u;
	if (!A.B.Holds(cx, cz)) { return nullptr; }
	const int64_t c = A.B.Column(cx, cz);
	*count = A.offsets[c + 1] - A.offsets[c];
	return perNode + A.offsets[c];
}

template <class Rule> __global__ __launch_bounds__(256) void count_kernel(NodeArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > A.n) { return; }
	if (i == A.n) { // (the scan then leaves the node total behind the last column's offset)
		A.offsets[i] = 0u;
		return;
	}
	const int64_t x = A.B.x0 + i / A.B.SizeZ(), z = A.B.z0 + i % A.B.SizeZ();
	A.offsets[i] = Rule::Count(cvxb::CopyColumnAt(A.W, x, z), A.B.y0, A.B.y1);
}

template <class Rule> __global__ __launch_bounds__(256) void nodes_kernel(NodeArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t first = A.offsets[i], count = A.offsets[i + 1] - first;
	if (count == 0u) { return; }
	const int64_t x = A.B.x0 + i / A.B.SizeZ(), z = A.B.z0 + i % A.B.SizeZ();
	Rule::Intervals(cvxb::CopyColumnAt(A.W, x, z), A.B.y0, A.B.y1, count, A.lohi + 2 * (size_t)first);
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
__device__ inline bool HookColumn(const NodeArgs &A, uint32_t i, uint32_t lo, uint32_t hi, uint32_t c2)
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

template <class Rule> __global__ __launch_bounds__(256) void hook_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.nodes) { return; }
	const uint32_t lo = A.lohi[2 * (size_t)i], hi = A.lohi[2 * (size_t)i + 1], c = A.column[i];
	const int sizeZ = A.B.SizeZ();
	bool changed = false;
	if (i + 1u < A.offsets[c + 1] && Rule::Stacked(lo, A.lohi[2 * (size_t)(i + 1u) + 1])) { changed = Unite(A.parent, i, i + 1u); }
	if ((int)(c / (uint32_t)sizeZ) + 1 < A.B.SizeX()) { changed = HookColumn(A, i, lo, hi, c + (uint32_t)sizeZ) || changed; }
	if ((int)(c % (uint32_t)sizeZ) + 1 < sizeZ) { changed = HookColumn(A, i, lo, hi, c + 1u) || changed; }
	if (changed) { atomicOr(&A.totals->changed, 1u); }
}

// Totals of the roots.  Neighbouring nodes mostly belong to one component (the largest piece, the sky): a wave whose nodes have one root reduces
// first and sends one set of atomics.
template <class Rule> __global__ __launch_bounds__(256) void stats_kernel(NodeArgs A)
{
	using cvxi::WaveReduce;
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
		bits = (uint32_t)(Rule::Bits(A.W, A.B, x, z, lo, hi) & A.faceMask);
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

template <class Rule> RuleKernels KernelsOf() { return RuleKernels{ count_kernel<Rule>, nodes_kernel<Rule>, hook_kernel<Rule>, stats_kernel<Rule> }; }
#endif

} // namespace cvxcomp
