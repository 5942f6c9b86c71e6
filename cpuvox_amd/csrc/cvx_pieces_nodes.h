// cvx_pieces_nodes.h -- the node tables of cvx_pieces.hip (steps 1 .. 5 of its header comment), left on the device for the calls that go on from
// them: cvx_world_pieces' REMOVE and cvx_world_settle (cvx_settle.hip); the lock-free union-find is shared with cvx_world_cavities (cvx_cavity.hip).  cvxpieces::Analyse checks the arguments the two calls share, runs the
// analysis and brings the totals and the head of the list to the host; the caller frees the tables with Analysis::Release.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "cvx_context.h"
#include "cvx_pieces.h"

namespace cvxpieces {

constexpr uint32_t kFloats = 0x100u; // in a root's bits, besides CVX_ANCHOR_*
constexpr unsigned kThreads = 256;

inline unsigned Grid(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

struct Totals {
	unsigned long long nodes;      // the count scan's total
	unsigned long long floating;   // the rank scan's total
	unsigned long long elements;   // REMOVE / settle: the blob's element count
	unsigned long long mostVoxels; // the largest piece
	unsigned int largest;          // ... its root
	unsigned int changed;          // a hook pass hooked something
	unsigned int overLimit;        // REMOVE / settle
	unsigned int pad;
	int x0, x1, z0, z1;            // XZ bounding box of the floating pieces
	cvx_pieces_summary summary;
};

struct PiecesArgs {
	cvxb::CopyWorld W;
	cvxb::PiecesBox B;
	int n;                         // columns of the box
	uint32_t nodes;
	int anchors;
	uint32_t *offsets;             // n + 1: the first node of every column
	uint32_t *lohi;                // per node: lo, hi
	uint32_t *column;              // per node: its column in the box
	uint32_t *parent;              // per node: the label; after the analysis: its root
	unsigned long long *voxels;    // per root
	int32_t *bounds;               // per root: min x, y, z, max x, y, z
	uint32_t *bits;                // per root: CVX_ANCHOR_* | kFloats
	uint32_t *rank;                // per node: floating root -> its place in the list; REMOVE later: the node floats
	Totals *totals;
	cvx_piece *list;
	int capacity;
	// REMOVE / settle: the rectangle and its blob
	int rx0, rz0, rSizeZ, rn;
	uint32_t *counts;
	uint32_t *headers;
	uint32_t *elements;
};

// What Analyse leaves behind.  A.offsets / A.totals live in columnScratch; the node tables in nodeScratch (null when the box holds no solid run).
struct Analysis {
	PiecesArgs A{};
	Totals host{};               // the totals, on the host
	size_t nodes = 0;
	int dim[3] = { 0, 0, 0 };    // the world
	std::vector<cvx_piece> list; // the first min(pieceCapacity, floatingPieces) floating pieces
	float ms = 0.f;              // device time of the analysis: ev[0] .. ev[1]
	hipEvent_t ev[2] = { nullptr, nullptr };
	uint8_t *columnScratch = nullptr, *nodeScratch = nullptr;

	void Release();
};

// `call`: the entry point's name for messages.  `extraError` (may be null): the message of the call's own argument check (op / maxDrop), reported
// as CVX_ERR_INVALID_ARGUMENT in its place among the shared checks.  Anything but CVX_OK: everything is released already.
int Analyse(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, const char *extraError, int levelCount,
            const cvx_piece *pieces, int pieceCapacity, Analysis *R);
// hipErrorOutOfMemory -> CVX_ERR_CAPACITY, anything else -> CVX_ERR_HIP
int FailHip(cvx_context *ctx, const char *call, hipError_t e);

#ifdef __HIPCC__
__device__ inline uint32_t Load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, typename F> __device__ inline T WaveReduce(T v, F f)
{
	for (int d = 32; d > 0; d >>= 1) { v = f(v, __shfl_xor(v, d, 64)); }
	return v;
}

// The root of i; every node on the way is pointed at its grandparent (labels only ever fall, so a late or lost update is harmless).
__device__ inline uint32_t Find(uint32_t *parent, uint32_t i)
{
	for (;;) {
		const uint32_t p = Load(parent + i);
		if (p == i) { return i; }
		const uint32_t g = Load(parent + p);
		if (g != p) { atomicMin(parent + i, g); }
		i = g;
	}
}

// Joins the pieces of a and b: the larger root goes under the smaller one.  atomicMin returns what the larger one pointed at: itself -> hooked;
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
__device__ inline const uint32_t *ColumnNodes(const PiecesArgs &A, const uint32_t *perNode, int cx, int cz, uint32_t *count)
{
	*count = 0u;
	if (!A.B.Holds(cx, cz)) { return nullptr; }
	const int64_t c = A.B.Column(cx, cz);
	*count = A.offsets[c + 1] - A.offsets[c];
	return perNode + A.offsets[c];
}
#endif

} // namespace cvxpieces
