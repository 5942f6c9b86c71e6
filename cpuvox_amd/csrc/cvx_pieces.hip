// cvx_pieces.hip -- libcpuvox_gpu.so, the floating pieces of the device-resident world (cvx_world_pieces).  See include/cpuvox_gpu.h for the
// contract and cvx_pieces.h for the rules.
//
// Connected components over the solid RUNS of LOD 0 inside the box, not over its voxels: a node is one solid run of one column clipped to the
// box's y range, an edge joins nodes of face-neighbouring columns whose y intervals overlap (and the two halves of a split run).  The components
// are the engine's (cvx_components.h, steps 1 .. 5); this file adds
//   the rule    PiecesRule: cvx_pieces.h's runs, their stacking and their anchor bits
//   the select  the largest piece by two reductions (CVX_ANCHOR_LARGEST); the roots without an anchor flagged floating, totalled and ranked
//   6. REMOVE   cvxi::ColumnEdit (cvx_edit.hip) over the floating pieces' rectangle: count and write of the sub-world blob are
//               cvxb::PiecesRemoveColumn.  Nothing in the arena is written before its last step.
// cvxpieces::Analyse (cvx_pieces_nodes.h) is the analysis behind the argument checks: cvx_world_settle (cvx_settle.hip) goes on from its node tables too.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "cvx_context.h"
#include "cvx_pieces.h"
#include "cvx_pieces_nodes.h"

using cvxi::Fail;
using cvxi::Grid;
using cvxi::kThreads;
using cvxi::WaveReduce;

namespace cvxpieces {

using cvxcomp::ColumnNodes;
using cvxcomp::kSelected; // in a root's bits, besides CVX_ANCHOR_*: the piece floats
using cvxcomp::NodeArgs;

struct PiecesRule {
	CVX_HD static uint32_t Count(const cvxb::ArenaColumn &col, int64_t y0, int64_t y1) { return cvxb::PiecesRunCount(col, y0, y1); }
	// (count and intervals are both PiecesRunRange's: nothing is left for `count` to bound)
	CVX_HD static void Intervals(const cvxb::ArenaColumn &col, int64_t y0, int64_t y1, uint32_t, uint32_t *lohi) { (void)cvxb::PiecesClippedRuns(col, y0, y1, lohi); }
	CVX_HD static bool Stacked(uint32_t lo, uint32_t hiBelow) { return cvxb::PiecesStacked(lo, hiBelow); }
	CVX_HD static int Bits(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int64_t x, int64_t z, uint32_t lo, uint32_t hi)
	{
		return cvxb::PiecesNodeAnchors(W, B, x, z, lo, hi);
	}
};

__device__ inline Totals *TotalsOf(const NodeArgs &A) { return reinterpret_cast<Totals *>(A.totals); }

// CVX_ANCHOR_LARGEST: the most voxels, then the smallest root among the pieces that have them
__global__ __launch_bounds__(256) void pieces_most_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long v = i < A.nodes && A.parent[i] == i ? A.voxels[i] : 0ull;
	v = WaveReduce(v, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; });
	if ((threadIdx.x & 63u) == 0u && v) { atomicMax(&TotalsOf(A)->mostVoxels, v); }
}

__global__ __launch_bounds__(256) void pieces_largest_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t r = i < A.nodes && A.parent[i] == i && A.voxels[i] == TotalsOf(A)->mostVoxels ? i : 0xFFFFFFFFu;
	r = WaveReduce(r, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
	if ((threadIdx.x & 63u) == 0u && r != 0xFFFFFFFFu) { atomicMin(&TotalsOf(A)->largest, r); }
}

// roots: anchored or floating; rank = 1 for a floating root (-> its place in the list after the scan); the four totals and the floating pieces' XZ box
__global__ __launch_bounds__(256) void pieces_flag_kernel(NodeArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool root = i < A.nodes && A.parent[i] == i;
	bool floats = false;
	unsigned long long voxels = 0ull;
	int x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	if (root) {
		const bool anchored = A.bits[i] != 0u || ((A.faceMask & CVX_ANCHOR_LARGEST) && TotalsOf(A)->largest == i);
		floats = !anchored;
		voxels = A.voxels[i];
		if (floats) {
			const int32_t *b = A.bounds + 6 * (size_t)i;
			A.bits[i] |= kSelected;
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
	Totals *T = TotalsOf(A);
	if (fp) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.floatingPieces), fp);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.floatingVoxels), fv);
		atomicMin(&T->head.x0, x0);
		atomicMin(&T->head.z0, z0);
		atomicMax(&T->head.x1, x1);
		atomicMax(&T->head.z1, z1);
	}
	if (ap) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.anchoredPieces), ap);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.anchoredVoxels), av);
	}
}

// REMOVE (behind cvxcomp::MarkSelected): rank[i] = node i belongs to a floating piece
__global__ __launch_bounds__(256) void pieces_remove_count_kernel(NodeArgs A)
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

__global__ __launch_bounds__(256) void pieces_remove_write_kernel(NodeArgs A)
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

int Analyse(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, const char *extraError, int levelCount,
            const cvx_piece *pieces, int pieceCapacity, Analysis *R)
{
	if (!boxMin || !boxMax) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box is NULL"); }
	char bad[cvxb::kBoxMessage];
	if (cvxb::BoxCheck(boxMin, boxMax, 0, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", bad); }
	if (anchors & ~(CVX_ANCHOR_GROUND | CVX_ANCHOR_OUTSIDE | CVX_ANCHOR_LARGEST)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown anchors bits 0x%x", (unsigned)anchors); }
	if (extraError) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", extraError); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (pieceCapacity < 0 || (pieceCapacity > 0 && !pieces)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "pieceCapacity %d with %s list", pieceCapacity, pieces ? "a" : "no"); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const cvxcomp::Call engine{ call, "solid runs", cvxcomp::KernelsOf<PiecesRule>(), anchors, pieceCapacity, sizeof(Totals) };
	R->host = Totals{};
	return cvxcomp::Analyse(
		ctx, engine, boxMin, boxMax,
		[&](const NodeArgs &A) {
			const dim3 grid(Grid(A.nodes)), block(kThreads);
			if (anchors & CVX_ANCHOR_LARGEST) {
				hipLaunchKernelGGL(pieces_most_kernel, grid, block, 0, ctx->stream, A);
				hipLaunchKernelGGL(pieces_largest_kernel, grid, block, 0, ctx->stream, A);
			}
			hipLaunchKernelGGL(pieces_flag_kernel, grid, block, 0, ctx->stream, A);
			return hipSuccess;
		},
		&R->host, R);
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
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	Analysis R(ctx, call);
	int rc = Analyse(ctx, call, boxMin, boxMax, anchors, op != CVX_PIECES_REPORT && op != CVX_PIECES_REMOVE ? bad : nullptr, levelCount, pieces, pieceCapacity, &R);
	if (rc != CVX_OK) { return rc; }
	NodeArgs &A = R.A;
	Totals &host = R.host;
	float ms = R.ms;

	// 6. REMOVE: the floating pieces' rectangle without them, through cvx_world_edit's machinery (cvxi::ColumnEdit)
	if (op == CVX_PIECES_REMOVE && host.summary.floatingPieces) {
		cvxi::EditRectangle E;
		rc = cvxi::RoundEditRectangle(ctx, host.head.x0, host.head.x1, host.head.z0, host.head.z1, levelCount, "a removal over", &E);
		if (rc != CVX_OK) { return rc; }
		A.rx0 = E.x0;
		A.rz0 = E.z0;
		A.rSizeZ = E.sizeZ;
		A.rn = E.n;
		const cvxi::ColumnEditTotals totals{ A.totals, &host, sizeof host, offsetof(Totals, head.elements), offsetof(Totals, head.overLimit) };
		cvxi::ColumnEditCall edit{ call, CVX_ERR_CAPACITY, "a column without its floating runs", "the columns of the removal" };
		edit.totals = &totals;
		edit.done = R.device.Event(1);
		rc = cvxi::ColumnEdit(
			ctx, E, levelCount, edit,
			[&](const cvxi::ColumnEditJob &J) {
				A.counts = J.counts;
				cvxcomp::MarkSelected(ctx->stream, A);
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
		ms = R.device.Ms();
	}
	// (nothing is handed out before the call can no longer fail)
	if (!R.list.empty()) { std::memcpy(pieces, R.list.data(), R.list.size() * sizeof(cvx_piece)); }
	if (summary) { *summary = host.summary; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // extern "C"
