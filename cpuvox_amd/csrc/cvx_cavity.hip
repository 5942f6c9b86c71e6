// cvx_cavity.hip -- libcpuvox_gpu.so, the enclosed cavities of the device-resident world (cvx_world_cavities).  See include/cpuvox_gpu.h for the
// contract and cvx_cavity.h for the rules.
//
// Connected components over the AIR intervals of LOD 0 inside the box, not over its voxels: a node is one maximal air interval of one column
// inside the box's y range, an edge joins nodes of face-neighbouring columns whose y intervals overlap.  The components are the engine's
// (cvx_components.h, steps 1 .. 5; the sky is one region with a node in every column); this file adds
//   the rule    CavityRule: cvx_cavity.h's air intervals and their open bits; nodes of one column are never joined
//   the select  the roots flagged open / enclosed / selected (maxVoxels), totalled, and the selected ones ranked
//   6. FILL     cvxi::ColumnEdit (cvx_edit.hip) over the selected cavities' rectangle: count and write of the sub-world blob are
//               cvxb::CavityFillColumn.  Nothing in the arena is written before its last step.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "cvx_cavity.h"
#include "cvx_components.h"
#include "cvx_context.h"

using cvxi::Fail;
using cvxi::Grid;
using cvxi::kThreads;
using cvxi::WaveReduce;

namespace cvxcavity {

using cvxcomp::kSelected;
using cvxcomp::NodeArgs;

struct Totals {
	cvxcomp::TotalsHead head; // listed: the selected cavities; x0 .. z1: their XZ bounding box
	cvx_cavities_summary summary{};
};
static_assert(sizeof(Totals) % 16 == 0, "the list follows the totals");

struct CavityArgs {
	NodeArgs N;
	unsigned long long maxVoxels;
	uint32_t argb;
};

struct CavityRule {
	CVX_HD static uint32_t Count(const cvxb::ArenaColumn &col, int64_t y0, int64_t y1) { return cvxb::CavityNodeCount(col, y0, y1); }
	// cvxb::CavityNodes, bounded by the count of step 1 whatever the walk gives
	CVX_HD static void Intervals(const cvxb::ArenaColumn &col, int64_t y0, int64_t y1, uint32_t count, uint32_t *lohi)
	{
		cvxb::CavityWalk w = cvxb::CavityWalkFrom(col, y1);
		for (uint32_t j = 0; j < count; j++) {
			uint32_t lo = 0u, hi = 0u;
			(void)cvxb::CavityNextNode(col, y0, &w, &lo, &hi);
			lohi[2 * (size_t)j] = lo;
			lohi[2 * (size_t)j + 1] = hi;
		}
	}
	CVX_HD static bool Stacked(uint32_t, uint32_t) { return false; }
	CVX_HD static int Bits(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int64_t x, int64_t z, uint32_t lo, uint32_t hi)
	{
		return cvxb::CavityNodeOpen(W, B, x, z, lo, hi);
	}
};

// roots: open, enclosed, or enclosed and selected; rank = 1 for a selected root (-> its place in the list after the scan); the six totals and the
// selected cavities' XZ box
__global__ __launch_bounds__(256) void cavity_flag_kernel(CavityArgs C)
{
	const NodeArgs &A = C.N;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool root = i < A.nodes && A.parent[i] == i;
	bool open = false, selected = false;
	unsigned long long voxels = 0ull;
	int x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	if (root) {
		open = A.bits[i] != 0u;
		voxels = A.voxels[i];
		selected = !open && (C.maxVoxels == 0ull || voxels <= C.maxVoxels);
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
	Totals *T = reinterpret_cast<Totals *>(A.totals);
	if (ec) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.enclosedCavities), ec);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.enclosedVoxels), ev);
	}
	if (sc) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.selectedCavities), sc);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.selectedVoxels), sv);
		atomicMin(&T->head.x0, x0);
		atomicMin(&T->head.z0, z0);
		atomicMax(&T->head.x1, x1);
		atomicMax(&T->head.z1, z1);
	}
	if (oc) {
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.openRegions), oc);
		atomicAdd(reinterpret_cast<unsigned long long *>(&T->summary.openVoxels), ov);
	}
}

// FILL (behind cvxcomp::MarkSelected): rank[i] = node i belongs to a selected cavity
__global__ __launch_bounds__(256) void cavity_fill_count_kernel(CavityArgs C)
{
	const NodeArgs &A = C.N;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.rn) { return; }
	const int cx = A.rx0 + i / A.rSizeZ, cz = A.rz0 + i % A.rSizeZ;
	uint32_t nodes;
	const cvxb::BrushResult r = cvxb::CavityFillColumn(A.W, cx, cz, A.B.y0, A.B.y1, cvxcomp::ColumnNodes(A, A.rank, cx, cz, &nodes), C.argb, nullptr, nullptr);
	if (r.overLimit) { atomicOr(&A.totals->overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void cavity_fill_write_kernel(CavityArgs C)
{
	const NodeArgs &A = C.N;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.rn) { return; }
	const int cx = A.rx0 + i / A.rSizeZ, cz = A.rz0 + i % A.rSizeZ;
	uint32_t nodes;
	const uint32_t *selected = cvxcomp::ColumnNodes(A, A.rank, cx, cz, &nodes);
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	const cvxb::BrushResult r = cvxb::CavityFillColumn(A.W, cx, cz, A.B.y0, A.B.y1, selected, C.argb, nullptr, nullptr);
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::CavityFillColumn(A.W, cx, cz, A.B.y0, A.B.y1, selected, C.argb, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

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
	char bad[cvxb::kBoxMessage];
	if (cvxb::BoxCheck(P.boxMin, P.boxMax, 0, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", bad); }
	if (P.openFaces & ~0x3F) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "unknown openFaces bits 0x%x", (unsigned)P.openFaces); }
	if (P.op != CVX_CAVITIES_REPORT && P.op != CVX_CAVITIES_FILL) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad op %d", P.op); }
	if (P.maxVoxels < 0) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "maxVoxels %lld is negative", (long long)P.maxVoxels); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (cavityCapacity < 0 || (cavityCapacity > 0 && !cavities)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "cavityCapacity %d with %s list", cavityCapacity, cavities ? "a" : "no");
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }

	const cvxcomp::Call engine{ call, "air intervals", cvxcomp::KernelsOf<CavityRule>(), P.openFaces, cavityCapacity, sizeof(Totals) };
	CavityArgs C{};
	C.maxVoxels = (unsigned long long)P.maxVoxels;
	C.argb = P.argb;
	Totals host{};
	cvxcomp::Analysis R(ctx, call);
	int rc = cvxcomp::Analyse(
		ctx, engine, P.boxMin, P.boxMax,
		[&](const NodeArgs &A) {
			C.N = A;
			hipLaunchKernelGGL(cavity_flag_kernel, dim3(Grid(A.nodes)), dim3(kThreads), 0, ctx->stream, C);
			return hipSuccess;
		},
		&host, &R);
	if (rc != CVX_OK) { return rc; }
	NodeArgs &A = C.N;
	A = R.A;
	float ms = R.ms, editMs = 0.f;

	// 6. FILL: the selected cavities' rectangle with them solid, through cvx_world_edit's machinery (cvxi::ColumnEdit)
	if (P.op == CVX_CAVITIES_FILL && host.summary.selectedCavities) {
		cvxi::EditRectangle E;
		rc = cvxi::RoundEditRectangle(ctx, host.head.x0, host.head.x1, host.head.z0, host.head.z1, levelCount, "a fill over", &E);
		if (rc != CVX_OK) { return rc; }
		A.rx0 = E.x0;
		A.rz0 = E.z0;
		A.rSizeZ = E.sizeZ;
		A.rn = E.n;
		const cvxi::ColumnEditTotals totals{ A.totals, &host, sizeof host, offsetof(Totals, head.elements), offsetof(Totals, head.overLimit) };
		cvxi::ColumnEditCall edit{ call, CVX_ERR_CAPACITY, "a filled column", "the columns of the fill", " (one colour per voxel)" };
		edit.totals = &totals;
		edit.done = R.device.Event(1);
		rc = cvxi::ColumnEdit(
			ctx, E, levelCount, edit,
			[&](const cvxi::ColumnEditJob &J) {
				A.counts = J.counts;
				cvxcomp::MarkSelected(ctx->stream, A);
				hipLaunchKernelGGL(cavity_fill_count_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, C);
				return hipSuccess;
			},
			[&](const cvxi::ColumnEditJob &J) {
				A.headers = J.headers;
				A.elements = J.elements;
				hipLaunchKernelGGL(cavity_fill_write_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, C);
				return hipSuccess;
			},
			nullptr);
		if (rc != CVX_OK) { return rc; }
		ms = R.device.Ms();
		editMs = ms - R.ms; // (the second event is the end of the analysis first and the end of the edit then)
	}
#ifdef CVX_CAVITY_DIAG
	g_lastMs[0] = R.ms;
	g_lastMs[1] = editMs;
	g_lastCounts[0] = (int64_t)R.nodes;
	g_lastCounts[1] = R.rounds;
#else
	(void)editMs;
#endif
	// (nothing is handed out before the call can no longer fail)
	if (!R.list.empty()) { std::memcpy(cavities, R.list.data(), R.list.size() * sizeof(cvx_piece)); }
	if (summary) { *summary = host.summary; }
	if (outDeviceMs) { *outDeviceMs = ms; }
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
