// cvx_settle.hip -- libcpuvox_gpu.so, the floating pieces of the device-resident world fall until they rest (cvx_world_settle).  See
// include/cpuvox_gpu.h for the contract and cvx_settle.h for the rules.
//
// The pieces and their node tables come from cvxpieces::Analyse (cvx_pieces.hip: the component engine of cvx_components.h with the pieces' rule
// and select kernels).  How far piece p falls is the largest d with
// d_p <= g for every node of p over something static with g voxels of air between, and d_p <= d_q + g for every node of p over floating piece q:
// the shortest-path distance to "static" in the piece graph, found by relaxation.
//   1. init   (a thread per node): drop[root] = the piece's lowest y (the floor bounds every piece), or maxDrop if that is smaller
//   2. gap    (a thread per floating node): cvxb::SettleBelow; a static constraint goes into drop[root] with atomicMin (one per wave where a
//             wave's nodes share a root), a constraint against another floating piece is kept per node as (root below, gap)
//   3. relax  (a thread per kept constraint): atomicMin(drop[p], drop[q] + g), repeated until a sweep changes nothing.  Distances only ever fall,
//             to the unique fixpoint: no round limit or schedule decides the result.  A stack of k pieces needs about k sweeps, so a box of at most
//             kSingleNodes nodes is relaxed by ONE workgroup that loops over its nodes with a barrier between sweeps and stops by itself; a
//             larger box runs kSweepsPerLaunch sweeps per launch and the host reads the changed flag between launches.
//   4. finish (a thread per node): the node's shift = its piece's drop; per floating root the drop in list order, and the totals and the XZ box of
//             the pieces that fall
//   5. cvxi::ColumnEdit (cvx_edit.hip) over that box's rectangle: count and write of the sub-world blob are cvxb::SettleColumn.  Nothing in
//             the arena is written before its last step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_pieces_nodes.h"
#include "cvx_settle.h"

using cvxi::Fail;

namespace cvxsettle {

using cvxi::Load;
using cvxi::WaveReduce;
using cvxcomp::kSelected; // (in a root's bits: its piece floats)
using cvxcomp::NodeArgs;

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr unsigned kSingleThreads = 1024;
constexpr size_t kSingleNodes = 4096;  // up to here one workgroup relaxes the whole box
constexpr int kSweepsPerLaunch = 8;    // above it

struct SettleTotals {
	unsigned int changed;  // a relax launch lowered a drop
	unsigned int sweeps;   // of the single-workgroup loop
	int largestDrop;
	int pad;
	int x0, x1, z0, z1;    // XZ bounding box of the pieces that fall
	long long fallenPieces, fallenVoxels;
};

struct SettleArgs {
	NodeArgs P;
	uint32_t *drop;   // per root: how far its piece falls
	uint32_t *below;  // per node: the root of the floating piece under it, kNone: no constraint to relax
	uint32_t *gap;    // per node: the air under it
	uint32_t *shift;  // per node: its piece's drop (0: a static node)
	int32_t *drops;   // the drops in list order, the first `capacity`
	SettleTotals *totals;
	uint32_t maxDrop; // 0: no bound
	int sweeps;       // per launch of settle_relax_kernel
};

__device__ inline bool Floats(const NodeArgs &P, uint32_t root) { return (P.bits[root] & kSelected) != 0u; }

__global__ __launch_bounds__(256) void settle_init_kernel(SettleArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.P.nodes) { return; }
	uint32_t d = 0u;
	if (A.P.parent[i] == i && Floats(A.P, i)) {
		d = (uint32_t)A.P.bounds[6 * (size_t)i + 1];
		if (A.maxDrop && A.maxDrop < d) { d = A.maxDrop; }
	}
	A.drop[i] = d;
}

__global__ __launch_bounds__(256) void settle_gap_kernel(SettleArgs A)
{
	const NodeArgs &P = A.P;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t root = kNone, bound = kNone;
	bool active = false;
	if (i < P.nodes) {
		root = P.parent[i];
		active = Floats(P, root);
		uint32_t below = kNone, gap = 0u;
		if (active) {
			const uint32_t c = P.column[i], j = i - P.offsets[c], count = P.offsets[c + 1] - P.offsets[c];
			const int64_t x = P.B.x0 + (int)(c / (uint32_t)P.B.SizeZ()), z = P.B.z0 + (int)(c % (uint32_t)P.B.SizeZ());
			const cvxb::SettleConstraint con = cvxb::SettleBelow(cvxb::CopyColumnAt(P.W, x, z), P.B.y0, P.B.y1, j, count);
			const bool hasNode = con.kind == cvxb::SETTLE_NODE; // (then node i + 1 is in this column)
			const uint32_t rootBelow = hasNode ? P.parent[i + 1u] : 0u;
			const uint32_t kind = cvxb::SettleResolve(con.kind, root, rootBelow, hasNode && Floats(P, rootBelow));
			gap = con.gap;
			if (kind == cvxb::SETTLE_STATIC) { bound = gap; }
			if (kind == cvxb::SETTLE_NODE) { below = rootBelow; }
		}
		A.below[i] = below;
		A.gap[i] = gap;
	}
	const unsigned long long mask = __ballot(active);
	if (mask == 0ull) { return; }
	const int leader = __ffsll(mask) - 1;
	const uint32_t first = __shfl(root, leader, 64);
	if (__all(!active || root == first)) {
		bound = WaveReduce(bound, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
		if ((int)(threadIdx.x & 63u) != leader) { return; }
	}
	if (active && bound != kNone) { atomicMin(A.drop + root, bound); }
}

// one constraint, once; true: it lowered its piece's drop
__device__ inline bool Relax(const SettleArgs &A, uint32_t i)
{
	const uint32_t q = A.below[i];
	if (q == kNone) { return false; }
	const uint32_t v = Load(A.drop + q) + A.gap[i], p = A.P.parent[i];
	if (v >= Load(A.drop + p)) { return false; }
	atomicMin(A.drop + p, v);
	return true;
}

__global__ __launch_bounds__(256) void settle_relax_kernel(SettleArgs A)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.P.nodes || A.below[i] == kNone) { return; }
	bool changed = false;
	for (int s = 0; s < A.sweeps; s++) { changed = Relax(A, i) || changed; }
	if (changed) { atomicOr(&A.totals->changed, 1u); }
}

// the whole box in one workgroup: sweeps with a barrier between them until one changes nothing
__global__ __launch_bounds__(1024) void settle_relax_single_kernel(SettleArgs A)
{
	unsigned int sweeps = 0u;
	for (;;) {
		int changed = 0;
		for (uint32_t i = threadIdx.x; i < A.P.nodes; i += kSingleThreads) { changed |= Relax(A, i) ? 1 : 0; }
		sweeps++;
		if (!__syncthreads_or(changed)) { break; }
	}
	if (threadIdx.x == 0u) { A.totals->sweeps = sweeps; }
}

__global__ __launch_bounds__(256) void settle_finish_kernel(SettleArgs A)
{
	const NodeArgs &P = A.P;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	bool falls = false;
	long long voxels = 0;
	int d = 0, x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	if (i < P.nodes) {
		const uint32_t root = P.parent[i];
		const bool floats = Floats(P, root);
		A.shift[i] = floats ? A.drop[root] : 0u;
		if (floats && root == i) {
			d = (int)A.drop[i];
			if (P.rank[i] < (uint32_t)P.capacity) { A.drops[P.rank[i]] = d; }
			if (d > 0) {
				const int32_t *b = P.bounds + 6 * (size_t)i;
				falls = true;
				voxels = (long long)P.voxels[i];
				x0 = b[0]; z0 = b[2]; x1 = b[3]; z1 = b[5];
			}
		}
	}
	if (__ballot(falls) == 0ull) { return; }
	auto add = [](long long a, long long b) { return a + b; };
	const long long fp = WaveReduce<long long>(falls ? 1 : 0, add), fv = WaveReduce<long long>(voxels, add);
	d = WaveReduce(d, [](int p, int q) { return p > q ? p : q; });
	x0 = WaveReduce(x0, [](int p, int q) { return p < q ? p : q; });
	z0 = WaveReduce(z0, [](int p, int q) { return p < q ? p : q; });
	x1 = WaveReduce(x1, [](int p, int q) { return p > q ? p : q; });
	z1 = WaveReduce(z1, [](int p, int q) { return p > q ? p : q; });
	if ((threadIdx.x & 63u) != 0u) { return; }
	SettleTotals *T = A.totals;
	atomicAdd(reinterpret_cast<unsigned long long *>(&T->fallenPieces), (unsigned long long)fp);
	atomicAdd(reinterpret_cast<unsigned long long *>(&T->fallenVoxels), (unsigned long long)fv);
	atomicMax(&T->largestDrop, d);
	atomicMin(&T->x0, x0);
	atomicMin(&T->z0, z0);
	atomicMax(&T->x1, x1);
	atomicMax(&T->z1, z1);
}

__global__ __launch_bounds__(256) void settle_count_kernel(SettleArgs A)
{
	const NodeArgs &P = A.P;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.rn) { return; }
	const int cx = P.rx0 + i / P.rSizeZ, cz = P.rz0 + i % P.rSizeZ;
	uint32_t nodes;
	const uint32_t *shift = cvxcomp::ColumnNodes(P, A.shift, cx, cz, &nodes);
	const cvxb::BrushResult r = cvxb::SettleColumn(P.W, cx, cz, P.B.y0, P.B.y1, shift, nodes, nullptr, nullptr);
	if (r.overLimit) { atomicOr(&P.totals->overLimit, 1u); }
	P.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void settle_write_kernel(SettleArgs A)
{
	const NodeArgs &P = A.P;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.rn) { return; }
	const int cx = P.rx0 + i / P.rSizeZ, cz = P.rz0 + i % P.rSizeZ;
	uint32_t nodes;
	const uint32_t *shift = cvxcomp::ColumnNodes(P, A.shift, cx, cz, &nodes);
	const uint32_t off = P.counts[i];
	uint32_t *e = P.elements + off;
	const cvxb::BrushResult r = cvxb::SettleColumn(P.W, cx, cz, P.B.y0, P.B.y1, shift, nodes, nullptr, nullptr);
	uint32_t *h = P.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::SettleColumn(P.W, cx, cz, P.B.y0, P.B.y1, shift, nodes, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

#if defined(CVX_EXPERIMENTS) || defined(CVX_PROFILE_SECTIONS) /* include/cpuvox_gpu_diag.h: cvx_debug_settle */
#define CVX_SETTLE_DIAG 1
static int g_oneSweepPerLaunch = 0;
static float g_lastMs[3] = { 0.f, 0.f, 0.f };
static int64_t g_lastCounts[4] = { -1, 0, 0, 0 };
#endif

} // namespace cvxsettle

extern "C" {

int cvx_world_settle(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int maxDrop, int levelCount, cvx_piece *pieces, int32_t *drops,
                     int pieceCapacity, cvx_settle_summary *summary, float *outDeviceMs)
{
	using namespace cvxsettle;
	using cvxi::Grid;
	using cvxi::kThreads;
	static const char *const call = "cvx_world_settle";
	char bad[40];
	std::snprintf(bad, sizeof bad, "maxDrop %d is negative", maxDrop);
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxpieces::Analysis R(ctx, call);
	int rc = cvxpieces::Analyse(ctx, call, boxMin, boxMax, anchors, maxDrop < 0 ? bad : nullptr, levelCount, pieces, pieceCapacity, &R);
	if (rc != CVX_OK) { return rc; }
	const size_t nodes = R.nodes, floating = (size_t)R.host.summary.floatingPieces, wanted = R.list.size();
	cvx_settle_summary out{};
	out.floatingPieces = R.host.summary.floatingPieces;
	out.floatingVoxels = R.host.summary.floatingVoxels;
	float ms = R.ms;
	std::vector<int32_t> dropList(wanted, 0);
	// the drops: their scratch, and the event pair from the analysis' start to the end of the relaxation
	std::vector<uint8_t> back; // (outlives relax: freeing the device blocks waits for a copy still under way)
	cvxi::DeviceCall relax(ctx, call);
	uint8_t *settleScratch = nullptr;
	cvxi::ScratchLayout carve;
	unsigned sweeps = 0, launches = 0;
	bool single = nodes <= kSingleNodes;
	float relaxMs = 0.f, editMs = 0.f;

	SettleArgs A{};
	SettleTotals host{};
	if (floating) {
		// 1 .. 4. the drops
		const size_t oTotals = carve(sizeof(SettleTotals)), oDrops = carve(std::max<size_t>(wanted, 1) * 4), oDrop = carve(nodes * 4), oBelow = carve(nodes * 4),
		             oGap = carve(nodes * 4), oShift = carve(nodes * 4);
		static_assert(sizeof(SettleTotals) % 16 == 0, "the drops follow the totals");
		back.resize(sizeof(SettleTotals) + wanted * 4);
		host.x0 = host.z0 = INT_MAX;
		host.x1 = host.z1 = INT_MIN;
		hipError_t e = relax.Begin(R.device.Event(0));
		if (e == hipSuccess) { e = relax.Allocate(&settleScratch, carve.bytes); }
		if (e == hipSuccess) { e = hipMemcpyAsync(settleScratch + oTotals, &host, sizeof host, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) {
			A.P = R.A;
			A.totals = reinterpret_cast<SettleTotals *>(settleScratch + oTotals);
			A.drops = reinterpret_cast<int32_t *>(settleScratch + oDrops);
			A.drop = reinterpret_cast<uint32_t *>(settleScratch + oDrop);
			A.below = reinterpret_cast<uint32_t *>(settleScratch + oBelow);
			A.gap = reinterpret_cast<uint32_t *>(settleScratch + oGap);
			A.shift = reinterpret_cast<uint32_t *>(settleScratch + oShift);
			A.maxDrop = (uint32_t)maxDrop;
			A.sweeps = kSweepsPerLaunch;
#ifdef CVX_SETTLE_DIAG
			if (g_oneSweepPerLaunch) {
				single = false;
				A.sweeps = 1;
			}
#endif
			const dim3 grid(Grid(nodes)), block(kThreads);
			hipLaunchKernelGGL(settle_init_kernel, grid, block, 0, ctx->stream, A);
			hipLaunchKernelGGL(settle_gap_kernel, grid, block, 0, ctx->stream, A);
			e = hipGetLastError();
			if (e == hipSuccess && single) {
				hipLaunchKernelGGL(settle_relax_single_kernel, dim3(1), dim3(kSingleThreads), 0, ctx->stream, A);
				launches = 1;
				e = hipGetLastError();
			}
			while (e == hipSuccess && !single) { // until a launch lowers nothing
				e = hipMemsetAsync(&A.totals->changed, 0, sizeof(unsigned int), ctx->stream);
				if (e != hipSuccess) { break; }
				hipLaunchKernelGGL(settle_relax_kernel, grid, block, 0, ctx->stream, A);
				launches++;
				e = hipGetLastError();
				if (e == hipSuccess) { e = hipMemcpyAsync(&host.changed, &A.totals->changed, sizeof host.changed, hipMemcpyDeviceToHost, ctx->stream); }
				if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
				if (e != hipSuccess || !host.changed) { break; }
			}
			if (e == hipSuccess) {
				hipLaunchKernelGGL(settle_finish_kernel, grid, block, 0, ctx->stream, A);
				e = hipGetLastError();
			}
			// (the drops lie behind the totals: ONE copy brings both)
			if (e == hipSuccess) { e = hipMemcpyAsync(back.data(), settleScratch + oTotals, back.size(), hipMemcpyDeviceToHost, ctx->stream); }
			if (e == hipSuccess) { e = relax.End(); }
			if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		}
		if (e != hipSuccess) { return relax.Fail(e); }
		std::memcpy(&host, back.data(), sizeof host);
		if (wanted) { std::memcpy(dropList.data(), back.data() + sizeof host, wanted * 4); }
		sweeps = single ? host.sweeps : launches * (unsigned)A.sweeps;
		ms = relax.Ms();
		relaxMs = ms - R.ms; // (the analysis' end is the relaxation's start)
		out.fallenPieces = host.fallenPieces;
		out.fallenVoxels = host.fallenVoxels;
		out.largestDrop = host.largestDrop;
	}

	// 5. the rectangle of the pieces that fall, with them where they land, through cvx_world_edit's machinery (cvxi::ColumnEdit)
	if (out.fallenPieces) {
		NodeArgs &P = A.P;
		cvxi::EditRectangle E;
		rc = cvxi::RoundEditRectangle(ctx, host.x0, host.x1, host.z0, host.z1, levelCount, "a settle over", &E);
		if (rc != CVX_OK) { return rc; }
		P.rx0 = E.x0;
		P.rz0 = E.z0;
		P.rSizeZ = E.sizeZ;
		P.rn = E.n;
		cvxpieces::Totals back{};
		const cvxi::ColumnEditTotals totals{ P.totals, &back, sizeof back, offsetof(cvxpieces::Totals, head.elements), offsetof(cvxpieces::Totals, head.overLimit) };
		cvxi::ColumnEditCall edit{ call, CVX_ERR_CAPACITY, "a column with its pieces settled", "the columns of the settle" };
		edit.totals = &totals;
		edit.done = R.device.Event(1);
		rc = cvxi::ColumnEdit(
			ctx, E, levelCount, edit,
			[&](const cvxi::ColumnEditJob &J) {
				P.counts = J.counts;
				hipLaunchKernelGGL(settle_count_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			[&](const cvxi::ColumnEditJob &J) {
				P.headers = J.headers;
				P.elements = J.elements;
				hipLaunchKernelGGL(settle_write_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			nullptr);
		if (rc != CVX_OK) { return rc; }
		ms = R.device.Ms();
		editMs = ms - relax.Ms(); // (the relaxation's end is the edit's start)
	}
#ifdef CVX_SETTLE_DIAG
	g_lastMs[0] = R.ms;
	g_lastMs[1] = relaxMs;
	g_lastMs[2] = editMs;
	g_lastCounts[0] = (int64_t)nodes;
	g_lastCounts[1] = sweeps;
	g_lastCounts[2] = launches;
	g_lastCounts[3] = floating && single ? 1 : 0;
#else
	(void)sweeps;
	(void)relaxMs;
	(void)editMs;
#endif
	// (nothing is handed out before the call can no longer fail)
	if (wanted) { std::memcpy(pieces, R.list.data(), wanted * sizeof(cvx_piece)); }
	if (wanted && drops) { std::memcpy(drops, dropList.data(), wanted * sizeof(int32_t)); }
	if (summary) { *summary = out; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

#ifdef CVX_SETTLE_DIAG
int cvx_debug_settle(cvx_context *ctx, int oneSweepPerLaunch, float outMs[3], int64_t outCounts[4])
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (oneSweepPerLaunch >= 0) { cvxsettle::g_oneSweepPerLaunch = oneSweepPerLaunch ? 1 : 0; }
	if (outMs) { std::memcpy(outMs, cvxsettle::g_lastMs, sizeof cvxsettle::g_lastMs); }
	if (outCounts) { std::memcpy(outCounts, cvxsettle::g_lastCounts, sizeof cvxsettle::g_lastCounts); }
	return CVX_OK;
}
#endif

} // extern "C"
