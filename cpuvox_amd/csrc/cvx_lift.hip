// cvx_lift.hip -- libcpuvox_gpu.so, the floating pieces of the device-resident world as models with mass moments (cvx_world_lift_pieces).  See
// include/cpuvox_gpu_lift.h for the contract and cvx_lift.h for the rules.
//
// The pieces and their node tables come from cvxpieces::Analyse (cvx_pieces.hip: the component engine of cvx_components.h with the pieces' rule
// and select kernels): after it parent[i] is node i's root, bits[root] & kSelected says the piece floats, rank[root] is its place in the list and
// bounds[root] its box.  The host takes the list, runs cvxb::LiftPlan and uploads the offsets; then
//   1. moments (a thread per node): cvxb::LiftNodeSums of the nodes of listed pieces, added to the piece's nine sums with 64-bit atomics; a wave
//              whose nodes share one root reduces first and sends one set.  A second small kernel totals the box volumes of ALL floating roots.
//   2. write   (a wave per 64 consecutive nodes) behind a hipMemsetAsync of [0, storedVoxels) of each pool: an inclusive scan of the nodes'
//              lengths (0 for a node that is not stored) across the wave, then the wave walks its voxels 64 per step; lane l finds the node
//              that owns voxel t + l by a six-step search of the prefix sums read through __shfl and stores one colour word and one mask
//              byte.  y is the fastest axis of the box, so the lanes of one node store consecutive addresses; the 64 nodes of a wave may
//              belong to 64 pieces.  No LDS, no state across waves.
//   3. REMOVE  mark[i] = node i belongs to a STORED piece (a table of its own: rank[root] is still being read by the other nodes of the
//              piece), then cvxi::ColumnEdit (cvx_edit.hip) over the stored pieces' rectangle: count and write of the sub-world blob are
//              cvxb::PiecesRemoveColumn, as in cvx_world_pieces.  The pools are complete before the edit; nothing in the arena is written
//              before the edit's last step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "cvx_context.h"
#include "cvx_lift.h"
#include "cvx_pieces_nodes.h"

using cvxi::Fail;

namespace cvxlift {

using cvxi::WaveReduce;
using cvxcomp::kSelected; // (in a root's bits: its piece floats)
using cvxcomp::NodeArgs;

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct LiftArgs {
	NodeArgs P;
	const int64_t *offsets;     // per listed piece: LiftPlan's
	unsigned long long *sums;   // per listed piece: sum[3], moment[6]
	unsigned long long *needed; // the box volumes of all floating pieces
	uint32_t *mark;             // per node (REMOVE): it belongs to a stored piece
	uint32_t *argb;             // the pools; either may be null
	uint8_t *solid;
	uint32_t listed, stored;    // pieces
};

__global__ __launch_bounds__(256) void lift_moments_kernel(LiftArgs A)
{
	const NodeArgs &P = A.P;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t root = kNone, place = 0u;
	bool active = false;
	unsigned long long s[9] = { 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull };
	if (i < P.nodes) {
		root = P.parent[i];
		if (P.bits[root] & kSelected) {
			place = P.rank[root];
			active = place < A.listed;
		}
		if (active) {
			const int32_t *b = P.bounds + 6 * (size_t)root;
			const uint32_t c = P.column[i];
			const int x = P.B.x0 + (int)(c / (uint32_t)P.B.SizeZ()), z = P.B.z0 + (int)(c % (uint32_t)P.B.SizeZ());
			uint64_t out[9];
			cvxb::LiftNodeSums((uint64_t)(x - b[0]), (uint64_t)(z - b[2]), (uint64_t)((int)P.lohi[2 * (size_t)i] - b[1]), (uint64_t)((int)P.lohi[2 * (size_t)i + 1] - b[1]), out);
			for (int k = 0; k < 9; k++) { s[k] = out[k]; }
		}
	}
	const unsigned long long mask = __ballot(active);
	if (mask == 0ull) { return; }
	const int leader = __ffsll(mask) - 1;
	const uint32_t first = __shfl(root, leader, 64);
	if (__all(!active || root == first)) {
		for (int k = 0; k < 9; k++) { s[k] = WaveReduce(s[k], [](unsigned long long a, unsigned long long b) { return a + b; }); }
		if ((int)(threadIdx.x & 63u) != leader) { return; }
	}
	if (!active) { return; }
	for (int k = 0; k < 9; k++) { atomicAdd(A.sums + 9 * (size_t)place + k, s[k]); }
}

__global__ __launch_bounds__(256) void lift_needed_kernel(LiftArgs A)
{
	const NodeArgs &P = A.P;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long v = 0ull;
	if (i < P.nodes && P.parent[i] == i && (P.bits[i] & kSelected)) {
		const int32_t *b = P.bounds + 6 * (size_t)i;
		v = (unsigned long long)cvxb::LiftVolume(b, b + 3);
	}
	v = WaveReduce(v, [](unsigned long long a, unsigned long long b) { return a + b; });
	if ((threadIdx.x & 63u) == 0u && v) { atomicAdd(A.needed, v); }
}

__global__ __launch_bounds__(256) void lift_write_kernel(LiftArgs A)
{
	const NodeArgs &P = A.P;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const int lane = (int)(threadIdx.x & 63u);
	uint32_t length = 0u, colourBase = 0u, colourIndex = 0u; // colourIndex: of the node's LOWEST voxel; voxel lo + j has colourIndex - j
	long long element = 0;                                 // of the node's lowest voxel in the pools
	if (i < P.nodes) {
		const uint32_t root = P.parent[i];
		if ((P.bits[root] & kSelected) && P.rank[root] < A.stored) {
			const uint32_t lo = P.lohi[2 * (size_t)i], hi = P.lohi[2 * (size_t)i + 1], c = P.column[i];
			const int x = P.B.x0 + (int)(c / (uint32_t)P.B.SizeZ()), z = P.B.z0 + (int)(c % (uint32_t)P.B.SizeZ());
			const cvxb::ArenaColumn col = cvxb::CopyColumnAt(P.W, x, z);
			const cvxb::SolidRun run = col.Run(cvxb::RunAtOrBelow(col, (int64_t)hi - 1)); // the run that holds the node
			const int32_t *b = P.bounds + 6 * (size_t)root;
			element = A.offsets[P.rank[root]] + cvxb::LiftElement(x - b[0], (int)lo - b[1], z - b[2], b[4] - b[1], b[5] - b[2]);
			colourBase = col.ColorsBase();
			colourIndex = run.colorsIndex + (run.top - 1u - lo);
			length = hi - lo;
		}
	}
	uint32_t before = length; // inclusive scan of the lengths across the wave
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(before, d, 64);
		if (lane >= d) { before += t; }
	}
	const uint32_t total = __shfl(before, 63, 64);
	const int shift = P.W.colorShift - 2;
	for (uint32_t t = 0u; t < total; t += 64u) {
		const uint32_t v = t + (uint32_t)lane;
		int owner = 0; // the first lane whose inclusive sum is above v (v < total: there is one)
		for (int step = 32; step > 0; step >>= 1) {
			if (__shfl(before, owner + step - 1, 64) <= v) { owner += step; }
		}
		owner &= 63; // (v >= total: any lane, nothing is stored)
		const uint32_t ownerEnd = __shfl(before, owner, 64), ownerLength = __shfl(length, owner, 64);
		const uint32_t base = __shfl(colourBase, owner, 64), index = __shfl(colourIndex, owner, 64);
		const long long at = __shfl(element, owner, 64);
		if (v < total) {
			const uint32_t j = v - (ownerEnd - ownerLength);
			if (A.argb) { A.argb[at + j] = P.W.colourSlots[base + ((index - j) << shift)]; }
			if (A.solid) { A.solid[at + j] = (uint8_t)1; }
		}
	}
}

__global__ __launch_bounds__(256) void lift_mark_kernel(LiftArgs A)
{
	const NodeArgs &P = A.P;
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.nodes) { return; }
	const uint32_t root = P.parent[i];
	A.mark[i] = (P.bits[root] & kSelected) && P.rank[root] < A.stored ? 1u : 0u;
}

__global__ __launch_bounds__(256) void lift_remove_count_kernel(LiftArgs A)
{
	const NodeArgs &P = A.P;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.rn) { return; }
	const int cx = P.rx0 + i / P.rSizeZ, cz = P.rz0 + i % P.rSizeZ;
	uint32_t nodes;
	const uint32_t *gone = cvxcomp::ColumnNodes(P, A.mark, cx, cz, &nodes);
	const cvxb::BrushResult r = cvxb::PiecesRemoveColumn(P.W, cx, cz, P.B.y0, P.B.y1, gone, nodes, nullptr, nullptr);
	if (r.overLimit) { atomicOr(&P.totals->overLimit, 1u); }
	P.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void lift_remove_write_kernel(LiftArgs A)
{
	const NodeArgs &P = A.P;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.rn) { return; }
	const int cx = P.rx0 + i / P.rSizeZ, cz = P.rz0 + i % P.rSizeZ;
	uint32_t nodes;
	const uint32_t *gone = cvxcomp::ColumnNodes(P, A.mark, cx, cz, &nodes);
	const uint32_t off = P.counts[i];
	uint32_t *e = P.elements + off;
	const cvxb::BrushResult r = cvxb::PiecesRemoveColumn(P.W, cx, cz, P.B.y0, P.B.y1, gone, nodes, nullptr, nullptr);
	uint32_t *h = P.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::PiecesRemoveColumn(P.W, cx, cz, P.B.y0, P.B.y1, gone, nodes, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

// Both entry points: `device` says where the pools live.
static int Lift(cvx_context *ctx, const char *call, bool device, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount,
                cvx_lifted_piece *pieces, int pieceCapacity, uint32_t *argb, uint8_t *solid, int64_t voxelCapacity, cvx_lift_summary *summary, float *outDeviceMs)
{
	using cvxi::Grid;
	using cvxi::kThreads;
	char bad[96];
	const char *extra = nullptr;
	if (op != CVX_LIFT_COPY && op != CVX_LIFT_REMOVE) {
		std::snprintf(bad, sizeof bad, "bad op %d", op);
		extra = bad;
	} else if (voxelCapacity < 0) {
		std::snprintf(bad, sizeof bad, "voxelCapacity %lld is negative", (long long)voxelCapacity);
		extra = bad;
	} else if (voxelCapacity > 0 && !argb && !solid) {
		std::snprintf(bad, sizeof bad, "voxelCapacity %lld with no pool", (long long)voxelCapacity);
		extra = bad;
	}
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxpieces::Analysis R(ctx, call);
	// (the shared checks only ask whether there is a list)
	int rc = cvxpieces::Analyse(ctx, call, boxMin, boxMax, anchors, extra, levelCount, reinterpret_cast<const cvx_piece *>(pieces), pieceCapacity, &R);
	if (rc != CVX_OK) { return rc; }
	const size_t nodes = R.nodes, listed = R.list.size();
	std::vector<int64_t> offsets(listed, -1);
	const cvxb::LiftStored stored = cvxb::LiftPlan(R.list.data(), sizeof(cvx_piece), (int64_t)listed, voxelCapacity, offsets.data());
	const size_t storedVoxels = (size_t)stored.voxels;
	float ms = R.ms;

	// 1, 2. the sums and the pools: their scratch, and the event pair from the analysis' start to the end of the write
	std::vector<unsigned long long> back(2 + 9 * listed, 0ull); // needed, pad, the sums (outlives lift: freeing the device blocks waits for a copy still under way)
	cvxi::DeviceCall lift(ctx, call);
	LiftArgs A{};
	A.P = R.A;
	uint32_t *stagedArgb = nullptr;
	uint8_t *stagedSolid = nullptr;
	if (nodes && R.host.summary.floatingPieces) {
		uint8_t *scratch = nullptr;
		cvxi::ScratchLayout carve;
		const size_t oSums = carve(back.size() * 8), oOffsets = carve(std::max<size_t>(listed, 1) * 8), oMark = carve(op == CVX_LIFT_REMOVE && stored.pieces ? nodes * 4 : 0);
		hipError_t e = lift.Begin(R.device.Event(0));
		if (e == hipSuccess) { e = lift.Allocate(&scratch, carve.bytes); }
		if (e == hipSuccess && !device && storedVoxels && argb) { e = lift.Allocate(&stagedArgb, storedVoxels * 4); }
		if (e == hipSuccess && !device && storedVoxels && solid) { e = lift.Allocate(&stagedSolid, storedVoxels); }
		if (e == hipSuccess) { e = hipMemsetAsync(scratch + oSums, 0, back.size() * 8, ctx->stream); }
		if (e == hipSuccess && listed) { e = hipMemcpyAsync(scratch + oOffsets, offsets.data(), listed * 8, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) {
			A.needed = reinterpret_cast<unsigned long long *>(scratch + oSums);
			A.sums = A.needed + 2;
			A.offsets = reinterpret_cast<const int64_t *>(scratch + oOffsets);
			A.mark = reinterpret_cast<uint32_t *>(scratch + oMark);
			A.argb = device ? argb : stagedArgb;
			A.solid = device ? solid : stagedSolid;
			A.listed = (uint32_t)listed;
			A.stored = (uint32_t)stored.pieces;
			const dim3 grid(Grid(nodes)), block(kThreads);
			if (listed) { hipLaunchKernelGGL(lift_moments_kernel, grid, block, 0, ctx->stream, A); }
			hipLaunchKernelGGL(lift_needed_kernel, grid, block, 0, ctx->stream, A);
			e = hipGetLastError();
			if (e == hipSuccess && storedVoxels && A.argb) { e = hipMemsetAsync(A.argb, 0, storedVoxels * 4, ctx->stream); }
			if (e == hipSuccess && storedVoxels && A.solid) { e = hipMemsetAsync(A.solid, 0, storedVoxels, ctx->stream); }
			if (e == hipSuccess && stored.pieces && (A.argb || A.solid)) {
				hipLaunchKernelGGL(lift_write_kernel, grid, block, 0, ctx->stream, A);
				e = hipGetLastError();
			}
		}
		if (e == hipSuccess) { e = hipMemcpyAsync(back.data(), scratch + oSums, back.size() * 8, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = lift.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		// (the staged pools go to the host's before the edit: a failure here still leaves the world as it was)
		if (e == hipSuccess && stagedArgb) { e = hipMemcpy(argb, stagedArgb, storedVoxels * 4, hipMemcpyDeviceToHost); }
		if (e == hipSuccess && stagedSolid) { e = hipMemcpy(solid, stagedSolid, storedVoxels, hipMemcpyDeviceToHost); }
		if (e != hipSuccess) { return lift.Fail(e); }
		ms = lift.Ms();
	}

	// 3. REMOVE: the stored pieces' rectangle without them, through cvx_world_edit's machinery (cvxi::ColumnEdit)
	if (op == CVX_LIFT_REMOVE && stored.pieces) {
		NodeArgs &P = A.P;
		int64_t x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
		for (int64_t k = 0; k < stored.pieces; k++) {
			const cvx_piece &p = R.list[(size_t)k];
			x0 = std::min<int64_t>(x0, p.min[0]);
			x1 = std::max<int64_t>(x1, p.max[0]);
			z0 = std::min<int64_t>(z0, p.min[2]);
			z1 = std::max<int64_t>(z1, p.max[2]);
		}
		cvxi::EditRectangle E;
		rc = cvxi::RoundEditRectangle(ctx, x0, x1, z0, z1, levelCount, "a lift over", &E);
		if (rc != CVX_OK) { return rc; }
		P.rx0 = E.x0;
		P.rz0 = E.z0;
		P.rSizeZ = E.sizeZ;
		P.rn = E.n;
		cvxpieces::Totals totalsBack{};
		const cvxi::ColumnEditTotals totals{ P.totals, &totalsBack, sizeof totalsBack, offsetof(cvxpieces::Totals, head.elements), offsetof(cvxpieces::Totals, head.overLimit) };
		cvxi::ColumnEditCall edit{ call, CVX_ERR_CAPACITY, "a column without its lifted runs", "the columns of the lift" };
		edit.totals = &totals;
		edit.done = R.device.Event(1);
		rc = cvxi::ColumnEdit(
			ctx, E, levelCount, edit,
			[&](const cvxi::ColumnEditJob &J) {
				P.counts = J.counts;
				hipLaunchKernelGGL(lift_mark_kernel, dim3(Grid(nodes)), dim3(kThreads), 0, ctx->stream, A);
				hipLaunchKernelGGL(lift_remove_count_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			[&](const cvxi::ColumnEditJob &J) {
				P.headers = J.headers;
				P.elements = J.elements;
				hipLaunchKernelGGL(lift_remove_write_kernel, dim3(Grid((size_t)E.n)), dim3(kThreads), 0, ctx->stream, A);
				return hipSuccess;
			},
			nullptr);
		if (rc != CVX_OK) { return rc; }
		ms = R.device.Ms();
	}
	// (nothing is handed out before the call can no longer fail)
	for (size_t k = 0; k < listed; k++) {
		cvx_lifted_piece out{};
		out.piece = R.list[k];
		out.offset = offsets[k];
		for (int a = 0; a < 3; a++) { out.sum[a] = back[2 + 9 * k + a]; }
		for (int a = 0; a < 6; a++) { out.moment[a] = back[2 + 9 * k + 3 + a]; }
		pieces[k] = out;
	}
	if (summary) {
		cvx_lift_summary s{};
		s.pieces = R.host.summary;
		s.storedPieces = stored.pieces;
		s.storedVoxels = stored.voxels;
		s.neededVoxels = (int64_t)back[0];
		*summary = s;
	}
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // namespace cvxlift

extern "C" {

int cvx_world_lift_pieces(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount, cvx_lifted_piece *pieces,
                          int pieceCapacity, uint32_t *argb, uint8_t *solid, int64_t voxelCapacity, cvx_lift_summary *summary, float *outDeviceMs)
{
	return cvxlift::Lift(ctx, "cvx_world_lift_pieces", false, boxMin, boxMax, anchors, op, levelCount, pieces, pieceCapacity, argb, solid, voxelCapacity, summary, outDeviceMs);
}

int cvx_world_lift_pieces_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount, cvx_lifted_piece *pieces,
                                 int pieceCapacity, uint32_t *argbDevice, uint8_t *solidDevice, int64_t voxelCapacity, cvx_lift_summary *summary, float *outDeviceMs)
{
	return cvxlift::Lift(ctx, "cvx_world_lift_pieces_device", true, boxMin, boxMax, anchors, op, levelCount, pieces, pieceCapacity, argbDevice, solidDevice, voxelCapacity, summary,
	                     outDeviceMs);
}

int cvx_lifted_piece_mass(const cvx_lifted_piece *p, double centre[3], double inertia[6])
{
	if (!p || p->piece.voxels <= 0) { return Fail(nullptr, CVX_ERR_INVALID_ARGUMENT, "cvx_lifted_piece_mass: %s", p ? "the piece has no voxels" : "p is NULL"); }
	cvxb::LiftMass(*p, centre, inertia);
	return CVX_OK;
}

} // extern "C"
