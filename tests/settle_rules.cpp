// Host build of the rules of cvx_world_settle (cpuvox_amd/csrc/cvx_settle.h, on top of cvx_pieces.h) for tests/test_world_settle_cpu.py, driven
// sequentially: the union-find of tests/pieces_rules.cpp for the pieces, a Bellman-Ford over the node constraints (SettleBelow / SettleResolve)
// for the drops, SettleColumn for the columns.
//   settle_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <x0> <y0> <z0> <x1> <y1> <z1> <anchors> <maxDrop> <levelCount> <list out> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device, settles the box and writes the summary (40 bytes), every floating piece
//     (48 bytes each) and every drop (int32 each), and the sub-world blob of the settle's rectangle as cvx_settle.hip's write kernel makes it.
//     Prints the rectangle, the node count, the Bellman-Ford sweeps and the milliseconds of analysis + drops (tools/settle_bench.py: the host route).
//   settle_rules args
//     cvx_world_settle's argument checks on a context without a device or world: one return code per call.
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_settle.h"
#include "rules_world.h"
struct Settled {
	std::vector<uint32_t> offsets, lohi, column, root, shift; // per column + 1; per node: lo, hi; its column; its root; its piece's drop
	std::vector<int64_t> place;                               // per node: its piece's place in the list, -1: the piece is anchored
	std::vector<cvx_piece> floating;
	std::vector<int32_t> drops;
	cvx_settle_summary summary{ 0, 0, 0, 0, 0, 0 };
	int sweeps = 0;
};

static uint32_t Find(std::vector<uint32_t> &parent, uint32_t i)
{
	while (parent[i] != i) {
		parent[i] = parent[parent[i]];
		i = parent[i];
	}
	return i;
}

static void Unite(std::vector<uint32_t> &parent, uint32_t a, uint32_t b)
{
	a = Find(parent, a);
	b = Find(parent, b);
	if (a != b) { parent[a > b ? a : b] = a > b ? b : a; }
}

static Settled Settle(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int anchors, int maxDrop)
{
	Settled R;
	const int64_t n = B.Columns();
	const int sizeZ = B.SizeZ();
	auto columnAt = [&](uint32_t c) { return cvxb::CopyColumnAt(W, B.x0 + c / sizeZ, B.z0 + c % sizeZ); };
	R.offsets.assign((size_t)n + 1, 0u);
	for (int64_t c = 0; c < n; c++) { R.offsets[(size_t)c + 1] = R.offsets[(size_t)c] + cvxb::PiecesRunCount(columnAt((uint32_t)c), B.y0, B.y1); }
	const uint32_t nodes = R.offsets[(size_t)n];
	R.lohi.assign(2 * (size_t)nodes + 2, 0u);
	R.column.assign(nodes, 0u);
	std::vector<uint32_t> parent(nodes);
	for (int64_t c = 0; c < n; c++) {
		cvxb::PiecesClippedRuns(columnAt((uint32_t)c), B.y0, B.y1, R.lohi.data() + 2 * (size_t)R.offsets[(size_t)c]);
		for (uint32_t j = R.offsets[(size_t)c]; j < R.offsets[(size_t)c + 1]; j++) {
			parent[j] = j;
			R.column[j] = (uint32_t)c;
		}
	}
	auto lo = [&](uint32_t j) { return R.lohi[2 * (size_t)j]; };
	auto hi = [&](uint32_t j) { return R.lohi[2 * (size_t)j + 1]; };
	// the pieces: tests/pieces_rules.cpp
	for (uint32_t i = 0; i < nodes; i++) {
		const uint32_t c = R.column[i];
		if (i + 1 < R.offsets[c + 1] && cvxb::PiecesStacked(lo(i), hi(i + 1))) { Unite(parent, i, i + 1); }
		const int64_t beside[2] = { c / sizeZ + 1 < B.SizeX() ? (int64_t)c + sizeZ : -1, (int)(c % sizeZ) + 1 < sizeZ ? (int64_t)c + 1 : -1 };
		for (int64_t c2 : beside) {
			if (c2 < 0) { continue; }
			for (uint32_t j = R.offsets[(size_t)c2]; j < R.offsets[(size_t)c2 + 1]; j++) {
				if (cvxb::PiecesTouch(lo(i), hi(i), lo(j), hi(j))) { Unite(parent, i, j); }
			}
		}
	}
	std::vector<int64_t> voxels(nodes, 0);
	std::vector<int> bits(nodes, 0);
	std::vector<int32_t> bounds(6 * (size_t)nodes);
	R.root.assign(nodes, 0u);
	for (uint32_t i = 0; i < nodes; i++) {
		for (int a = 0; a < 3; a++) {
			bounds[6 * (size_t)i + a] = INT_MAX;
			bounds[6 * (size_t)i + 3 + a] = INT_MIN;
		}
	}
	for (uint32_t i = 0; i < nodes; i++) {
		const uint32_t r = R.root[i] = Find(parent, i);
		const int x = B.x0 + (int)(R.column[i] / sizeZ), z = B.z0 + (int)(R.column[i] % sizeZ);
		voxels[r] += hi(i) - lo(i);
		bits[r] |= cvxb::PiecesNodeAnchors(W, B, x, z, lo(i), hi(i)) & anchors;
		const int mn[3] = { x, (int)lo(i), z }, mx[3] = { x + 1, (int)hi(i), z + 1 };
		for (int a = 0; a < 3; a++) {
			if (mn[a] < bounds[6 * (size_t)r + a]) { bounds[6 * (size_t)r + a] = mn[a]; }
			if (mx[a] > bounds[6 * (size_t)r + 3 + a]) { bounds[6 * (size_t)r + 3 + a] = mx[a]; }
		}
	}
	int64_t largest = -1;
	for (uint32_t i = 0; i < nodes; i++) {
		if (parent[i] == i && (largest < 0 || voxels[i] > voxels[(size_t)largest])) { largest = i; }
	}
	std::vector<int64_t> placeOfRoot(nodes, -1);
	for (uint32_t i = 0; i < nodes; i++) {
		if (R.root[i] != i || bits[i] != 0 || ((anchors & CVX_ANCHOR_LARGEST) && largest == (int64_t)i)) { continue; }
		cvx_piece p{};
		for (int a = 0; a < 3; a++) {
			p.min[a] = bounds[6 * (size_t)i + a];
			p.max[a] = bounds[6 * (size_t)i + 3 + a];
		}
		p.seed[0] = B.x0 + (int)(R.column[i] / sizeZ);
		p.seed[1] = (int)hi(i) - 1;
		p.seed[2] = B.z0 + (int)(R.column[i] % sizeZ);
		p.voxels = voxels[i];
		placeOfRoot[i] = (int64_t)R.floating.size();
		R.floating.push_back(p);
		R.summary.floatingPieces++;
		R.summary.floatingVoxels += voxels[i];
	}
	R.place.assign(nodes, -1);
	for (uint32_t i = 0; i < nodes; i++) { R.place[i] = placeOfRoot[R.root[i]]; }
	// the drops: every piece starts at its floor bound (or maxDrop) and the constraints are swept until none lowers anything
	R.drops.assign(R.floating.size(), 0);
	for (size_t k = 0; k < R.floating.size(); k++) { R.drops[k] = maxDrop && maxDrop < R.floating[k].min[1] ? maxDrop : R.floating[k].min[1]; }
	for (bool changed = true; changed;) {
		changed = false;
		R.sweeps++;
		for (uint32_t i = 0; i < nodes; i++) {
			if (R.place[i] < 0) { continue; }
			const uint32_t c = R.column[i], j = i - R.offsets[c], count = R.offsets[c + 1] - R.offsets[c];
			const cvxb::SettleConstraint con = cvxb::SettleBelow(columnAt(c), B.y0, B.y1, j, count);
			const bool hasNode = con.kind == cvxb::SETTLE_NODE;
			const uint32_t kind = cvxb::SettleResolve(con.kind, R.root[i], hasNode ? R.root[i + 1] : 0u, hasNode && R.place[i + 1] >= 0);
			if (kind == cvxb::SETTLE_SELF) { continue; }
			const int64_t bound = (kind == cvxb::SETTLE_NODE ? (int64_t)R.drops[(size_t)R.place[i + 1]] : 0) + con.gap;
			if (bound < R.drops[(size_t)R.place[i]]) {
				R.drops[(size_t)R.place[i]] = (int32_t)bound;
				changed = true;
			}
		}
	}
	R.shift.assign((size_t)nodes + 1, 0u);
	for (uint32_t i = 0; i < nodes; i++) { R.shift[i] = R.place[i] < 0 ? 0u : (uint32_t)R.drops[(size_t)R.place[i]]; }
	for (size_t k = 0; k < R.floating.size(); k++) {
		if (R.drops[k] <= 0) { continue; }
		R.summary.fallenPieces++;
		R.summary.fallenVoxels += R.floating[k].voxels;
		if (R.drops[k] > R.summary.largestDrop) { R.summary.largestDrop = R.drops[k]; }
	}
	return R;
}

// the nodes of column (cx, cz): none outside the box
static const uint32_t *ColumnNodes(const Settled &R, const cvxb::PiecesBox &B, int64_t cx, int64_t cz, uint32_t *count)
{
	*count = 0u;
	if (!B.Holds(cx, cz)) { return nullptr; }
	const size_t c = (size_t)B.Column(cx, cz);
	*count = R.offsets[c + 1] - R.offsets[c];
	return R.shift.data() + R.offsets[c];
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	int32_t boxMin[3], boxMax[3];
	for (int a = 0; a < 3; a++) {
		boxMin[a] = std::atoi(argv[7 + a]);
		boxMax[a] = std::atoi(argv[10 + a]);
	}
	const int anchors = std::atoi(argv[13]), maxDrop = std::atoi(argv[14]), levelCount = std::atoi(argv[15]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	const auto t0 = std::chrono::steady_clock::now();
	const Settled R = Settle(W, B, anchors, maxDrop);
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	const size_t m = R.floating.size();
	std::vector<uint8_t> list(sizeof R.summary + m * sizeof(cvx_piece) + m * 4);
	std::memcpy(list.data(), &R.summary, sizeof R.summary);
	if (m) {
		std::memcpy(list.data() + sizeof R.summary, R.floating.data(), m * sizeof(cvx_piece));
		std::memcpy(list.data() + sizeof R.summary + m * sizeof(cvx_piece), R.drops.data(), m * 4);
	}
	if (WriteFile(argv[16], list.data(), list.size())) { return 2; }
	// the rectangle of the pieces that fall, and its sub-world blob: count, scan, write
	int64_t x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	for (size_t k = 0; k < m; k++) {
		if (R.drops[k] <= 0) { continue; }
		const cvx_piece &p = R.floating[k];
		x0 = p.min[0] < x0 ? p.min[0] : x0;
		z0 = p.min[2] < z0 ? p.min[2] : z0;
		x1 = p.max[0] > x1 ? p.max[0] : x1;
		z1 = p.max[2] > z1 ? p.max[2] : z1;
	}
	std::vector<uint32_t> headers, pool;
	int over = 0, sizeX = 0, sizeZ = 0;
	if (R.summary.fallenPieces) {
		const int64_t align = ((int64_t)1 << levelCount) - 1;
		x0 &= ~align;
		z0 &= ~align;
		x1 = (x1 + align) & ~align;
		z1 = (z1 + align) & ~align;
		x1 = x1 > dimX ? dimX : x1;
		z1 = z1 > dimZ ? dimZ : z1;
		sizeX = (int)(x1 - x0);
		sizeZ = (int)(z1 - z0);
		headers.assign(3 * (size_t)sizeX * sizeZ, 0u);
		for (int i = 0; i < sizeX * sizeZ; i++) {
			const int64_t cx = x0 + i / sizeZ, cz = z0 + i % sizeZ;
			uint32_t nodes;
			const uint32_t *shift = ColumnNodes(R, B, cx, cz, &nodes);
			const cvxb::BrushResult r = cvxb::SettleColumn(W, cx, cz, B.y0, B.y1, shift, nodes, nullptr, nullptr);
			over |= r.overLimit ? 1 : 0;
			if (r.runCount == 0u || r.overLimit) { continue; }
			const size_t off = pool.size();
			pool.resize(off + r.runCount + 2u + r.colours, 0u);
			const cvxb::BrushResult again = cvxb::SettleColumn(W, cx, cz, B.y0, B.y1, shift, nodes, pool.data() + off + 1, pool.data() + off + r.runCount + 2u);
			if (again.runCount != r.runCount || again.colours != r.colours) { return 3; }
			headers[3 * (size_t)i] = (uint32_t)off;
			headers[3 * (size_t)i + 1] = r.runCount | (r.worldMin << 16);
			headers[3 * (size_t)i + 2] = r.worldMax;
		}
		headers.insert(headers.end(), pool.begin(), pool.end());
	} else {
		x0 = z0 = 0;
	}
	std::printf("colorShift %d listed %lld over %d rect %lld %lld %d %d nodes %u sweeps %d ms %.3f\n", H.colorShift, (long long)H.listedColumns, over, (long long)x0,
	            (long long)z0, sizeX, sizeZ, R.offsets.back(), R.sweeps, ms);
	return WriteFile(argv[17], headers.data(), headers.size() * 4);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 8, 8, 8 }, emptyHi[3] = { 8, 0, 8 };
	cvx_piece list[2];
	int32_t drops[2];
	cvx_settle_summary summary;
	const int codes[] = {
		cvx_world_settle(nullptr, lo, hi, 0, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, nullptr, hi, 0, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, nullptr, 0, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, emptyHi, 0, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, hi, lo, 0, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 8, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, -1, 0, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 7, -1, 0, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 7, 0, -1, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 7, 0, 6, list, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 7, 0, 0, list, drops, -1, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 7, 0, 0, nullptr, drops, 2, &summary, nullptr),
		cvx_world_settle(ctx, lo, hi, 7, 3, 5, list, nullptr, 2, nullptr, nullptr),  // valid (drops may be NULL): no world yet
		cvx_world_settle(ctx, lo, hi, 7, 0, 5, nullptr, nullptr, 0, nullptr, nullptr), // valid: no world yet
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 18 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: settle_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <box: 6> <anchors> <maxDrop> <levelCount> <list out> <blob out> | args\n");
	return 2;
}
