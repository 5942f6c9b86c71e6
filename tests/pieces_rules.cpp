// Host build of the rules of cvx_world_pieces (cpuvox_amd/csrc/cvx_pieces.h) for tests/test_world_pieces_cpu.py, driven by a sequential
// union-find: per-column clipped runs, the edge rules, the anchor rules, the REMOVE column rule.
//   pieces_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then boxMin[3] boxMax[3] anchors.  Out per case (uint32 words):
//     floatingPieces floatingVoxels anchoredPieces anchoredVoxels, per floating piece min[3] max[3] seed[3] voxels, then for every column of
//     the world without the floating pieces: the edited-column block (tests/rules_world.h).
//   pieces_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <x0> <y0> <z0> <x1> <y1> <z1> <anchors> <levelCount> <list out> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device, analyses the box and writes the summary (32 bytes) and every floating
//     piece (48 bytes each), and the sub-world blob of the REMOVE rectangle as cvx_pieces.hip's write kernel makes it.  Prints the layout, the
//     rectangle, the node count and the milliseconds of the analysis alone (tools/pieces_bench.py: the host route).
//   pieces_rules args
//     cvx_world_pieces' argument checks on a context without a device or world: one return code per call.
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_pieces.h"
#include "rules_world.h"

struct Analysis {
	std::vector<uint32_t> offsets, lohi, floats; // per column + 1; per node lo, hi; per node: its piece floats
	std::vector<cvx_piece> floating;
	cvx_pieces_summary summary{ 0, 0, 0, 0 };
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

static Analysis Analyse(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int anchors)
{
	Analysis R;
	const int64_t n = B.Columns();
	const int sizeZ = B.SizeZ();
	R.offsets.assign((size_t)n + 1, 0u);
	for (int64_t c = 0; c < n; c++) {
		R.offsets[(size_t)c + 1] = R.offsets[(size_t)c] + cvxb::PiecesRunCount(cvxb::CopyColumnAt(W, B.x0 + c / sizeZ, B.z0 + c % sizeZ), B.y0, B.y1);
	}
	const uint32_t nodes = R.offsets[(size_t)n];
	R.lohi.assign(2 * (size_t)nodes + 2, 0u);
	std::vector<uint32_t> parent(nodes), column(nodes);
	for (int64_t c = 0; c < n; c++) {
		cvxb::PiecesClippedRuns(cvxb::CopyColumnAt(W, B.x0 + c / sizeZ, B.z0 + c % sizeZ), B.y0, B.y1, R.lohi.data() + 2 * (size_t)R.offsets[(size_t)c]);
		for (uint32_t j = R.offsets[(size_t)c]; j < R.offsets[(size_t)c + 1]; j++) {
			parent[j] = j;
			column[j] = (uint32_t)c;
		}
	}
	auto lo = [&](uint32_t j) { return R.lohi[2 * (size_t)j]; };
	auto hi = [&](uint32_t j) { return R.lohi[2 * (size_t)j + 1]; };
	for (uint32_t i = 0; i < nodes; i++) {
		const uint32_t c = column[i];
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
	for (uint32_t i = 0; i < nodes; i++) {
		for (int a = 0; a < 3; a++) {
			bounds[6 * (size_t)i + a] = INT_MAX;
			bounds[6 * (size_t)i + 3 + a] = INT_MIN;
		}
	}
	for (uint32_t i = 0; i < nodes; i++) {
		const uint32_t r = Find(parent, i);
		const int x = B.x0 + (int)(column[i] / sizeZ), z = B.z0 + (int)(column[i] % sizeZ);
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
	R.floats.assign((size_t)nodes + 1, 0u);
	for (uint32_t i = 0; i < nodes; i++) {
		if (parent[i] != i) { continue; }
		const bool anchored = bits[i] != 0 || ((anchors & CVX_ANCHOR_LARGEST) && largest == (int64_t)i);
		if (anchored) {
			R.summary.anchoredPieces++;
			R.summary.anchoredVoxels += voxels[i];
			continue;
		}
		R.summary.floatingPieces++;
		R.summary.floatingVoxels += voxels[i];
		cvx_piece p{};
		for (int a = 0; a < 3; a++) {
			p.min[a] = bounds[6 * (size_t)i + a];
			p.max[a] = bounds[6 * (size_t)i + 3 + a];
		}
		p.seed[0] = B.x0 + (int)(column[i] / sizeZ);
		p.seed[1] = (int)hi(i) - 1;
		p.seed[2] = B.z0 + (int)(column[i] % sizeZ);
		p.voxels = voxels[i];
		R.floating.push_back(p);
		R.floats[i] = 2u;
	}
	for (uint32_t i = 0; i < nodes; i++) { R.floats[i] = R.floats[Find(parent, i)] ? (R.floats[i] | 1u) : 0u; }
	for (uint32_t i = 0; i < nodes; i++) { R.floats[i] &= 1u; }
	return R;
}

// the nodes of column (cx, cz): none outside the box
static const uint32_t *ColumnNodes(const Analysis &R, const cvxb::PiecesBox &B, int64_t cx, int64_t cz, uint32_t *count)
{
	*count = 0u;
	if (!B.Holds(cx, cz)) { return nullptr; }
	const size_t c = (size_t)B.Column(cx, cz);
	*count = R.offsets[c + 1] - R.offsets[c];
	return R.floats.data() + R.offsets[c];
}

static int Columns(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		CaseWorld C;
		p = C.Read(p);
		const int dimY = C.dimY, gx = C.gx, gz = C.gz;
		int32_t boxMin[3], boxMax[3];
		for (int a = 0; a < 3; a++) { boxMin[a] = *p++; }
		for (int a = 0; a < 3; a++) { boxMax[a] = *p++; }
		const int anchors = *p++;
		const cvxb::CopyWorld W = C.View();
		cvxb::PiecesBox B;
		if (!cvxb::PiecesClipBox(boxMin, boxMax, gx, dimY, gz, &B)) { return 4; }
		const Analysis R = Analyse(W, B, anchors);
		out.push_back((uint32_t)R.summary.floatingPieces);
		out.push_back((uint32_t)R.summary.floatingVoxels);
		out.push_back((uint32_t)R.summary.anchoredPieces);
		out.push_back((uint32_t)R.summary.anchoredVoxels);
		for (const cvx_piece &piece : R.floating) {
			for (int a = 0; a < 3; a++) { out.push_back((uint32_t)piece.min[a]); }
			for (int a = 0; a < 3; a++) { out.push_back((uint32_t)piece.max[a]); }
			for (int a = 0; a < 3; a++) { out.push_back((uint32_t)piece.seed[a]); }
			out.push_back((uint32_t)piece.voxels);
		}
		for (int c = 0; c < gx * gz; c++) {
			const int64_t cx = c / gz, cz = c % gz;
			uint32_t nodes;
			const uint32_t *floats = ColumnNodes(R, B, cx, cz, &nodes);
			if (!AppendEditedColumn(&out, [&](uint32_t *runs, uint32_t *colours) { return cvxb::PiecesRemoveColumn(W, cx, cz, B.y0, B.y1, floats, nodes, runs, colours); })) { return 3; }
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	int32_t boxMin[3], boxMax[3];
	for (int a = 0; a < 3; a++) {
		boxMin[a] = std::atoi(argv[7 + a]);
		boxMax[a] = std::atoi(argv[10 + a]);
	}
	const int anchors = std::atoi(argv[13]), levelCount = std::atoi(argv[14]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	const auto t0 = std::chrono::steady_clock::now();
	const Analysis R = Analyse(W, B, anchors);
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	std::vector<uint8_t> list(sizeof R.summary + R.floating.size() * sizeof(cvx_piece));
	std::memcpy(list.data(), &R.summary, sizeof R.summary);
	if (!R.floating.empty()) { std::memcpy(list.data() + sizeof R.summary, R.floating.data(), R.floating.size() * sizeof(cvx_piece)); }
	if (WriteFile(argv[15], list.data(), list.size())) { return 2; }
	// the rectangle of a REMOVE, and its sub-world blob: count, scan, write
	int64_t x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	for (const cvx_piece &p : R.floating) {
		x0 = p.min[0] < x0 ? p.min[0] : x0;
		z0 = p.min[2] < z0 ? p.min[2] : z0;
		x1 = p.max[0] > x1 ? p.max[0] : x1;
		z1 = p.max[2] > z1 ? p.max[2] : z1;
	}
	std::vector<uint32_t> headers, pool;
	int over = 0, sizeX = 0, sizeZ = 0;
	if (!R.floating.empty()) {
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
			const uint32_t *floats = ColumnNodes(R, B, cx, cz, &nodes);
			const cvxb::BrushResult r = cvxb::PiecesRemoveColumn(W, cx, cz, B.y0, B.y1, floats, nodes, nullptr, nullptr);
			over |= r.overLimit ? 1 : 0;
			if (r.runCount == 0u) { continue; }
			const size_t off = pool.size();
			pool.resize(off + r.runCount + 2u + r.colours, 0u);
			cvxb::PiecesRemoveColumn(W, cx, cz, B.y0, B.y1, floats, nodes, pool.data() + off + 1, pool.data() + off + r.runCount + 2u);
			headers[3 * (size_t)i] = (uint32_t)off;
			headers[3 * (size_t)i + 1] = r.runCount | (r.worldMin << 16);
			headers[3 * (size_t)i + 2] = r.worldMax;
		}
		headers.insert(headers.end(), pool.begin(), pool.end());
	} else {
		x0 = z0 = 0;
	}
	std::printf("colorShift %d listed %lld over %d rect %lld %lld %d %d nodes %u ms %.3f\n", H.colorShift, (long long)H.listedColumns, over, (long long)x0, (long long)z0,
	            sizeX, sizeZ, R.offsets.back(), ms);
	return WriteFile(argv[16], headers.data(), headers.size() * 4);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 8, 8, 8 }, emptyHi[3] = { 8, 0, 8 };
	cvx_piece list[2];
	cvx_pieces_summary summary;
	const int codes[] = {
		cvx_world_pieces(nullptr, lo, hi, 0, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, nullptr, hi, 0, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, nullptr, 0, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, emptyHi, 0, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, hi, lo, 0, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 8, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, -1, CVX_PIECES_REPORT, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, 2, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, -1, 0, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, CVX_PIECES_REMOVE, -1, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, CVX_PIECES_REMOVE, 6, list, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, CVX_PIECES_REPORT, 0, list, -1, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, CVX_PIECES_REPORT, 0, nullptr, 2, &summary, nullptr),
		cvx_world_pieces(ctx, lo, hi, 7, CVX_PIECES_REMOVE, 5, nullptr, 0, nullptr, nullptr), // valid: no world yet
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 17 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: pieces_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <box: 6> <anchors> <levelCount> <list out> <blob out> | args\n");
	return 2;
}
