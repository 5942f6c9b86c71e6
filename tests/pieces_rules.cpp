// Host build of the rules of cvx_world_pieces (cpuvox_amd/csrc/cvx_pieces.h) for tests/test_world_pieces_cpu.py, driven by a sequential
// union-find: per-column clipped runs, the edge rules, the anchor rules, the REMOVE column rule.
//   pieces_rules columns <cases in> <results out>
//     Each case is a small world of gx x gz columns in the reference's layout (int32 words, the format of tests/copy_rules.cpp): dimY gx gz stride,
//     per column (x-major) colorsBase runCount (colorsIndex length)* colourCount colour*, then boxMin[3] boxMax[3] anchors.  Out per case (uint32
//     words): floatingPieces floatingVoxels anchoredPieces anchoredVoxels, per floating piece min[3] max[3] seed[3] voxels, then for every column of
//     the world without the floating pieces: overLimit runCount colours worldMin worldMax and (unless over the limits) the runs and the colours.
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

#include "cvx_context.h"
#include "cvx_pieces.h"

static std::vector<uint8_t> ReadFile(const char *path)
{
	std::vector<uint8_t> out;
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::exit(2); }
	uint8_t buffer[65536];
	for (size_t n; (n = std::fread(buffer, 1, sizeof buffer, f)) > 0;) { out.insert(out.end(), buffer, buffer + n); }
	std::fclose(f);
	return out;
}

static int WriteFile(const char *path, const void *data, size_t bytes)
{
	FILE *f = std::fopen(path, "wb");
	if (!f) { return 2; }
	std::fwrite(data, 1, bytes, f);
	std::fclose(f);
	return 0;
}

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
		const int dimY = *p++, gx = *p++, gz = *p++, stride = *p++;
		int rowShift = 0;
		while ((1 << rowShift) < gz) { rowShift++; }
		std::vector<uint4> records((size_t)gx << rowShift, uint4{ 0u, 0u, 0u, 0u });
		std::vector<uint32_t> runs(8, 0u), slots(64, 0u);
		for (int c = 0; c < gx * gz; c++) {
			const int colorsBase = *p++, runCount = *p++;
			std::vector<uint32_t> elements(1, 0u);
			uint32_t start = 0;
			int64_t lowest = -1, highest = -1;
			for (int r = 0; r < runCount; r++) {
				const int32_t ci = *p++, length = *p++;
				elements.push_back(((uint32_t)ci & 0xFFFFu) | ((uint32_t)length << 16));
				if (ci >= 0) {
					const int64_t top = (int64_t)dimY - start;
					if (highest < 0) { highest = top; }
					lowest = top - length;
				}
				start += (uint32_t)length;
			}
			elements.push_back(0u);
			const int colourCount = *p++;
			if (slots.size() < (size_t)colorsBase + (size_t)stride * (colourCount + 1) + 64) { slots.resize((size_t)colorsBase + (size_t)stride * (colourCount + 1) + 64, 0u); }
			for (int k = 0; k < colourCount; k++) { slots[(size_t)colorsBase + (size_t)k * stride] = (uint32_t)*p++; }
			const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)(lowest < 0 ? 0 : lowest) << 16), (uint32_t)(highest < 0 ? 0 : highest) };
			uint4 rec{ 0u, 0u, 0u, 0u };
			if (runCount > 0 && highest >= 0) {
				const cvxe::ColumnWords w = cvxe::BuildColumnWords(header, elements.data(), 0, dimY);
				rec = uint4{ w.x | (uint32_t)colorsBase, w.y, w.z, w.w };
				if (w.code == 0u) {
					const size_t entry = runs.size() / 2;
					rec.z = (uint32_t)entry;
					runs.resize(runs.size() + 2u * w.solid + 8u, 0u);
					cvxe::BuildListedRuns(header, elements.data(), 0, dimY, runs.data() + 2 * entry);
				}
			}
			records[((size_t)(c / gz) << rowShift) + (size_t)(c % gz)] = rec;
		}
		int32_t boxMin[3], boxMax[3];
		for (int a = 0; a < 3; a++) { boxMin[a] = *p++; }
		for (int a = 0; a < 3; a++) { boxMax[a] = *p++; }
		const int anchors = *p++;
		cvxb::CopyWorld W;
		W.records = reinterpret_cast<const uint32_t *>(records.data());
		W.runs = runs.data();
		W.colourSlots = slots.data();
		W.rowShift = rowShift;
		W.colorShift = stride == 1 ? 2 : 7;
		W.dimX = gx;
		W.dimY = dimY;
		W.dimZ = gz;
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
			const cvxb::BrushResult r = cvxb::PiecesRemoveColumn(W, cx, cz, B.y0, B.y1, floats, nodes, nullptr, nullptr);
			out.push_back(r.overLimit ? 1u : 0u);
			out.push_back(r.runCount);
			out.push_back(r.colours);
			out.push_back(r.worldMin);
			out.push_back(r.worldMax);
			if (!r.overLimit) {
				std::vector<uint32_t> newRuns(r.runCount + 1u), newColours(r.colours + 1u);
				const cvxb::BrushResult again = cvxb::PiecesRemoveColumn(W, cx, cz, B.y0, B.y1, floats, nodes, newRuns.data(), newColours.data());
				if (again.runCount != r.runCount || again.colours != r.colours) { return 3; }
				out.insert(out.end(), newRuns.begin(), newRuns.begin() + r.runCount);
				out.insert(out.end(), newColours.begin(), newColours.begin() + r.colours);
			}
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int World(char **argv)
{
	std::vector<uint8_t> blob = ReadFile(argv[2]);
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	int32_t boxMin[3], boxMax[3];
	for (int a = 0; a < 3; a++) {
		boxMin[a] = std::atoi(argv[7 + a]);
		boxMax[a] = std::atoi(argv[10 + a]);
	}
	const int anchors = std::atoi(argv[13]), levelCount = std::atoi(argv[14]);
	cvx_context *ctx = new cvx_context();
	const int rc = cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size(), dimX, dimY, dimZ, columnCount);
	if (rc != CVX_OK) { std::printf("upload failed %d: %s\n", rc, ctx->error.c_str()); return 1; }
	const cvx_context::HostLevel &H = ctx->hostLevel[0];
	cvxb::CopyWorld W;
	W.records = reinterpret_cast<const uint32_t *>(H.records.data());
	W.runs = reinterpret_cast<const uint32_t *>(H.runs.data());
	W.colourSlots = H.elements.data();
	W.rowShift = H.rowShift;
	W.colorShift = H.colorShift;
	W.dimX = dimX;
	W.dimY = dimY;
	W.dimZ = dimZ;
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
