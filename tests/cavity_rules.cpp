// Host build of the rules of cvx_world_cavities (cpuvox_amd/csrc/cvx_cavity.h) for tests/test_world_cavities_cpu.py, driven by a sequential
// union-find: per-column air intervals, the edge rule, the open bits, the FILL column rule.
//   cavity_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then boxMin[3] boxMax[3] openFaces maxVoxels argb.  Out per case (uint32
//     words): the six totals of cvx_cavities_summary, per selected cavity min[3] max[3] seed[3] voxels, then for every column of the world with
//     the selected cavities filled: the edited-column block (tests/rules_world.h).
//   cavity_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <x0> <y0> <z0> <x1> <y1> <z1> <openFaces> <maxVoxels> <argb> <levelCount> <list out> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device, analyses the box and writes the summary (48 bytes) and every selected
//     cavity (48 bytes each), and the sub-world blob of the FILL rectangle as cvx_cavity.hip's write kernel makes it.  Prints the layout, the
//     rectangle, the node count and the milliseconds of the analysis alone (tools/cavity_bench.py: the host route).
//   cavity_rules args
//     cvx_world_cavities' argument checks on a context without a device or world: one return code per call.
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_cavity.h"
#include "rules_world.h"

struct Analysis {
	std::vector<uint32_t> offsets, lohi, chosen; // per column + 1; per node lo, hi; per node: its cavity is selected
	std::vector<cvx_piece> selected;
	cvx_cavities_summary summary{ 0, 0, 0, 0, 0, 0 };
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

static Analysis Analyse(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int openFaces, int64_t maxVoxels)
{
	Analysis R;
	const int64_t n = B.Columns();
	const int sizeZ = B.SizeZ();
	R.offsets.assign((size_t)n + 1, 0u);
	for (int64_t c = 0; c < n; c++) {
		R.offsets[(size_t)c + 1] = R.offsets[(size_t)c] + cvxb::CavityNodeCount(cvxb::CopyColumnAt(W, B.x0 + c / sizeZ, B.z0 + c % sizeZ), B.y0, B.y1);
	}
	const uint32_t nodes = R.offsets[(size_t)n];
	R.lohi.assign(2 * (size_t)nodes + 2, 0u);
	std::vector<uint32_t> parent(nodes), column(nodes);
	for (int64_t c = 0; c < n; c++) {
		const uint32_t made = cvxb::CavityNodes(cvxb::CopyColumnAt(W, B.x0 + c / sizeZ, B.z0 + c % sizeZ), B.y0, B.y1, R.lohi.data() + 2 * (size_t)R.offsets[(size_t)c]);
		if (made != R.offsets[(size_t)c + 1] - R.offsets[(size_t)c]) { std::exit(5); }
		for (uint32_t j = R.offsets[(size_t)c]; j < R.offsets[(size_t)c + 1]; j++) {
			parent[j] = j;
			column[j] = (uint32_t)c;
		}
	}
	auto lo = [&](uint32_t j) { return R.lohi[2 * (size_t)j]; };
	auto hi = [&](uint32_t j) { return R.lohi[2 * (size_t)j + 1]; };
	for (uint32_t i = 0; i < nodes; i++) {
		const uint32_t c = column[i];
		const int64_t beside[2] = { (int)(c / sizeZ) + 1 < B.SizeX() ? (int64_t)c + sizeZ : -1, (int)(c % sizeZ) + 1 < sizeZ ? (int64_t)c + 1 : -1 };
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
		bits[r] |= cvxb::CavityNodeOpen(W, B, x, z, lo(i), hi(i)) & openFaces;
		const int mn[3] = { x, (int)lo(i), z }, mx[3] = { x + 1, (int)hi(i), z + 1 };
		for (int a = 0; a < 3; a++) {
			if (mn[a] < bounds[6 * (size_t)r + a]) { bounds[6 * (size_t)r + a] = mn[a]; }
			if (mx[a] > bounds[6 * (size_t)r + 3 + a]) { bounds[6 * (size_t)r + 3 + a] = mx[a]; }
		}
	}
	R.chosen.assign((size_t)nodes + 1, 0u);
	for (uint32_t i = 0; i < nodes; i++) {
		if (parent[i] != i) { continue; }
		if (bits[i] != 0) {
			R.summary.openRegions++;
			R.summary.openVoxels += voxels[i];
			continue;
		}
		R.summary.enclosedCavities++;
		R.summary.enclosedVoxels += voxels[i];
		if (maxVoxels != 0 && voxels[i] > maxVoxels) { continue; }
		R.summary.selectedCavities++;
		R.summary.selectedVoxels += voxels[i];
		cvx_piece p{};
		for (int a = 0; a < 3; a++) {
			p.min[a] = bounds[6 * (size_t)i + a];
			p.max[a] = bounds[6 * (size_t)i + 3 + a];
		}
		p.seed[0] = B.x0 + (int)(column[i] / sizeZ);
		p.seed[1] = (int)hi(i) - 1;
		p.seed[2] = B.z0 + (int)(column[i] % sizeZ);
		p.voxels = voxels[i];
		R.selected.push_back(p);
		R.chosen[i] = 2u;
	}
	for (uint32_t i = 0; i < nodes; i++) { R.chosen[i] = R.chosen[Find(parent, i)] ? (R.chosen[i] | 1u) : 0u; }
	for (uint32_t i = 0; i < nodes; i++) { R.chosen[i] &= 1u; }
	return R;
}

// the per-node flags of column (cx, cz): null outside the box
static const uint32_t *ColumnNodes(const Analysis &R, const cvxb::PiecesBox &B, int64_t cx, int64_t cz)
{
	return B.Holds(cx, cz) ? R.chosen.data() + R.offsets[(size_t)B.Column(cx, cz)] : nullptr;
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
		const int openFaces = *p++;
		const int64_t maxVoxels = *p++;
		const uint32_t argb = (uint32_t)*p++;
		const cvxb::CopyWorld W = C.View();
		cvxb::PiecesBox B;
		if (!cvxb::PiecesClipBox(boxMin, boxMax, gx, dimY, gz, &B)) { return 4; }
		const Analysis R = Analyse(W, B, openFaces, maxVoxels);
		const int64_t totals[6] = { R.summary.enclosedCavities, R.summary.enclosedVoxels, R.summary.selectedCavities, R.summary.selectedVoxels,
			                        R.summary.openRegions, R.summary.openVoxels };
		for (int64_t t : totals) { out.push_back((uint32_t)t); }
		for (const cvx_piece &piece : R.selected) {
			for (int a = 0; a < 3; a++) { out.push_back((uint32_t)piece.min[a]); }
			for (int a = 0; a < 3; a++) { out.push_back((uint32_t)piece.max[a]); }
			for (int a = 0; a < 3; a++) { out.push_back((uint32_t)piece.seed[a]); }
			out.push_back((uint32_t)piece.voxels);
		}
		for (int c = 0; c < gx * gz; c++) {
			const int64_t cx = c / gz, cz = c % gz;
			const uint32_t *chosen = ColumnNodes(R, B, cx, cz);
			if (!AppendEditedColumn(&out, [&](uint32_t *runs, uint32_t *colours) { return cvxb::CavityFillColumn(W, cx, cz, B.y0, B.y1, chosen, argb, runs, colours); })) { return 3; }
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
	const int openFaces = std::atoi(argv[13]), levelCount = std::atoi(argv[16]);
	const int64_t maxVoxels = std::atoll(argv[14]);
	const uint32_t argb = (uint32_t)std::strtoul(argv[15], nullptr, 0);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	const auto t0 = std::chrono::steady_clock::now();
	const Analysis R = Analyse(W, B, openFaces, maxVoxels);
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	std::vector<uint8_t> list(sizeof R.summary + R.selected.size() * sizeof(cvx_piece));
	std::memcpy(list.data(), &R.summary, sizeof R.summary);
	if (!R.selected.empty()) { std::memcpy(list.data() + sizeof R.summary, R.selected.data(), R.selected.size() * sizeof(cvx_piece)); }
	if (WriteFile(argv[17], list.data(), list.size())) { return 2; }
	// the rectangle of a FILL, and its sub-world blob: count, scan, write
	int64_t x0 = INT_MAX, x1 = INT_MIN, z0 = INT_MAX, z1 = INT_MIN;
	for (const cvx_piece &p : R.selected) {
		x0 = p.min[0] < x0 ? p.min[0] : x0;
		z0 = p.min[2] < z0 ? p.min[2] : z0;
		x1 = p.max[0] > x1 ? p.max[0] : x1;
		z1 = p.max[2] > z1 ? p.max[2] : z1;
	}
	std::vector<uint32_t> headers, pool;
	int over = 0, sizeX = 0, sizeZ = 0;
	if (!R.selected.empty()) {
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
			const uint32_t *chosen = ColumnNodes(R, B, cx, cz);
			const cvxb::BrushResult r = cvxb::CavityFillColumn(W, cx, cz, B.y0, B.y1, chosen, argb, nullptr, nullptr);
			over |= r.overLimit ? 1 : 0;
			if (r.runCount == 0u) { continue; }
			const size_t off = pool.size();
			pool.resize(off + r.runCount + 2u + r.colours, 0u);
			cvxb::CavityFillColumn(W, cx, cz, B.y0, B.y1, chosen, argb, pool.data() + off + 1, pool.data() + off + r.runCount + 2u);
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
	return WriteFile(argv[18], headers.data(), headers.size() * 4);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_piece list[2];
	cvx_cavities_summary summary;
	auto params = [](int x1, int y1, int openFaces, int op, int64_t maxVoxels) {
		cvx_cavity_params p{};
		p.boxMax[0] = x1;
		p.boxMax[1] = y1;
		p.boxMax[2] = 8;
		p.openFaces = openFaces;
		p.op = op;
		p.maxVoxels = maxVoxels;
		return p;
	};
	const cvx_cavity_params good = params(8, 8, CVX_CAVITY_OPEN_DEFAULT, CVX_CAVITIES_FILL, 0), emptyY = params(8, 0, 0, 0, 0), emptyX = params(-1, 8, 0, 0, 0),
	                        faces = params(8, 8, 0x40, 0, 0), negativeFaces = params(8, 8, -1, 0, 0), op = params(8, 8, 0, 2, 0), negativeOp = params(8, 8, 0, -1, 0),
	                        limit = params(8, 8, 0, 0, -1);
	const int codes[] = {
		cvx_world_cavities(nullptr, &good, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, nullptr, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &emptyY, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &emptyX, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &faces, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &negativeFaces, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &op, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &negativeOp, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &limit, 0, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &good, -1, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &good, 6, list, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &good, 0, list, -1, &summary, nullptr),
		cvx_world_cavities(ctx, &good, 0, nullptr, 2, &summary, nullptr),
		cvx_world_cavities(ctx, &good, 5, nullptr, 0, nullptr, nullptr), // valid: no world yet
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 19 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: cavity_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <box: 6> <openFaces> <maxVoxels> <argb> <levelCount> <list out> <blob out> | args\n");
	return 2;
}
