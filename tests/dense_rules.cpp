// Host build of the dense-box rules (cpuvox_amd/csrc/cvx_dense.h) for tests/test_world_dense_cpu.py.
//   dense_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h) plus one write: boxMin[3] boxSize[3] op hasArgb hasSolid, the argb words (if
//     hasArgb) and the mask, a word per voxel (if hasSolid).  Every column goes through cvxb::DenseColumn AND through the kernels' walk, 64
//     voxels per step (WaveColumn below: the steps of cvx_dense.h, lane after lane); the two must agree word for word (exit code 3 otherwise).
//     Out per case and column: the edited-column block (tests/rules_world.h).
//   dense_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <write> <x0> <z0> <sizeX> <sizeZ> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host), runs the kernels' walk
//     on every column of the rectangle (count, scan, write, as cvx_dense.hip does) and writes the sub-world blob; cvxb::DenseColumn must give the
//     same words.  <write>: boxMin[3] boxSize[3] op hasArgb hasSolid, argb words, mask words.
//   dense_rules read <blob> <dimX> <dimY> <dimZ> <columnCount> <minX> <minY> <minZ> <sizeX> <sizeY> <sizeZ> <out>
//     cvxb::DenseVoxel over the box in the arrays' order: the argb words, then the mask bytes.
//   dense_rules args
//     The argument checks of the four calls on a context without a device or world: one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_dense.h"
#include "rules_world.h"

// One write as the files hold it.
struct DenseWrite {
	cvxb::DenseBox box;
	int op;
	std::vector<uint32_t> argbWords;
	std::vector<uint8_t> solidBytes;
	const uint32_t *argb = nullptr;
	const uint8_t *solid = nullptr;

	const int32_t *Parse(const int32_t *p)
	{
		for (int a = 0; a < 3; a++) { box.min[a] = *p++; }
		for (int a = 0; a < 3; a++) { box.size[a] = *p++; }
		op = *p++;
		const int hasArgb = *p++, hasSolid = *p++;
		const size_t n = (size_t)box.size[0] * box.size[1] * box.size[2];
		if (hasArgb) {
			argbWords.assign(reinterpret_cast<const uint32_t *>(p), reinterpret_cast<const uint32_t *>(p) + n);
			p += n;
		}
		if (hasSolid) {
			solidBytes.resize(n);
			for (size_t k = 0; k < n; k++) { solidBytes[k] = (uint8_t)(*p++ != 0 ? 1 : 0); }
		}
		argb = hasArgb ? argbWords.data() : nullptr;
		solid = hasSolid ? solidBytes.data() : nullptr;
		return p;
	}
};

static uint32_t Below(uint64_t mask, int lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }

// cvx_dense.hip's WalkColumn with the wave's lanes run one after the other.
static cvxb::BrushResult WaveColumn(const cvxb::ArenaColumn &col, const uint32_t *slots, int colorShift, const DenseWrite &W, int64_t cx, int64_t cz, int dimY,
                                    uint32_t *outRuns, uint32_t *outColours)
{
	int64_t lo, hi, base;
	cvxb::DenseSpan(W.box, cx, cz, dimY, &lo, &hi, &base);
	const uint32_t count = col.Count();
	uint32_t cursor = 0u;
	cvxb::DenseWalk w;
	for (int yTop = dimY - 1; yTop >= 0; yTop -= 64) {
		const int air = cvxb::DenseAirSteps(col, count, &cursor, lo, hi, yTop);
		if (air > 0) {
			const int voxels = air * 64 < yTop + 1 ? air * 64 : yTop + 1;
			cvxb::DenseAdvanceAir(w, (uint32_t)voxels, outRuns);
			yTop -= (air - 1) * 64;
			continue;
		}
		const uint32_t valid = (uint32_t)(yTop + 1 < 64 ? yTop + 1 : 64);
		cvxb::Voxel v[64];
		uint64_t mask = 0;
		for (int lane = 0; lane < 64; lane++) {
			const int y = yTop - lane;
			v[lane] = cvxb::Voxel{ false, 0u };
			if (y >= 0) { v[lane] = cvxb::DenseFinal(col, slots, colorShift, lo <= y && y < hi, base + y, W.argb, W.solid, W.op, y); }
			if (v[lane].solid) { mask |= 1ull << lane; }
		}
		const uint64_t starts = cvxb::DenseStarts(w, mask, valid);
		if (outRuns) {
			for (int lane = 0; lane < 64; lane++) {
				cvxb::DenseLaneRun(w, mask, starts, lane, Below(starts, lane), Below(mask, lane), outRuns);
				if (v[lane].solid) { outColours[w.colours + Below(mask, lane)] = v[lane].argb; }
			}
		}
		cvxb::DenseAdvance(w, mask, starts, valid, yTop, outRuns);
	}
	return cvxb::DenseFinish(w, outRuns);
}

static bool Same(const cvxb::BrushResult &a, const cvxb::BrushResult &b)
{
	return a.runCount == b.runCount && a.colours == b.colours && a.worldMin == b.worldMin && a.worldMax == b.worldMax && a.overLimit == b.overLimit;
}

// Both walks of one column; false: they disagree.  The runs and colours are the scalar rule's.
static bool BothWalks(const cvxb::ArenaColumn &col, const uint32_t *slots, int colorShift, const DenseWrite &W, int64_t cx, int64_t cz, int dimY, cvxb::BrushResult *result,
                      std::vector<uint32_t> *runs, std::vector<uint32_t> *colours)
{
	const cvxb::BrushResult r = cvxb::DenseColumn(col, slots, colorShift, W.box, W.argb, W.solid, W.op, cx, cz, dimY, nullptr, nullptr);
	const cvxb::BrushResult counted = WaveColumn(col, slots, colorShift, W, cx, cz, dimY, nullptr, nullptr);
	*result = r;
	runs->assign(r.runCount + 1u, 0xDEADBEEFu);
	colours->assign(r.colours + 1u, 0xDEADBEEFu);
	if (!Same(r, counted)) { std::fprintf(stderr, "column (%lld, %lld): the wave's count differs from the rule's\n", (long long)cx, (long long)cz); return false; }
	if (r.overLimit || r.runCount == 0u) { return true; } // (an empty column is not walked again: the kernel writes its zero header and leaves)
	std::vector<uint32_t> waveRuns(*runs), waveColours(*colours);
	const cvxb::BrushResult again = cvxb::DenseColumn(col, slots, colorShift, W.box, W.argb, W.solid, W.op, cx, cz, dimY, runs->data(), colours->data());
	const cvxb::BrushResult written = WaveColumn(col, slots, colorShift, W, cx, cz, dimY, waveRuns.data(), waveColours.data());
	if (!Same(r, again) || !Same(r, written) || waveRuns != *runs || waveColours != *colours || runs->back() != 0xDEADBEEFu || colours->back() != 0xDEADBEEFu) {
		std::fprintf(stderr, "column (%lld, %lld): the wave's runs or colours differ from the rule's\n", (long long)cx, (long long)cz);
		for (size_t k = 0; k < runs->size(); k++) { if ((*runs)[k] != waveRuns[k]) { std::fprintf(stderr, "  run %zu of %u: %08x, the wave's %08x\n", k, r.runCount, (*runs)[k], waveRuns[k]); } }
		for (size_t k = 0; k < colours->size(); k++) { if ((*colours)[k] != waveColours[k]) { std::fprintf(stderr, "  colour %zu of %u: %08x, the wave's %08x\n", k, r.colours, (*colours)[k], waveColours[k]); } }
		return false;
	}
	return true;
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
		DenseWrite W;
		p = W.Parse(p);
		const cvxb::CopyWorld world = C.View();
		for (int c = 0; c < gx * gz; c++) {
			const int64_t cx = c / gz, cz = c % gz;
			cvxb::BrushResult r;
			std::vector<uint32_t> newRuns, newColours;
			if (!BothWalks(cvxb::CopyColumnAt(world, cx, cz), world.colourSlots, world.colorShift, W, cx, cz, dimY, &r, &newRuns, &newColours)) { return 3; }
			out.push_back(r.overLimit ? 1u : 0u);
			out.push_back(r.runCount);
			out.push_back(r.colours);
			out.push_back(r.worldMin);
			out.push_back(r.worldMax);
			if (!r.overLimit) {
				out.insert(out.end(), newRuns.begin(), newRuns.begin() + r.runCount);
				out.insert(out.end(), newColours.begin(), newColours.begin() + r.colours);
			}
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static BlobWorld Upload(char **argv) { return LoadBlobWorld(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])); }
static int World(char **argv)
{
	const BlobWorld blob = Upload(argv);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	const std::vector<uint8_t> writeBytes = ReadFile(argv[7]);
	DenseWrite D;
	D.Parse(reinterpret_cast<const int32_t *>(writeBytes.data()));
	const int x0 = std::atoi(argv[8]), z0 = std::atoi(argv[9]), sizeX = std::atoi(argv[10]), sizeZ = std::atoi(argv[11]);
	// count, scan, write: what dense_count_kernel, cvxi::ExclusiveScan and dense_write_kernel do
	const int columns = sizeX * sizeZ;
	std::vector<uint32_t> headers(3 * (size_t)columns, 0u), pool;
	int over = 0;
	for (int i = 0; i < columns; i++) {
		const int64_t cx = x0 + i / sizeZ, cz = z0 + i % sizeZ;
		const cvxb::ArenaColumn col = cvxb::CopyColumnAt(W, cx, cz);
		cvxb::BrushResult r;
		std::vector<uint32_t> runs, colours;
		if (!BothWalks(col, W.colourSlots, W.colorShift, D, cx, cz, W.dimY, &r, &runs, &colours)) { return 3; }
		over |= r.overLimit ? 1 : 0;
		if (r.runCount == 0u || r.overLimit) { continue; }
		const size_t off = pool.size();
		pool.resize(off + r.runCount + 2u + r.colours, 0u);
		WaveColumn(col, W.colourSlots, W.colorShift, D, cx, cz, W.dimY, pool.data() + off + 1, pool.data() + off + r.runCount + 2u);
		headers[3 * (size_t)i] = (uint32_t)off;
		headers[3 * (size_t)i + 1] = r.runCount | (r.worldMin << 16);
		headers[3 * (size_t)i + 2] = r.worldMax;
	}
	headers.insert(headers.end(), pool.begin(), pool.end());
	std::printf("colorShift %d listed %lld over %d\n", H.colorShift, (long long)H.listedColumns, over);
	return WriteFile(argv[12], headers.data(), headers.size() * 4);
}

static int Read(char **argv)
{
	const BlobWorld blob = Upload(argv);
	const cvxb::CopyWorld &W = blob.W;
	int64_t min[3], size[3];
	for (int a = 0; a < 3; a++) {
		min[a] = std::atoll(argv[7 + a]);
		size[a] = std::atoll(argv[10 + a]);
	}
	const size_t n = (size_t)(size[0] * size[1] * size[2]);
	std::vector<uint8_t> out(n * 5);
	uint32_t *argb = reinterpret_cast<uint32_t *>(out.data());
	uint8_t *solid = out.data() + n * 4;
	for (int64_t x = 0; x < size[0]; x++) {
		for (int64_t z = 0; z < size[2]; z++) {
			for (int64_t y = 0; y < size[1]; y++) {
				const cvxb::Voxel v = cvxb::DenseVoxel(W, min[0] + x, min[1] + y, min[2] + z);
				const size_t i = (size_t)((x * size[2] + z) * size[1] + y);
				argb[i] = v.argb;
				solid[i] = v.solid ? 1 : 0;
			}
		}
	}
	return WriteFile(argv[13], out.data(), out.size());
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 2, 2, 2 }, emptyHi[3] = { 2, 0, 2 }, farLo[3] = { -(1 << 30) - 1, 0, 0 }, farHi[3] = { 2, (1 << 30) + 1, 2 };
	const int32_t hugeLo[3] = { -1024, -1024, -1024 }, hugeHi[3] = { 1024, 1024, -512 }; // 2048 * 2048 * 512 = 2^31 voxels
	uint32_t argb[8] = {};
	uint8_t solid[8] = {};
	const int codes[] = {
		// reads
		cvx_world_read_voxels(nullptr, lo, hi, argb, solid, nullptr),
		cvx_world_read_voxels(ctx, nullptr, hi, argb, solid, nullptr), cvx_world_read_voxels(ctx, lo, nullptr, argb, solid, nullptr),
		cvx_world_read_voxels(ctx, lo, emptyHi, argb, solid, nullptr), cvx_world_read_voxels(ctx, farLo, hi, argb, solid, nullptr),
		cvx_world_read_voxels(ctx, lo, farHi, argb, solid, nullptr), cvx_world_read_voxels(ctx, hugeLo, hugeHi, argb, solid, nullptr),
		cvx_world_read_voxels(ctx, lo, hi, nullptr, nullptr, nullptr), cvx_world_read_voxels_device(ctx, lo, hi, nullptr, nullptr, nullptr),
		cvx_world_read_voxels_device(ctx, lo, emptyHi, argb, solid, nullptr),
		// writes
		cvx_world_write_voxels(nullptr, lo, hi, argb, solid, CVX_COPY_REPLACE, 0, nullptr),
		cvx_world_write_voxels(ctx, nullptr, hi, argb, solid, CVX_COPY_REPLACE, 0, nullptr), cvx_world_write_voxels(ctx, lo, emptyHi, argb, solid, CVX_COPY_REPLACE, 0, nullptr),
		cvx_world_write_voxels(ctx, farLo, hi, argb, solid, CVX_COPY_REPLACE, 0, nullptr), cvx_world_write_voxels(ctx, hugeLo, hugeHi, argb, solid, CVX_COPY_REPLACE, 0, nullptr),
		cvx_world_write_voxels(ctx, lo, hi, argb, solid, 4, 0, nullptr), cvx_world_write_voxels(ctx, lo, hi, argb, solid, -1, 0, nullptr),
		cvx_world_write_voxels(ctx, lo, hi, argb, solid, CVX_COPY_REPLACE, 6, nullptr), cvx_world_write_voxels(ctx, lo, hi, argb, solid, CVX_COPY_REPLACE, -1, nullptr),
		cvx_world_write_voxels(ctx, lo, hi, nullptr, solid, CVX_BRUSH_FILL, 0, nullptr), cvx_world_write_voxels(ctx, lo, hi, nullptr, nullptr, CVX_BRUSH_CARVE, 0, nullptr),
		cvx_world_write_voxels_device(ctx, lo, hi, nullptr, solid, CVX_COPY_REPLACE, 0, nullptr), cvx_world_write_voxels_device(ctx, lo, hi, argb, nullptr, 7, 0, nullptr),
		// valid: no world yet
		cvx_world_read_voxels(ctx, lo, hi, argb, nullptr, nullptr), cvx_world_read_voxels_device(ctx, lo, hi, nullptr, solid, nullptr),
		cvx_world_write_voxels(ctx, lo, hi, argb, nullptr, CVX_COPY_REPLACE, 5, nullptr), cvx_world_write_voxels(ctx, lo, hi, nullptr, solid, CVX_BRUSH_CARVE, 0, nullptr),
		cvx_world_write_voxels_device(ctx, lo, hi, argb, solid, CVX_BRUSH_PAINT, 3, nullptr),
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 13 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	if (argc == 14 && std::strcmp(argv[1], "read") == 0) { return Read(argv); }
	std::fprintf(stderr, "usage: dense_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <write> <x0> <z0> <sizeX> <sizeZ> <out> | "
	                     "read <blob> <dimX> <dimY> <dimZ> <columnCount> <min x y z> <size x y z> <out> | args\n");
	return 2;
}
