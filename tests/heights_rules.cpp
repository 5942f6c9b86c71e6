// Host build of the height-map rules (cpuvox_amd/csrc/cvx_heights.h) for tests/test_world_heights_cpu.py.
//   heights_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h) plus one write: boxMin[3] boxSize[3] op thickness flags hasArgb hasSide, the
//     heights and (if hasArgb / hasSide) the argb and sideArgb words, X * Z each.  Every column goes through cvxb::HeightsColumn -- the
//     function the kernels run, counting and then writing -- AND through cvxb::DenseColumn on the write expanded into dense arrays, the call's
//     definition; the two must agree word for word (exit code 3 otherwise).
//     Out per case and column: the edited-column block (tests/rules_world.h).
//   heights_rules read <blob> <dimX> <dimY> <dimZ> <columnCount> <minX> <minY> <minZ> <sizeX> <sizeY> <sizeZ> <out>
//     Uploads the LOD-0 blob into a context that never touches a device and runs cvxb::HeightsTop over the footprint in the arrays' order: the
//     heights, then the argb words, then the bottoms.
//   heights_rules args
//     The argument checks of the four calls on a context without a device or world: one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_dense.h"
#include "cvx_heights.h"
#include "rules_world.h"

// One write as the files hold it, and its expansion: the dense arrays of the cvx_world_write_voxels call that defines it.
struct HeightsWrite {
	cvxb::HeightsBox box;
	int op;
	std::vector<int32_t> heights;
	std::vector<uint32_t> argbWords, sideWords;
	cvxb::HeightsArrays arrays;
	cvxb::DenseBox dense;
	std::vector<uint32_t> denseArgb;
	std::vector<uint8_t> denseSolid;

	const int32_t *Parse(const int32_t *p)
	{
		int32_t min[3], size[3];
		for (int a = 0; a < 3; a++) { min[a] = *p++; }
		for (int a = 0; a < 3; a++) { size[a] = *p++; }
		box = cvxb::HeightsBox{ min[0], min[2], size[0], size[2], min[1], min[1] + size[1] };
		op = *p++;
		const int thickness = *p++, flags = *p++, hasArgb = *p++, hasSide = *p++;
		const size_t n = (size_t)size[0] * size[2];
		heights.assign(p, p + n);
		p += n;
		if (hasArgb) {
			argbWords.assign(reinterpret_cast<const uint32_t *>(p), reinterpret_cast<const uint32_t *>(p) + n);
			p += n;
		}
		if (hasSide) {
			sideWords.assign(reinterpret_cast<const uint32_t *>(p), reinterpret_cast<const uint32_t *>(p) + n);
			p += n;
		}
		arrays = cvxb::HeightsArrays{ heights.data(), hasArgb ? argbWords.data() : nullptr, hasSide ? sideWords.data() : nullptr, thickness, flags };
		// the expansion, a voxel at a time
		dense = cvxb::DenseBox{ { min[0], min[1], min[2] }, { size[0], size[1], size[2] } };
		denseArgb.assign(n * (size_t)size[1], 0u);
		denseSolid.assign(n * (size_t)size[1], 0);
		for (int64_t bx = 0; bx < size[0]; bx++) {
			for (int64_t bz = 0; bz < size[2]; bz++) {
				const cvxb::HeightsInterval s = cvxb::HeightsSpan(box, arrays, bx, bz);
				for (int64_t y = s.b; y < s.H; y++) {
					const size_t at = (size_t)((bx * size[2] + bz) * size[1] + (y - min[1]));
					denseSolid[at] = 1;
					denseArgb[at] = y == s.H - 1 ? s.top : s.side;
				}
			}
		}
		return p;
	}
};

static bool Same(const cvxb::BrushResult &a, const cvxb::BrushResult &b)
{
	return a.runCount == b.runCount && a.colours == b.colours && a.worldMin == b.worldMin && a.worldMax == b.worldMax && a.overLimit == b.overLimit;
}

// The column as the kernels make it (count, then write behind the counted runs) and as the definition makes it; false: they disagree.
static bool BothRules(const cvxb::ArenaColumn &col, const uint32_t *slots, int colorShift, const HeightsWrite &W, int64_t cx, int64_t cz, int dimY, cvxb::BrushResult *result,
                      std::vector<uint32_t> *runs, std::vector<uint32_t> *colours)
{
	const cvxb::BrushResult r = cvxb::HeightsColumn(col, slots, colorShift, W.box, W.arrays, W.op, cx, cz, dimY, nullptr, nullptr);
	const uint32_t *denseArgb = W.arrays.argb ? W.denseArgb.data() : nullptr;
	const cvxb::BrushResult d = cvxb::DenseColumn(col, slots, colorShift, W.dense, denseArgb, W.denseSolid.data(), W.op, cx, cz, dimY, nullptr, nullptr);
	*result = r;
	runs->assign(r.runCount + 1u, 0xDEADBEEFu);
	colours->assign(r.colours + 1u, 0xDEADBEEFu);
	if (!Same(r, d)) {
		std::fprintf(stderr, "column (%lld, %lld): %u runs %u colours [%u, %u) over %d, the dense rule's %u runs %u colours [%u, %u) over %d\n", (long long)cx, (long long)cz,
		             r.runCount, r.colours, r.worldMin, r.worldMax, (int)r.overLimit, d.runCount, d.colours, d.worldMin, d.worldMax, (int)d.overLimit);
		return false;
	}
	if (r.overLimit || r.runCount == 0u) { return true; }
	std::vector<uint32_t> denseRuns(*runs), denseColours(*colours);
	const cvxb::BrushResult again = cvxb::HeightsColumn(col, slots, colorShift, W.box, W.arrays, W.op, cx, cz, dimY, runs->data(), colours->data());
	cvxb::DenseColumn(col, slots, colorShift, W.dense, denseArgb, W.denseSolid.data(), W.op, cx, cz, dimY, denseRuns.data(), denseColours.data());
	if (!Same(r, again) || denseRuns != *runs || denseColours != *colours || runs->back() != 0xDEADBEEFu || colours->back() != 0xDEADBEEFu) {
		std::fprintf(stderr, "column (%lld, %lld): the runs or colours differ from the dense rule's\n", (long long)cx, (long long)cz);
		for (size_t k = 0; k < runs->size(); k++) { if ((*runs)[k] != denseRuns[k]) { std::fprintf(stderr, "  run %zu of %u: %08x, the dense rule's %08x\n", k, r.runCount, (*runs)[k], denseRuns[k]); } }
		for (size_t k = 0; k < colours->size(); k++) { if ((*colours)[k] != denseColours[k]) { std::fprintf(stderr, "  colour %zu of %u: %08x, the dense rule's %08x\n", k, r.colours, (*colours)[k], denseColours[k]); } }
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
		HeightsWrite W;
		p = W.Parse(p);
		const cvxb::CopyWorld world = C.View();
		for (int c = 0; c < gx * gz; c++) {
			const int64_t cx = c / gz, cz = c % gz;
			cvxb::BrushResult r;
			std::vector<uint32_t> newRuns, newColours;
			if (!BothRules(cvxb::CopyColumnAt(world, cx, cz), world.colourSlots, world.colorShift, W, cx, cz, dimY, &r, &newRuns, &newColours)) { return 3; }
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

static int Read(char **argv)
{
	const BlobWorld blob = LoadBlobWorld(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
	const cvxb::CopyWorld &W = blob.W;
	int32_t min[3], size[3];
	for (int a = 0; a < 3; a++) {
		min[a] = std::atoi(argv[7 + a]);
		size[a] = std::atoi(argv[10 + a]);
	}
	const cvxb::HeightsBox box{ min[0], min[2], size[0], size[2], min[1], min[1] + size[1] };
	const size_t n = (size_t)size[0] * size[2];
	std::vector<uint32_t> out(3 * n);
	for (int64_t x = 0; x < size[0]; x++) {
		for (int64_t z = 0; z < size[2]; z++) {
			const cvxb::HeightsRead r = cvxb::HeightsTop(W, box, min[0] + x, min[2] + z);
			const size_t i = (size_t)(x * size[2] + z);
			out[i] = (uint32_t)r.height;
			out[n + i] = r.argb;
			out[2 * n + i] = (uint32_t)r.bottom;
		}
	}
	return WriteFile(argv[13], out.data(), out.size() * 4);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 2, 2, 2 }, emptyHi[3] = { 2, 0, 2 }, emptyX[3] = { 0, 2, 2 }, farLo[3] = { -(1 << 30) - 1, 0, 0 }, farHi[3] = { 2, (1 << 30) + 1, 2 };
	const int32_t hugeLo[3] = { -(1 << 15), 0, -(1 << 15) }, hugeHi[3] = { 1 << 15, 1, 1 << 15 }; // 65536 * 65536 = 2^32 columns
	const int32_t wideLo[3] = { 0, 0, 0 }, wideHi[3] = { 1 << 16, 1, 1 << 15 };                  // 2^31 columns
	int32_t h[4] = {}, b[4] = {};
	uint32_t argb[4] = {};
	const int R = CVX_COPY_REPLACE;
	const int codes[] = {
		// reads
		cvx_world_read_heights(nullptr, lo, hi, h, argb, b, nullptr),
		cvx_world_read_heights(ctx, nullptr, hi, h, argb, b, nullptr), cvx_world_read_heights(ctx, lo, nullptr, h, argb, b, nullptr),
		cvx_world_read_heights(ctx, lo, emptyHi, h, argb, b, nullptr), cvx_world_read_heights(ctx, lo, emptyX, h, argb, b, nullptr),
		cvx_world_read_heights(ctx, farLo, hi, h, argb, b, nullptr), cvx_world_read_heights(ctx, lo, farHi, h, argb, b, nullptr),
		cvx_world_read_heights(ctx, hugeLo, hugeHi, h, argb, b, nullptr), cvx_world_read_heights(ctx, wideLo, wideHi, h, argb, b, nullptr),
		cvx_world_read_heights(ctx, lo, hi, nullptr, nullptr, nullptr, nullptr), cvx_world_read_heights_device(ctx, lo, hi, nullptr, nullptr, nullptr, nullptr),
		cvx_world_read_heights_device(ctx, lo, emptyHi, h, argb, b, nullptr),
		// writes
		cvx_world_write_heights(nullptr, lo, hi, h, argb, argb, 1, 0, R, 0, nullptr),
		cvx_world_write_heights(ctx, nullptr, hi, h, argb, argb, 1, 0, R, 0, nullptr), cvx_world_write_heights(ctx, lo, emptyHi, h, argb, argb, 1, 0, R, 0, nullptr),
		cvx_world_write_heights(ctx, farLo, hi, h, argb, argb, 1, 0, R, 0, nullptr), cvx_world_write_heights(ctx, wideLo, wideHi, h, argb, argb, 1, 0, R, 0, nullptr),
		cvx_world_write_heights(ctx, lo, hi, nullptr, argb, argb, 1, 0, R, 0, nullptr), cvx_world_write_heights(ctx, lo, hi, h, nullptr, argb, 1, 0, R, 0, nullptr),
		cvx_world_write_heights(ctx, lo, hi, h, nullptr, nullptr, 1, 0, CVX_BRUSH_FILL, 0, nullptr), cvx_world_write_heights(ctx, lo, hi, h, nullptr, nullptr, 1, 0, CVX_BRUSH_PAINT, 0, nullptr),
		cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, -1, 0, R, 0, nullptr), cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 32768, 0, R, 0, nullptr),
		cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 1, 2, R, 0, nullptr), cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 1, -1, R, 0, nullptr),
		cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 1, 0, 4, 0, nullptr), cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 1, 0, -1, 0, nullptr),
		cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 1, 0, R, 6, nullptr), cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 1, 0, R, -1, nullptr),
		cvx_world_write_heights_device(ctx, lo, hi, nullptr, argb, nullptr, 1, 0, R, 0, nullptr), cvx_world_write_heights_device(ctx, lo, hi, h, argb, nullptr, 1, 4, R, 0, nullptr),
		// valid: no world yet
		cvx_world_read_heights(ctx, lo, hi, h, nullptr, nullptr, nullptr), cvx_world_read_heights_device(ctx, lo, hi, nullptr, nullptr, b, nullptr),
		cvx_world_write_heights(ctx, lo, hi, h, argb, nullptr, 0, CVX_HEIGHTS_WALLED, R, 5, nullptr), cvx_world_write_heights(ctx, lo, hi, h, nullptr, nullptr, 32767, 0, CVX_BRUSH_CARVE, 0, nullptr),
		cvx_world_write_heights_device(ctx, lo, hi, h, argb, argb, 2, 0, CVX_BRUSH_PAINT, 3, nullptr),
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 14 && std::strcmp(argv[1], "read") == 0) { return Read(argv); }
	std::fprintf(stderr, "usage: heights_rules columns <in> <out> | read <blob> <dimX> <dimY> <dimZ> <columnCount> <min x y z> <size x y z> <out> | args\n");
	return 2;
}
