// Host build of the brush shapes' rules (cpuvox_amd/csrc/cvx_brush.h) for tests/test_world_shapes_cpu.py.
//   shape_rules spans <cases in> <results out>      (int32 words)
//     Per case: dimY x0 x1 z0 z1, then one stroke (op shape a0 a1 a2 b0 b1 b2 argb pad).  Out: cvxb::StrokeSpan's lo hi for every column of
//     [x0, x1) x [z0, z1), x-major.
//   shape_rules points <cases in> <results out>     (int64 words; strokes at the limits, where there is no grid)
//     Per case: dimY, the stroke's ten fields, columnCount, (cx cz)*.  Out: lo hi per column.
//   shape_rules cull <case in>                      (int32 words)
//     dimY x0 z0 sizeX sizeZ stride strokeCount stroke* and per column of the rectangle (blob order) the column's words (tests/rules_world.h).
//     For every strip of 64 columns the stroke list is culled as the kernels cull it (cvxb::StripBox, 64 strokes at a time through
//     cvxb::StrokeMeetsStrip, survivors appended in order); every column then goes through cvxb::BrushColumn over the whole list and
//     cvxb::BrushColumnOver over the strip's list.  Prints: columns strips wrappedStrips listed mismatches.
//   shape_rules args
//     cvx_world_brush's argument checks on a context that never touched a device: one return code per call.
//   -DSHAPE_RULES_NO_LIBRARY (the sanitizer build) leaves `args` out: the rest calls nothing of the library, so nothing of it is linked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_brush.h"
#include "rules_world.h"

template <class T>
static cvx_brush_stroke Stroke(const T *p)
{
	cvx_brush_stroke s;
	s.op = (int32_t)p[0];
	s.shape = (int32_t)p[1];
	for (int a = 0; a < 3; a++) {
		s.a[a] = (int32_t)p[2 + a];
		s.b[a] = (int32_t)p[5 + a];
	}
	s.argb = (uint32_t)p[8];
	s.pad_ = (int32_t)p[9];
	return s;
}

static int Spans(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data()), *end = p + bytes.size() / 4;
	std::vector<int32_t> out;
	while (p < end) {
		const int dimY = p[0], x0 = p[1], x1 = p[2], z0 = p[3], z1 = p[4];
		const cvx_brush_stroke s = Stroke(p + 5);
		p += 15;
		for (int x = x0; x < x1; x++) {
			for (int z = z0; z < z1; z++) {
				int64_t lo, hi;
				cvxb::StrokeSpan(s, x, z, dimY, &lo, &hi);
				out.push_back((int32_t)lo);
				out.push_back((int32_t)hi);
			}
		}
	}
	return WriteFile(outPath, out);
}

static int Points(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int64_t *p = reinterpret_cast<const int64_t *>(bytes.data()), *end = p + bytes.size() / 8;
	std::vector<int64_t> out;
	while (p < end) {
		const int64_t dimY = p[0];
		const cvx_brush_stroke s = Stroke(p + 1);
		const int64_t count = p[11];
		p += 12;
		for (int64_t k = 0; k < count; k++, p += 2) {
			int64_t lo, hi;
			cvxb::StrokeSpan(s, p[0], p[1], dimY, &lo, &hi);
			out.push_back(lo);
			out.push_back(hi);
		}
	}
	return WriteFile(outPath, out);
}

// One arena column of the rectangle: its record and its own run list (tests/rules_world.h); the colour slots are shared
struct HostColumn {
	std::vector<uint32_t> runs = std::vector<uint32_t>(8, 0u);
	uint4 rec{ 0u, 0u, 0u, 0u };
	cvxb::ArenaColumn Column() const { return cvxb::ArenaColumn{ rec.x, rec.y, rec.z, rec.w, runs.data() }; }
};

static int Cull(const char *in)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int dimY = p[0], x0 = p[1], z0 = p[2], sizeX = p[3], sizeZ = p[4], stride = p[5], strokeCount = p[6];
	p += 7;
	std::vector<cvx_brush_stroke> strokes;
	for (int s = 0; s < strokeCount; s++, p += 10) { strokes.push_back(Stroke(p)); }
	const int n = sizeX * sizeZ;
	std::vector<HostColumn> columns((size_t)n);
	std::vector<uint32_t> slots;
	for (HostColumn &col : columns) { p = ReadCaseColumn(p, dimY, stride, &col.runs, &slots, &col.rec); }
	const int colorShift = CaseColorShift(stride);
	long long strips = 0, wrapped = 0, listed = 0, mismatches = 0;
	std::vector<uint16_t> list((size_t)strokeCount + 1);
	std::vector<uint32_t> runsA((size_t)dimY + 2), runsB((size_t)dimY + 2), coloursA((size_t)dimY + 2), coloursB((size_t)dimY + 2);
	for (int first = 0; first < n; first += 64, strips++) {
		const int last = (first + 64 < n ? first + 64 : n) - 1;
		int64_t bx0, bx1, bz0, bz1;
		cvxb::StripBox(first, last, x0, z0, sizeZ, &bx0, &bx1, &bz0, &bz1);
		wrapped += first / sizeZ != last / sizeZ;
		int count = 0;
		for (int base = 0; base < strokeCount; base += 64) { // the ballot step: the kept lanes in lane order behind what is listed
			for (int lane = 0; lane < 64 && base + lane < strokeCount; lane++) {
				if (cvxb::StrokeMeetsStrip(strokes[(size_t)(base + lane)], bx0, bx1, bz0, bz1)) { list[(size_t)count++] = (uint16_t)(base + lane); }
			}
		}
		listed += count;
		const cvxb::ListedStrokes some{ strokes.data(), list.data() };
		for (int i = first; i <= last; i++) {
			const int cx = x0 + i / sizeZ, cz = z0 + i % sizeZ;
			const cvxb::ArenaColumn col = columns[(size_t)i].Column();
			const cvxb::BrushResult a = cvxb::BrushColumn(col, slots.data(), colorShift, strokes.data(), strokeCount, cx, cz, dimY, runsA.data(), coloursA.data());
			const cvxb::BrushResult b = cvxb::BrushColumnOver(col, slots.data(), colorShift, some, count, cx, cz, dimY, runsB.data(), coloursB.data());
			const bool same = a.runCount == b.runCount && a.colours == b.colours && a.worldMin == b.worldMin && a.worldMax == b.worldMax && a.overLimit == b.overLimit &&
			                  std::memcmp(runsA.data(), runsB.data(), 4 * (size_t)a.runCount) == 0 && std::memcmp(coloursA.data(), coloursB.data(), 4 * (size_t)a.colours) == 0;
			mismatches += !same;
		}
	}
	std::printf("%d %lld %lld %lld %lld\n", n, strips, wrapped, listed, mismatches);
	return 0;
}

#ifndef SHAPE_RULES_NO_LIBRARY
static int Args()
{
	cvx_context *ctx = new cvx_context();
	const cvx_brush_stroke capsule{ CVX_BRUSH_CARVE, CVX_SHAPE_CAPSULE, { 1 << 30, -(1 << 30), 5 }, { (1 << 30) - 8191, -(1 << 30) + 8191, 5 }, 0u, 8191 };
	const cvx_brush_stroke ellipsoid{ CVX_BRUSH_FILL, CVX_SHAPE_ELLIPSOID, { 3, 4, 5 }, { 1, 1024, 7 }, 0u, -77 };
	std::vector<cvx_brush_stroke> list;
	list.push_back(capsule);   // valid: -3, no world
	list.push_back(ellipsoid); // valid (pad_ is ignored)
	cvx_brush_stroke s = capsule;
	s.pad_ = -1;
	list.push_back(s);
	s = capsule;
	s.pad_ = 8192;
	list.push_back(s);
	for (int a = 0; a < 3; a++) {
		s = capsule;
		s.a[a] = 0;
		s.b[a] = 8192;
		list.push_back(s);
		s.b[a] = -8192;
		list.push_back(s);
		s = capsule;
		s.a[a] = (1 << 30) + 1;
		s.b[a] = s.a[a];
		list.push_back(s);
		s.a[a] = -(1 << 30) - 1;
		s.b[a] = s.a[a];
		list.push_back(s);
		s = ellipsoid;
		s.b[a] = 0;
		list.push_back(s);
		s.b[a] = 1025;
		list.push_back(s);
		s.b[a] = -3;
		list.push_back(s);
	}
	for (const cvx_brush_stroke &k : list) { std::printf("%d ", cvx_world_brush(ctx, &k, 1, 0, nullptr)); }
	std::printf("| ");
	for (int shape = 2; shape < 16; shape++) {
		s = ellipsoid;
		s.shape = shape;
		std::printf("%d ", cvx_world_brush(ctx, &s, 1, 0, nullptr));
	}
	// ... and as the last stroke of an otherwise valid list: the message names it
	cvx_brush_stroke three[3] = { capsule, ellipsoid, capsule };
	three[2].pad_ = 9000;
	std::printf("| %d %s\n", cvx_world_brush(ctx, three, 3, 0, nullptr), ctx->error.c_str());
	return 0;
}
#endif

int main(int argc, char **argv)
{
#ifndef SHAPE_RULES_NO_LIBRARY
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
#endif
	if (argc == 4 && std::strcmp(argv[1], "spans") == 0) { return Spans(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "points") == 0) { return Points(argv[2], argv[3]); }
	if (argc == 3 && std::strcmp(argv[1], "cull") == 0) { return Cull(argv[2]); }
	std::fprintf(stderr, "usage: shape_rules spans <in> <out> | points <in> <out> | cull <in> | args\n");
	return 2;
}
