// Host build of the brush and pick rules (cpuvox_amd/csrc/cvx_brush.h) for tests/test_world_brush_cpu.py.
//   brush_rules brush <cases in> <results out>
//     Each case is one column in the reference's layout plus a stroke list (int32 words): dimY cx cz stride colorsBase runCount (colorsIndex length)*
//     colourCount colour* strokeCount (op shape a0 a1 a2 b0 b1 b2 argb pad)*.  The column gets its record from the edit's record rule (cvx_edit.h;
//     a listed column its run-list block at entry 2), its colours at colorsBase + k * stride, and goes through cvxb::BrushColumn.  Out per case:
//     overLimit runCount colours worldMin worldMax, then (unless over the limits) the runs and the colours.
//   brush_rules pick <blob> <dimX> <dimY> <dimZ> <columnCount> <rays in> <hits out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host), then cvxb::PickRay on
//     every ray (cvx_pick_ray in, cvx_pick_hit out) against the host copy of the level, with a guard row of zeros around its records.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_brush.h"
#include "cvx_context.h"

static std::vector<uint8_t> ReadFile(const char *path)
{
	std::vector<uint8_t> out;
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::exit(2); }
	for (int c; (c = std::fgetc(f)) != EOF;) { out.push_back((uint8_t)c); }
	std::fclose(f);
	return out;
}

static int Brush(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		const int dimY = *p++, cx = *p++, cz = *p++, stride = *p++, colorsBase = *p++, runCount = *p++;
		// the column as a blob: header {0, runCount | worldMin << 16, worldMax}, elements [guard][runs][guard][colours]
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
		std::vector<uint32_t> slots((size_t)colorsBase + (size_t)stride * (colourCount + 1) + 64, 0u);
		for (int k = 0; k < colourCount; k++) { slots[(size_t)colorsBase + (size_t)k * stride] = (uint32_t)*p++; }
		const int strokeCount = *p++;
		std::vector<cvx_brush_stroke> strokes((size_t)strokeCount);
		std::memcpy(strokes.data(), p, (size_t)strokeCount * sizeof(cvx_brush_stroke));
		p += (size_t)strokeCount * sizeof(cvx_brush_stroke) / 4;
		const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)(lowest < 0 ? 0 : lowest) << 16), (uint32_t)(highest < 0 ? 0 : highest) };
		uint32_t x = 0, y = 0, z = 0, w = 0;
		std::vector<uint32_t> runs(8, 0u);
		if (runCount > 0) {
			const cvxe::ColumnWords c = cvxe::BuildColumnWords(header, elements.data(), 0, dimY);
			x = c.x | (uint32_t)colorsBase;
			y = c.y;
			z = c.z;
			w = c.w;
			if (c.code == 0u) {
				z = 2u;
				runs.resize(2u * (2u + c.solid) + 8u, 0u);
				cvxe::BuildListedRuns(header, elements.data(), 0, dimY, runs.data() + 4);
			}
		}
		const cvxb::ArenaColumn col{ x, y, z, w, runs.data() };
		const int colorShift = stride == 1 ? 2 : 7;
		const cvxb::BrushResult r = cvxb::BrushColumn(col, slots.data(), colorShift, strokes.data(), strokeCount, cx, cz, dimY, nullptr, nullptr);
		out.push_back(r.overLimit ? 1u : 0u);
		out.push_back(r.runCount);
		out.push_back(r.colours);
		out.push_back(r.worldMin);
		out.push_back(r.worldMax);
		if (!r.overLimit) {
			std::vector<uint32_t> newRuns(r.runCount + 1u), newColours(r.colours + 1u);
			const cvxb::BrushResult again = cvxb::BrushColumn(col, slots.data(), colorShift, strokes.data(), strokeCount, cx, cz, dimY, newRuns.data(), newColours.data());
			if (again.runCount != r.runCount || again.colours != r.colours) { return 3; }
			out.insert(out.end(), newRuns.begin(), newRuns.begin() + r.runCount);
			out.insert(out.end(), newColours.begin(), newColours.begin() + r.colours);
		}
	}
	FILE *f = std::fopen(outPath, "wb");
	if (!f) { return 2; }
	std::fwrite(out.data(), 4, out.size(), f);
	std::fclose(f);
	return 0;
}

static int Pick(char **argv)
{
	std::vector<uint8_t> blob = ReadFile(argv[2]);
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const std::vector<uint8_t> rayBytes = ReadFile(argv[7]);
	cvx_context *ctx = new cvx_context();
	const int rc = cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size(), dimX, dimY, dimZ, columnCount);
	if (rc != CVX_OK) { std::printf("upload failed %d: %s\n", rc, ctx->error.c_str()); return 1; }
	const cvx_context::HostLevel &H = ctx->hostLevel[0];
	const size_t guard = ((size_t)1 << H.rowShift) + 4; // records
	std::vector<uint4> records(guard + H.records.size() + guard, uint4{ 0u, 0u, 0u, 0u });
	std::memcpy(records.data() + guard, H.records.data(), H.records.size() * sizeof(uint4));
	std::vector<uint2> runs(H.runs);
	runs.resize(runs.size() + 2, uint2{ 0u, 0u });
	cvxb::PickWorld W;
	W.records = reinterpret_cast<const uint32_t *>(records.data() + guard);
	W.runs = reinterpret_cast<const uint32_t *>(runs.data());
	W.colours = reinterpret_cast<const uint8_t *>(H.elements.data());
	W.rowShift = H.rowShift;
	W.colorShift = H.colorShift;
	W.dimX = dimX;
	W.dimY = dimY;
	W.dimZ = dimZ;
	const size_t n = rayBytes.size() / sizeof(cvx_pick_ray);
	const cvx_pick_ray *rays = reinterpret_cast<const cvx_pick_ray *>(rayBytes.data());
	std::vector<cvx_pick_hit> hits(n);
	for (size_t i = 0; i < n; i++) {
		const cvxb::PickResult r = cvxb::PickRay(W, rays[i].origin, rays[i].direction, rays[i].maxT);
		std::memcpy(hits[i].voxel, r.voxel, sizeof r.voxel);
		hits[i].face = r.face;
		hits[i].argb = r.argb;
		hits[i].t = r.t;
	}
	FILE *f = std::fopen(argv[8], "wb");
	if (!f) { return 2; }
	std::fwrite(hits.data(), sizeof(cvx_pick_hit), n, f);
	std::fclose(f);
	std::printf("colorShift %d listed %lld\n", H.colorShift, (long long)H.listedColumns);
	return 0;
}

// The argument checks of the two calls on a context that never touched a device (no world): prints one return code per call
static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_brush_stroke ok{ CVX_BRUSH_FILL, CVX_SHAPE_BOX, { 0, 0, 0 }, { 1, 1, 1 }, 0u, 0 };
	cvx_brush_stroke badOp = ok, badShape = ok, badRadius = ok;
	badOp.op = 3;
	badShape.shape = 2;
	badRadius.shape = CVX_SHAPE_SPHERE;
	badRadius.b[0] = -1;
	std::vector<cvx_brush_stroke> many(CVX_BRUSH_MAX_STROKES + 1, ok);
	cvx_pick_ray ray{ { 0.f, 0.f, 0.f }, { 1.f, 0.f, 0.f }, 1.f, 0.f };
	cvx_pick_hit hit;
	const int codes[] = {
		cvx_world_brush(ctx, &ok, 0, 0, nullptr), cvx_world_brush(ctx, nullptr, 1, 0, nullptr), cvx_world_brush(ctx, many.data(), (int)many.size(), 0, nullptr),
		cvx_world_brush(ctx, &ok, 1, -1, nullptr), cvx_world_brush(ctx, &ok, 1, 6, nullptr), cvx_world_brush(ctx, &badOp, 1, 0, nullptr),
		cvx_world_brush(ctx, &badShape, 1, 0, nullptr), cvx_world_brush(ctx, &badRadius, 1, 0, nullptr),
		cvx_world_brush(ctx, &ok, 1, 5, nullptr),  // valid: no world yet
		cvx_world_pick(ctx, -1, &ray, &hit), cvx_world_pick(ctx, 1, nullptr, &hit), cvx_world_pick(ctx, 1, &ray, &hit),
		cvx_world_pick_device(ctx, 1, nullptr, nullptr, nullptr),
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "brush") == 0) { return Brush(argv[2], argv[3]); }
	if (argc == 9 && std::strcmp(argv[1], "pick") == 0) { return Pick(argv); }
	std::fprintf(stderr, "usage: brush_rules brush <in> <out> | pick <blob> <dimX> <dimY> <dimZ> <columnCount> <rays> <hits>\n");
	return 2;
}
