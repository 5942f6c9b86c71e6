// Host build of the brush and pick rules (cpuvox_amd/csrc/cvx_brush.h) for tests/test_world_brush_cpu.py.
//   brush_rules brush <cases in> <results out>
//     Each case is one column plus a stroke list (int32 words): dimY cx cz stride, the column's words (tests/rules_world.h), strokeCount
//     (op shape a0 a1 a2 b0 b1 b2 argb pad)*.  The column goes through cvxb::BrushColumn.  Out per case: the edited-column block
//     (tests/rules_world.h).
//   brush_rules pick <blob> <dimX> <dimY> <dimZ> <columnCount> <rays in> <hits out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host), then cvxb::PickRay on
//     every ray (cvx_pick_ray in, cvx_pick_hit out) against the host copy of the level, with a guard row of zeros around its records.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_brush.h"
#include "rules_world.h"

static int Brush(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		const int dimY = *p++, cx = *p++, cz = *p++, stride = *p++;
		CaseColumn C;
		p = C.Read(p, dimY, stride);
		const int strokeCount = *p++;
		std::vector<cvx_brush_stroke> strokes((size_t)strokeCount);
		std::memcpy(strokes.data(), p, (size_t)strokeCount * sizeof(cvx_brush_stroke));
		p += (size_t)strokeCount * sizeof(cvx_brush_stroke) / 4;
		const cvxb::ArenaColumn col = C.Column();
		const int colorShift = CaseColorShift(stride);
		if (!AppendEditedColumn(&out, [&](uint32_t *runs, uint32_t *colours) {
			    return cvxb::BrushColumn(col, C.slots.data(), colorShift, strokes.data(), strokeCount, cx, cz, dimY, runs, colours);
		    })) { return 3; }
	}
	return WriteFile(outPath, out);
}

static int Pick(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const std::vector<uint8_t> rayBytes = ReadFile(argv[7]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
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
	if (WriteFile(argv[8], hits)) { return 2; }
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
