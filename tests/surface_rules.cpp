// Host build of the rule of cvx_world_surface (cpuvox_amd/csrc/cvx_surface.h) for tests/test_world_surface_cpu.py and tools/surface_bench.py,
// driven as cvx_surface.hip drives it: a count pass over the (column, face) pairs, a prefix sum, a write pass.
//   surface_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then boxMin[3] boxMax[3] solidOutside flags.  Out per case: the
//     cvx_surface_summary (64 bytes) and every quad (24 bytes each).
//   surface_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <x0> <y0> <z0> <x1> <y1> <z1> <solidOutside> <flags> <out>
//     Uploads the LOD-0 blob into a context that never touches a device, walks the box and writes the summary and every quad.  Prints the
//     layout and the milliseconds of the walk alone (tools/surface_bench.py: the host route).
//   surface_rules args
//     The argument checks of the two world calls on a context without a device: one return code per call.
//   surface_rules colours <argb>...
//     Per colour word: the word cvx_world_stamp_mesh's colour rule (cvx_stamp.h, TriangleColour) makes of the vertex colour
//     cvx_surface_triangles gives a quad of that word.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_stamp.h"
#include "cvx_surface.h"
#include "rules_world.h"

struct CountSink {
	uint32_t quads;
	int64_t unitFaces;
	void operator()(const cvx_surface_quad &q)
	{
		quads++;
		unitFaces += q.length;
	}
};

struct StoreSink {
	cvx_surface_quad *quads;
	uint32_t at, end;
	void operator()(const cvx_surface_quad &q)
	{
		if (at >= end) { std::exit(5); } // the write pass found more than the count pass
		quads[at++] = q;
	}
};

// summary + quads, appended to `out`
static void Walk(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int solidOutside, int flags, std::vector<uint8_t> &out)
{
	const int64_t pairs = B.Columns() * 6;
	const int sizeZ = B.SizeZ();
	std::vector<uint32_t> offsets((size_t)pairs + 1, 0u);
	cvx_surface_summary summary{};
	for (int64_t i = 0; i < pairs; i++) {
		const int64_t c = i / 6;
		CountSink sink{ 0u, 0 };
		cvxb::SurfaceWalk(W, B, B.x0 + c / sizeZ, B.z0 + c % sizeZ, (int)(i % 6), solidOutside, flags, sink);
		offsets[(size_t)i + 1] = offsets[(size_t)i] + sink.quads;
		summary.unitFaces += sink.unitFaces;
		summary.quadsPerFace[i % 6] += sink.quads;
	}
	summary.quads = offsets[(size_t)pairs];
	std::vector<cvx_surface_quad> quads((size_t)summary.quads + 1);
	for (int64_t i = 0; i < pairs; i++) {
		const int64_t c = i / 6;
		StoreSink sink{ quads.data(), offsets[(size_t)i], offsets[(size_t)i + 1] };
		cvxb::SurfaceWalk(W, B, B.x0 + c / sizeZ, B.z0 + c % sizeZ, (int)(i % 6), solidOutside, flags, sink);
		if (sink.at != sink.end) { std::exit(5); }
	}
	const uint8_t *s = reinterpret_cast<const uint8_t *>(&summary), *q = reinterpret_cast<const uint8_t *>(quads.data());
	out.insert(out.end(), s, s + sizeof summary);
	out.insert(out.end(), q, q + (size_t)summary.quads * sizeof(cvx_surface_quad));
}

static int Columns(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint8_t> out;
	while (p < end) {
		CaseWorld C;
		p = C.Read(p);
		const int dimY = C.dimY, gx = C.gx, gz = C.gz;
		int32_t boxMin[3], boxMax[3];
		for (int a = 0; a < 3; a++) { boxMin[a] = *p++; }
		for (int a = 0; a < 3; a++) { boxMax[a] = *p++; }
		const int solidOutside = *p++, flags = *p++;
		const cvxb::CopyWorld W = C.View();
		cvxb::PiecesBox B;
		if (!cvxb::PiecesClipBox(boxMin, boxMax, gx, dimY, gz, &B)) { return 4; }
		Walk(W, B, solidOutside, flags, out);
	}
	return WriteFile(outPath, out.data(), out.size());
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	int32_t boxMin[3], boxMax[3];
	for (int a = 0; a < 3; a++) {
		boxMin[a] = std::atoi(argv[7 + a]);
		boxMax[a] = std::atoi(argv[10 + a]);
	}
	const int solidOutside = std::atoi(argv[13]), flags = std::atoi(argv[14]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	std::vector<uint8_t> out;
	const auto t0 = std::chrono::steady_clock::now();
	Walk(W, B, solidOutside, flags, out);
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	std::printf("colorShift %d listed %lld ms %.3f\n", H.colorShift, (long long)H.listedColumns, ms);
	return WriteFile(argv[15], out.data(), out.size());
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_surface_quad list[2];
	cvx_surface_summary summary;
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 8, 8, 8 }, emptyY[3] = { 8, 0, 8 }, emptyX[3] = { -1, 8, 8 }, beyond[3] = { 100, 0, 0 }, beyondMax[3] = { 108, 8, 8 };
	std::vector<int> codes = {
		cvx_world_surface(nullptr, lo, hi, CVX_SURFACE_OUTSIDE_DEFAULT, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, nullptr, hi, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, nullptr, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, emptyY, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, emptyX, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, 0x40, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, -1, 0, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, 0, 2, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, 0, -1, list, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, 0, 0, list, -1, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, 0, 0, nullptr, 2, &summary, nullptr),
		cvx_world_surface_device(ctx, nullptr, hi, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface_device(ctx, lo, hi, 0x40, 0, list, 2, &summary, nullptr),
		cvx_world_surface_device(ctx, lo, hi, 0, 2, list, 2, &summary, nullptr),
		cvx_world_surface_device(ctx, lo, hi, 0, 0, list, -1, &summary, nullptr),
		cvx_world_surface_device(ctx, lo, hi, 0, 0, nullptr, 2, &summary, nullptr),
		cvx_world_surface(ctx, lo, hi, 0x3F, 1, nullptr, 0, nullptr, nullptr), // valid: no world yet
		cvx_world_surface_device(ctx, lo, hi, 0x3F, 1, nullptr, 0, nullptr, nullptr),
	};
	// an 8 x 8 x 8 world of empty columns on the host side of the context: a box wholly outside it is rejected before any device call
	std::vector<uint32_t> blob(3 * 64, 0u);
	if (cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size() * 4, 8, 8, 8, 64) != CVX_OK) { return 1; }
	codes.push_back(cvx_world_surface(ctx, beyond, beyondMax, 0, 0, list, 2, &summary, nullptr));
	codes.push_back(cvx_world_surface_device(ctx, beyond, beyondMax, 0, 0, list, 2, &summary, nullptr));
	// cvx_surface_triangles: no context at all
	cvx_surface_quad bad{ { 0, 0, 0 }, 6, 1, 0u };
	cvx_mesh_vertex vertices[4];
	int32_t indices[6];
	codes.push_back(cvx_surface_triangles(nullptr, -1, vertices, indices));
	codes.push_back(cvx_surface_triangles(nullptr, 1, vertices, indices));
	codes.push_back(cvx_surface_triangles(&bad, 1, nullptr, indices));
	codes.push_back(cvx_surface_triangles(&bad, 1, vertices, nullptr));
	codes.push_back(cvx_surface_triangles(&bad, 1, vertices, indices));
	codes.push_back(cvx_surface_triangles(nullptr, 0, nullptr, nullptr)); // valid
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

static int Colours(int argc, char **argv)
{
	for (int i = 2; i < argc; i++) {
		const cvx_surface_quad q{ { 1, 2, 3 }, 1, 4, (uint32_t)std::strtoul(argv[i], nullptr, 0) };
		cvx_mesh_vertex vertices[4];
		int32_t indices[6];
		if (cvx_surface_triangles(&q, 1, vertices, indices) != CVX_OK) { return 1; }
		uint32_t argb = 0u;
		if (!cvxs::TriangleColour(vertices[0], vertices[1], vertices[2], 0.25f, 0.25f, 0.5f, nullptr, 0, nullptr, &argb)) { return 1; }
		std::printf("%u ", argb);
	}
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc >= 2 && std::strcmp(argv[1], "colours") == 0) { return Colours(argc, argv); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 16 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: surface_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <box: 6> <solidOutside> <flags> <out> | args | colours <argb>...\n");
	return 2;
}
