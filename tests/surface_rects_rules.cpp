// Host build of the rule of cvx_world_surface_rects (cpuvox_amd/csrc/cvx_surface_rects.h) for tests/test_world_surface_rects_cpu.py, driven as
// cvx_surface_rects.hip drives it: count the strips of the (column, face) pairs, prefix sum, list them, the first pass, the row pass, prefix
// sum, write.
//   surface_rects_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <x0> <y0> <z0> <x1> <y1> <z1> <solidOutside> <flags> <out>
//     Uploads the LOD-0 blob into a context that never touches a device, walks the box and writes the cvx_surface_rects_summary (72 bytes) and
//     every rectangle (32 bytes each).
//   surface_rects_rules args
//     The argument checks of the two world calls on a context without a device and those of cvx_surface_rect_triangles: one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_surface_rects.h"
#include "rules_world.h"
struct CountSink {
	uint32_t strips;
	int64_t unitFaces;
	void operator()(const cvx_surface_quad &q)
	{
		strips++;
		unitFaces += q.length;
	}
};

struct StoreSink {
	cvxb::RectStrip *strips;
	uint32_t at, end;
	void operator()(const cvx_surface_quad &q)
	{
		if (at >= end) { std::exit(5); } // the write pass found more than the count pass
		strips[at++] = cvxb::RectStrip{ q.voxel[1], q.length, q.argb };
	}
};

// summary + rectangles
static void Walk(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, int solidOutside, int flags, std::vector<uint8_t> &out)
{
	const int64_t pairs = B.Columns() * 6;
	const int sizeZ = B.SizeZ();
	cvx_surface_rects_summary summary{};
	std::vector<uint32_t> offsets((size_t)pairs + 1, 0u);
	for (int64_t i = 0; i < pairs; i++) {
		const int64_t c = i / 6;
		CountSink sink{ 0u, 0 };
		cvxb::SurfaceWalk(W, B, B.x0 + c / sizeZ, B.z0 + c % sizeZ, (int)(i % 6), solidOutside, flags, sink);
		offsets[(size_t)i + 1] = offsets[(size_t)i] + sink.strips;
		summary.unitFaces += sink.unitFaces;
	}
	summary.strips = offsets[(size_t)pairs];
	std::vector<cvxb::RectStrip> strips((size_t)summary.strips + 1);
	for (int64_t i = 0; i < pairs; i++) {
		const int64_t c = i / 6;
		StoreSink sink{ strips.data(), offsets[(size_t)i], offsets[(size_t)i + 1] };
		cvxb::SurfaceWalk(W, B, B.x0 + c / sizeZ, B.z0 + c % sizeZ, (int)(i % 6), solidOutside, flags, sink);
		if (sink.at != sink.end) { std::exit(5); }
	}
	// the passes: the first writes `along`, the row pass reads it and writes `rows`
	std::vector<uint32_t> along(strips.size(), ~0u), rows(strips.size(), ~0u), rectOffsets((size_t)pairs + 1, 0u);
	const bool ignoreColour = (flags & CVX_SURFACE_IGNORE_COLOUR) != 0;
	for (int pass = 0; pass < 2; pass++) {
		const cvxb::RectsPass P{ strips.data(), offsets.data(), pass ? along.data() : nullptr, ignoreColour };
		for (int64_t i = 0; i < pairs; i++) {
			const int face = (int)(i % 6);
			if (pass && !cvxb::RectsHasRowPass(face)) { continue; }
			const cvxb::RectsAxis axis = cvxb::RectsAxisOf(B, i / 6, pass || cvxb::RectsFirstPassAlongZ(face));
			const uint32_t firsts = cvxb::RectsMergePair(P, i, axis, pass ? rows.data() : along.data());
			if (pass || !cvxb::RectsHasRowPass(face)) { rectOffsets[(size_t)i + 1] = firsts; }
		}
	}
	for (int64_t i = 0; i < pairs; i++) {
		summary.rectsPerFace[i % 6] += rectOffsets[(size_t)i + 1];
		rectOffsets[(size_t)i + 1] += rectOffsets[(size_t)i];
	}
	summary.rects = rectOffsets[(size_t)pairs];
	std::vector<cvx_surface_rect> rects((size_t)summary.rects + 1);
	for (int64_t i = 0; i < pairs; i++) {
		const int64_t c = i / 6;
		const int face = (int)(i % 6);
		uint32_t at = rectOffsets[(size_t)i];
		for (uint32_t k = offsets[(size_t)i]; k < offsets[(size_t)i + 1]; k++) {
			const uint32_t r = cvxb::RectsHasRowPass(face) ? rows[k] : 1u;
			if (along[k] == ~0u || r == ~0u) { std::exit(6); } // a pass left a strip out
			if (along[k] == 0u || r == 0u) { continue; }
			if (at >= rectOffsets[(size_t)i + 1]) { std::exit(5); }
			rects[at++] = cvxb::RectOf(strips[k], (int32_t)(B.x0 + c / sizeZ), (int32_t)(B.z0 + c % sizeZ), face, along[k], r);
		}
		if (at != rectOffsets[(size_t)i + 1]) { std::exit(5); }
	}
	const uint8_t *s = reinterpret_cast<const uint8_t *>(&summary), *q = reinterpret_cast<const uint8_t *>(rects.data());
	out.insert(out.end(), s, s + sizeof summary);
	out.insert(out.end(), q, q + (size_t)summary.rects * sizeof(cvx_surface_rect));
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
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	std::vector<uint8_t> out;
	Walk(W, B, solidOutside, flags, out);
	return WriteFile(argv[15], out.data(), out.size());
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_surface_rect list[2];
	cvx_surface_rects_summary summary;
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 8, 8, 8 }, emptyY[3] = { 8, 0, 8 }, emptyX[3] = { -1, 8, 8 }, beyond[3] = { 100, 0, 0 }, beyondMax[3] = { 108, 8, 8 };
	std::vector<int> codes = {
		cvx_world_surface_rects(nullptr, lo, hi, CVX_SURFACE_OUTSIDE_DEFAULT, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, nullptr, hi, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, nullptr, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, emptyY, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, emptyX, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, 0x40, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, -1, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, 0, 2, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, 0, -1, list, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, 0, 0, list, -1, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, 0, 0, nullptr, 2, &summary, nullptr),
		cvx_world_surface_rects_device(ctx, nullptr, hi, 0, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects_device(ctx, lo, hi, 0x40, 0, list, 2, &summary, nullptr),
		cvx_world_surface_rects_device(ctx, lo, hi, 0, 2, list, 2, &summary, nullptr),
		cvx_world_surface_rects_device(ctx, lo, hi, 0, 0, list, -1, &summary, nullptr),
		cvx_world_surface_rects_device(ctx, lo, hi, 0, 0, nullptr, 2, &summary, nullptr),
		cvx_world_surface_rects(ctx, lo, hi, 0x3F, 1, nullptr, 0, nullptr, nullptr), // valid: no world yet
		cvx_world_surface_rects_device(ctx, lo, hi, 0x3F, 1, nullptr, 0, nullptr, nullptr),
	};
	// an 8 x 8 x 8 world of empty columns on the host side of the context: a box wholly outside it is rejected before any device call
	std::vector<uint32_t> blob(3 * 64, 0u);
	if (cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size() * 4, 8, 8, 8, 64) != CVX_OK) { return 1; }
	codes.push_back(cvx_world_surface_rects(ctx, beyond, beyondMax, 0, 0, list, 2, &summary, nullptr));
	codes.push_back(cvx_world_surface_rects_device(ctx, beyond, beyondMax, 0, 0, list, 2, &summary, nullptr));
	// cvx_surface_rect_triangles: no context at all
	const cvx_surface_rect good{ { 0, 0, 0 }, { 1, 4, 5 }, 1, 0u };
	cvx_surface_rect badFace = good, zeroSize = good, thick = good, thickTop = good;
	badFace.face = 6;
	zeroSize.size[2] = 0;
	thick.size[0] = 2;         // face 1: the normal axis is x
	thickTop.face = 3;         // face 3: the normal axis is y, where the size is 4
	cvx_mesh_vertex vertices[4];
	int32_t indices[6];
	codes.push_back(cvx_surface_rect_triangles(nullptr, -1, vertices, indices));
	codes.push_back(cvx_surface_rect_triangles(nullptr, 1, vertices, indices));
	codes.push_back(cvx_surface_rect_triangles(&good, 1, nullptr, indices));
	codes.push_back(cvx_surface_rect_triangles(&good, 1, vertices, nullptr));
	codes.push_back(cvx_surface_rect_triangles(&badFace, 1, vertices, indices));
	codes.push_back(cvx_surface_rect_triangles(&zeroSize, 1, vertices, indices));
	codes.push_back(cvx_surface_rect_triangles(&thick, 1, vertices, indices));
	codes.push_back(cvx_surface_rect_triangles(&thickTop, 1, vertices, indices));
	codes.push_back(cvx_surface_rect_triangles(&good, 1, vertices, indices));       // valid
	codes.push_back(cvx_surface_rect_triangles(nullptr, 0, nullptr, nullptr));      // valid
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 16 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: surface_rects_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <box: 6> <solidOutside> <flags> <out> | args\n");
	return 2;
}
