// Host build of the rules of cvx_world_light (cpuvox_amd/csrc/cvx_light.h) for tests/test_world_light_cpu.py, driven sequentially with every
// occupancy test answered from the records (cvxb::ArenaOcc).
//   light_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then the 16 words of cvx_light_params.  Out per case (uint32 words), for
//     every column of the world after the call: the edited-column block (tests/rules_world.h).
//   light_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <16 words of cvx_light_params> <levelCount> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device and writes the sub-world blob of the call's rectangle as cvx_light.hip
//     makes it.  Prints the layout, the rectangle, the voxels lit and the milliseconds of the lighting alone (tools/light_bench.py: the host route).
//   light_rules shade <dimX> <dimY> <dimZ> <16 words of cvx_light_params> <voxel count> (x y z)* -- <x y z>
//     The shade of voxel <x y z> in a world of the listed solid voxels (the constructed cases): prints sky, facing, den, lit, shade.
//   light_rules args
//     cvx_world_light's argument checks on a context without a device or world: one return code per call.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_light.h"
#include "rules_world.h"

static cvx_light_params Params(const int32_t *w)
{
	cvx_light_params P;
	std::memcpy(&P, w, sizeof P);
	return P;
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
		const cvx_light_params P = Params(p);
		p += 16;
		const cvxb::CopyWorld W = C.View();
		if (cvxb::LightParamsError(P)) { return 4; }
		cvxb::PiecesBox B{ 0, 0, 0, 0, 0, 0 }; // (a box outside the world lights nothing)
		(void)cvxb::PiecesClipBox(P.boxMin, P.boxMax, gx, dimY, gz, &B);
		for (int c = 0; c < gx * gz; c++) {
			const int cx = c / gz, cz = c % gz;
			const cvxb::LightFromRecords recolour{ cvxb::ArenaOcc{ W }, B, P, cx, cz };
			if (!AppendEditedColumn(&out, [&](uint32_t *runs, uint32_t *colours) { return cvxb::LightColumn(W, cx, cz, runs, colours, recolour); })) { return 3; }
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	int32_t words[16];
	for (int k = 0; k < 16; k++) { words[k] = std::atoi(argv[7 + k]); }
	const cvx_light_params P = Params(words);
	const int levelCount = std::atoi(argv[23]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (cvxb::LightParamsError(P) || !cvxb::PiecesClipBox(P.boxMin, P.boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	const int64_t align = ((int64_t)1 << levelCount) - 1;
	const int64_t x0 = B.x0 & ~align, z0 = B.z0 & ~align;
	int64_t x1 = (B.x1 + align) & ~align, z1 = (B.z1 + align) & ~align;
	x1 = x1 > dimX ? dimX : x1;
	z1 = z1 > dimZ ? dimZ : z1;
	const int sizeX = (int)(x1 - x0), sizeZ = (int)(z1 - z0);
	std::vector<uint32_t> headers(3 * (size_t)sizeX * sizeZ, 0u), pool;
	int over = 0;
	int64_t lit = 0;
	const auto t0 = std::chrono::steady_clock::now();
	for (int i = 0; i < sizeX * sizeZ; i++) {
		const int cx = (int)x0 + i / sizeZ, cz = (int)z0 + i % sizeZ;
		const cvxb::LightFromRecords recolour{ cvxb::ArenaOcc{ W }, B, P, cx, cz };
		const cvxb::BrushResult r = cvxb::LightColumn(W, cx, cz, nullptr, nullptr, cvxb::LightKeep{});
		over |= r.overLimit ? 1 : 0;
		if (r.runCount == 0u) { continue; }
		const size_t off = pool.size();
		pool.resize(off + r.runCount + 2u + r.colours, 0u);
		cvxb::LightColumn(W, cx, cz, pool.data() + off + 1, pool.data() + off + r.runCount + 2u, recolour);
		headers[3 * (size_t)i] = (uint32_t)off;
		headers[3 * (size_t)i + 1] = r.runCount | (r.worldMin << 16);
		headers[3 * (size_t)i + 2] = r.worldMax;
		if (B.Holds(cx, cz)) {
			const cvxb::ArenaColumn col = cvxb::CopyColumnAt(W, cx, cz);
			for (uint32_t k = 0; k < col.Count(); k++) {
				const cvxb::SolidRun run = col.Run(k);
				const int64_t a = (int64_t)run.bottom > B.y0 ? (int64_t)run.bottom : B.y0, b = (int64_t)run.top < B.y1 ? (int64_t)run.top : B.y1;
				lit += b > a ? b - a : 0;
			}
		}
	}
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	headers.insert(headers.end(), pool.begin(), pool.end());
	std::printf("colorShift %d listed %lld over %d rect %lld %lld %d %d voxels %lld ms %.3f\n", H.colorShift, (long long)H.listedColumns, over, (long long)x0, (long long)z0,
	            sizeX, sizeZ, (long long)lit, ms);
	return WriteFile(argv[24], headers.data(), headers.size() * 4);
}

// a dense world of listed voxels for the constructed cases
struct DenseOcc {
	const std::vector<uint8_t> *solid;
	cvxb::LightDims dims;
	bool operator()(int64_t x, int64_t y, int64_t z) const { return dims.Holds(x, y, z) && (*solid)[((size_t)x * dims.y + (size_t)y) * dims.z + (size_t)z] != 0; }
};

static int ShadeOf(int argc, char **argv)
{
	const cvxb::LightDims dims{ std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) };
	int32_t words[16];
	for (int k = 0; k < 16; k++) { words[k] = std::atoi(argv[5 + k]); }
	const cvx_light_params P = Params(words);
	const int count = std::atoi(argv[21]);
	if (argc != 22 + 3 * count + 4) { return 2; }
	std::vector<uint8_t> solid((size_t)dims.x * dims.y * dims.z, 0);
	for (int k = 0; k < count; k++) {
		const int x = std::atoi(argv[22 + 3 * k]), y = std::atoi(argv[23 + 3 * k]), z = std::atoi(argv[24 + 3 * k]);
		if (!dims.Holds(x, y, z)) { return 2; }
		solid[((size_t)x * dims.y + (size_t)y) * dims.z + (size_t)z] = 1;
	}
	const int x = std::atoi(argv[argc - 3]), y = std::atoi(argv[argc - 2]), z = std::atoi(argv[argc - 1]);
	const DenseOcc occ{ &solid, dims };
	const int sky = P.skyRange > 0 ? cvxb::Sky(occ, x, y, z, P.skyRange) : cvxb::kLightSkyTotal;
	int facing = 0, den = 0;
	bool lit = false;
	if (P.sunDir[0] || P.sunDir[1] || P.sunDir[2]) {
		facing = cvxb::SunFacing(occ, x, y, z, P.sunDir[0], P.sunDir[1], P.sunDir[2], &den);
		lit = cvxb::SunLit(occ, dims, x, y, z, P.sunDir[0], P.sunDir[1], P.sunDir[2], P.sunRange);
	}
	std::printf("%d %d %d %d %d %d\n", sky, facing, den, lit ? 1 : 0, cvxb::Shade(P, sky, facing, den, lit), cvxb::VoxelShade(occ, occ, dims, P, x, y, z));
	return 0;
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_light_params good{};
	good.boxMax[0] = good.boxMax[1] = good.boxMax[2] = 8;
	good.sunDir[1] = 1;
	good.sunLevel = 100;
	good.sunRange = 64;
	good.skyLevel = 100;
	good.skyRange = 8;
	std::vector<int> codes;
	float ms = 0.f;
	codes.push_back(cvx_world_light(nullptr, &good, 0, &ms));
	codes.push_back(cvx_world_light(ctx, nullptr, 0, &ms));
	auto bad = [&](auto change, int levelCount = 0) {
		cvx_light_params P = good;
		change(P);
		codes.push_back(cvx_world_light(ctx, &P, levelCount, &ms));
	};
	bad([](cvx_light_params &P) { P.boxMax[0] = 0; });
	bad([](cvx_light_params &P) { P.boxMin[1] = 9; });
	bad([](cvx_light_params &P) { P.boxMin[2] = 8; });
	bad([](cvx_light_params &P) { P.target = 2; });
	bad([](cvx_light_params &P) { P.target = -1; });
	bad([](cvx_light_params &P) { P.sunLevel = 256; });
	bad([](cvx_light_params &P) { P.sunLevel = -1; });
	bad([](cvx_light_params &P) { P.skyLevel = 256; });
	bad([](cvx_light_params &P) { P.skyLevel = -1; });
	bad([](cvx_light_params &P) { P.floorLevel = 256; });
	bad([](cvx_light_params &P) { P.floorLevel = -1; });
	bad([](cvx_light_params &P) { P.sunRange = 4097; });
	bad([](cvx_light_params &P) { P.sunRange = -1; });
	bad([](cvx_light_params &P) { P.skyRange = 33; });
	bad([](cvx_light_params &P) { P.skyRange = -1; });
	bad([](cvx_light_params &P) { P.sunDir[0] = 1025; });
	bad([](cvx_light_params &P) { P.sunDir[2] = -1025; });
	bad([](cvx_light_params &) {}, -1);
	bad([](cvx_light_params &) {}, 6);
	bad([](cvx_light_params &) {}, 5); // valid: no world yet
	bad([](cvx_light_params &P) { P.sunDir[0] = -1024; P.sunDir[1] = 0; P.sunRange = 4096; P.skyRange = 32; P.sunLevel = P.skyLevel = P.floorLevel = 255; P.target = 1; }); // valid too
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 25 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	if (argc >= 26 && std::strcmp(argv[1], "shade") == 0) { return ShadeOf(argc, argv); }
	std::fprintf(stderr, "usage: light_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <params: 16> <levelCount> <blob out> | shade ... | args\n");
	return 2;
}
