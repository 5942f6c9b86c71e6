// Host build of the rules of cvx_world_light_lamps (cpuvox_amd/csrc/cvx_lamps.h) for tests/test_world_lamps_cpu.py, driven sequentially with every
// occupancy test answered from the records (cvxb::ArenaOcc).  The formats are those of tests/light_rules.cpp with the lamps appended.
//   lamp_rules columns <cases in> <results out>
//     Per case (int32 words): a case world (tests/rules_world.h), the 16 words of cvx_light_params, lampCount, per lamp x y z radius level.
//     Out per case (uint32 words), for every column of the world after the call: the edited-column block (tests/rules_world.h).
//   lamp_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <16 words of cvx_light_params> <levelCount> <lamps file: 5 int32 per lamp> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device and writes the sub-world blob of the call's rectangle as cvx_light.hip
//     makes it.  Prints the rectangle, the voxels lit and the milliseconds of the lighting alone (tools/light_bench.py: the host route).
//   lamp_rules shade <dimX> <dimY> <dimZ> <16 words of cvx_light_params> <voxel count> (x y z)* -- <x y z> <lampCount> (x y z radius level)*
//     Voxel <x y z> in a world of the listed solid voxels: prints the shade without lamps, every lamp's term and the shade with them.
//   lamp_rules args
//     cvx_world_light_lamps' argument checks on a context without a device or world: one return code per call, then the error texts.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cvx_lamps.h"
#include "rules_world.h"

static cvx_light_params Params(const int32_t *w)
{
	cvx_light_params P;
	std::memcpy(&P, w, sizeof P);
	return P;
}

static std::vector<cvx_lamp> Lamps(const int32_t *w, int count)
{
	std::vector<cvx_lamp> out((size_t)count);
	for (int l = 0; l < count; l++) { out[(size_t)l] = cvx_lamp{ { w[5 * l], w[5 * l + 1], w[5 * l + 2] }, w[5 * l + 3], w[5 * l + 4], { 0, 0, 0 } }; }
	return out;
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
		const int lampCount = *p++;
		const std::vector<cvx_lamp> lamps = Lamps(p, lampCount);
		p += 5 * lampCount;
		const cvxb::CopyWorld W = C.View();
		if (cvxb::LightParamsError(P) || cvxb::LampParamsError(lamps.data(), lampCount)) { return 4; }
		cvxb::PiecesBox B{ 0, 0, 0, 0, 0, 0 }; // (a box outside the world lights nothing)
		(void)cvxb::PiecesClipBox(P.boxMin, P.boxMax, gx, dimY, gz, &B);
		for (int c = 0; c < gx * gz; c++) {
			const int cx = c / gz, cz = c % gz;
			const cvxb::LightLampsFromRecords recolour{ cvxb::ArenaOcc{ W }, B, P, cx, cz, lamps.data(), lampCount };
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
	const std::vector<uint8_t> lampBytes = ReadFile(argv[24]);
	const int lampCount = (int)(lampBytes.size() / 20);
	const std::vector<cvx_lamp> lamps = Lamps(reinterpret_cast<const int32_t *>(lampBytes.data()), lampCount);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (cvxb::LightParamsError(P) || cvxb::LampParamsError(lamps.data(), lampCount) || !cvxb::PiecesClipBox(P.boxMin, P.boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	const int64_t align = ((int64_t)1 << levelCount) - 1;
	const int64_t x0 = B.x0 & ~align, z0 = B.z0 & ~align;
	int64_t x1 = (B.x1 + align) & ~align, z1 = (B.z1 + align) & ~align;
	x1 = x1 > dimX ? dimX : x1;
	z1 = z1 > dimZ ? dimZ : z1;
	const int sizeX = (int)(x1 - x0), sizeZ = (int)(z1 - z0);
	std::vector<uint32_t> headers(3 * (size_t)sizeX * sizeZ, 0u), pool;
	int64_t lit = 0;
	const auto t0 = std::chrono::steady_clock::now();
	for (int i = 0; i < sizeX * sizeZ; i++) {
		const int cx = (int)x0 + i / sizeZ, cz = (int)z0 + i % sizeZ;
		const cvxb::LightLampsFromRecords recolour{ cvxb::ArenaOcc{ W }, B, P, cx, cz, lamps.data(), lampCount };
		const cvxb::BrushResult r = cvxb::LightColumn(W, cx, cz, nullptr, nullptr, cvxb::LightKeep{});
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
	std::printf("rect %lld %lld %d %d voxels %lld ms %.3f\n", (long long)x0, (long long)z0, sizeX, sizeZ, (long long)lit, ms);
	return WriteFile(argv[25], headers.data(), headers.size() * 4);
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
	int at = 22 + 3 * count;
	if (argc < at + 5 || std::strcmp(argv[at], "--") != 0) { return 2; }
	std::vector<uint8_t> solid((size_t)dims.x * dims.y * dims.z, 0);
	for (int k = 0; k < count; k++) {
		const int x = std::atoi(argv[22 + 3 * k]), y = std::atoi(argv[23 + 3 * k]), z = std::atoi(argv[24 + 3 * k]);
		if (!dims.Holds(x, y, z)) { return 2; }
		solid[((size_t)x * dims.y + (size_t)y) * dims.z + (size_t)z] = 1;
	}
	const int x = std::atoi(argv[at + 1]), y = std::atoi(argv[at + 2]), z = std::atoi(argv[at + 3]);
	const int lampCount = std::atoi(argv[at + 4]);
	if (argc != at + 5 + 5 * lampCount) { return 2; }
	std::vector<int32_t> lampWords;
	for (int k = 0; k < 5 * lampCount; k++) { lampWords.push_back(std::atoi(argv[at + 5 + k])); }
	const std::vector<cvx_lamp> lamps = Lamps(lampWords.data(), lampCount);
	if (cvxb::LampParamsError(lamps.data(), lampCount)) { return 4; }
	const DenseOcc occ{ &solid, dims };
	std::printf("%d", cvxb::VoxelShade(occ, occ, dims, P, x, y, z));
	for (const cvx_lamp &l : lamps) { std::printf(" %d", cvxb::LampVoxelTerm(occ, x, y, z, l.pos[0], l.pos[1], l.pos[2], l.radius, l.level)); }
	std::printf(" %d\n", cvxb::VoxelShadeLamps(occ, occ, dims, P, x, y, z, lamps.data(), lampCount));
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
	const cvx_lamp lamp{ { 1, 2, 3 }, 8, 200, { 0, 0, 0 } };
	std::vector<int> codes;
	std::vector<std::string> texts;
	float ms = 0.f;
	auto call = [&](cvx_context *c, const cvx_light_params *P, const cvx_lamp *lamps, int lampCount, int levelCount) {
		codes.push_back(cvx_world_light_lamps(c, P, lamps, lampCount, levelCount, &ms));
		texts.push_back(c ? cvx_last_error(c) : "");
	};
	auto bad = [&](auto change) {
		std::vector<cvx_lamp> lamps(3, lamp);
		change(lamps[1]);
		call(ctx, &good, lamps.data(), 3, 0);
	};
	call(nullptr, &good, &lamp, 1, 0);
	call(ctx, nullptr, &lamp, 1, 0);
	call(ctx, &good, &lamp, -1, 0);
	call(ctx, &good, &lamp, 4097, 0);
	call(ctx, &good, nullptr, 1, 0);
	bad([](cvx_lamp &l) { l.radius = 0; });
	bad([](cvx_lamp &l) { l.radius = 65; });
	bad([](cvx_lamp &l) { l.level = -1; });
	bad([](cvx_lamp &l) { l.level = 256; });
	bad([](cvx_lamp &l) { l.pos[0] = (1 << 20) + 1; });
	bad([](cvx_lamp &l) { l.pos[2] = -(1 << 20) - 1; });
	{ // cvx_world_light's own rules hold too
		cvx_light_params P = good;
		P.skyRange = 33;
		call(ctx, &P, &lamp, 1, 0);
	}
	call(ctx, &good, &lamp, 1, 6);
	// valid: no world yet
	call(ctx, &good, nullptr, 0, 5);
	call(ctx, &good, &lamp, 1, 0);
	bad([](cvx_lamp &l) { l.radius = 64; l.level = 255; l.pos[0] = 1 << 20; l.pos[1] = -(1 << 20); });
	std::vector<cvx_lamp> most(4096, lamp);
	call(ctx, &good, most.data(), 4096, 0);
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	for (const std::string &t : texts) { std::printf("%s\n", t.c_str()); }
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 26 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	if (argc >= 27 && std::strcmp(argv[1], "shade") == 0) { return ShadeOf(argc, argv); }
	std::fprintf(stderr, "usage: lamp_rules columns <in> <out> | world ... | shade ... | args\n");
	return 2;
}
