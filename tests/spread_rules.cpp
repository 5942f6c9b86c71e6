// Host build of the spread rules (cpuvox_amd/csrc/cvx_spread.h) for tests/test_world_spread_cpu.py.
//   spread_rules fields <blob> <dimX> <dimY> <dimZ> <columnCount> <queries in> <fields out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host) and walks the call as
//     cvx_spread.hip does, with the functions its kernels call: SpreadInitHost (the chunk access of the init kernel, checked here against
//     cvxb::SpreadPassable voxel by voxel: exit code 4 when they differ), SpreadSeedHost, then launches of SpreadTileHost over the active tiles,
//     one tile after the other in a deliberately awkward order -- a stride permutation of the tile numbers, or that order reversed --, the active
//     flags double-buffered, until a launch lowers nothing (more than maxSteps + 2 launches: exit code 5), then SpreadResult.
//     A query is eleven int32 words boxMin[3] boxSize[3] medium stepFaces maxSteps order seedCount and four words per seed.  Out, per query: the
//     field, int32, in the dense layout, then six int32 words passable reached largestDistance seedsUsed launches tileVisits.
//   spread_rules args
//     The argument checks of the two calls on a context without a device or world: a line "code|message" per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_spread.h"
#include "rules_world.h"
static int64_t Gcd(int64_t a, int64_t b) { return b == 0 ? a : Gcd(b, a % b); }

static int Fields(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvxb::CopyWorld &W = blob.W;
	const std::vector<uint8_t> queryBytes = ReadFile(argv[7]);
	const int32_t *q = reinterpret_cast<const int32_t *>(queryBytes.data());
	const size_t words = queryBytes.size() / 4;
	FILE *f = std::fopen(argv[8], "wb");
	if (!f) { return 2; }
	for (size_t k = 0; k + 11 <= words;) {
		cvx_spread_params P{};
		for (int a = 0; a < 3; a++) {
			P.boxMin[a] = q[k + a];
			P.boxMax[a] = q[k + a] + q[k + 3 + a];
		}
		P.medium = q[k + 6];
		P.stepFaces = q[k + 7];
		P.maxSteps = q[k + 8];
		const bool reversed = q[k + 9] != 0;
		const int seedCount = q[k + 10];
		std::vector<cvx_spread_seed> seeds((size_t)seedCount);
		std::memcpy(seeds.data(), q + k + 11, (size_t)seedCount * 16);
		k += 11 + 4 * (size_t)seedCount;
		char message[160];
		int32_t probe = 0;
		if (cvxb::SpreadCheck(&P, seeds.data(), seedCount, &probe, message, sizeof message) != 0) { std::printf("rejected: %s\n", message); return 3; }
		const cvxb::SpreadGrid G = cvxb::SpreadGridOf(P);
		std::vector<uint16_t> dist(G.Elements(), 0);
		std::vector<uint64_t> bits(G.Words(), 0);
		const int64_t tiles = G.Tiles();
		std::vector<uint8_t> flags[2] = { std::vector<uint8_t>((size_t)tiles, 0), std::vector<uint8_t>((size_t)tiles, 0) };
		int64_t passable = SpreadInitHost(W, G, dist.data(), bits.data());
		int64_t check = 0;
		for (int64_t bx = 0; bx < G.box.size[0]; bx++) {
			for (int64_t bz = 0; bz < G.box.size[2]; bz++) {
				for (int64_t by = 0; by < G.box.size[1]; by++) {
					const bool want = cvxb::SpreadPassable(W, G, G.box.min[0] + bx, G.box.min[1] + by, G.box.min[2] + bz);
					if (want != G.Bit(bits.data(), bx, by, bz) || dist[G.Index(bx, by, bz)] != 0xFFFF) { return 4; }
					check += want ? 1 : 0;
				}
			}
		}
		if (check != passable) { return 4; }
		int32_t seedsUsed = 0;
		for (const cvx_spread_seed &s : seeds) { seedsUsed += cvxb::SpreadSeedHost(G, s, dist.data(), bits.data(), flags[0].data()) ? 1 : 0; }
		// the order of the tiles inside a launch: i -> (i * stride + 1) mod tiles, stride coprime with the tile count and near 0.618 of it
		int64_t stride = tiles * 618 / 1000 | 1;
		while (Gcd(stride, tiles) != 1) { stride += 2; }
		int64_t launches = 0, visits = 0;
		for (bool changed = true; changed;) {
			if (launches >= (int64_t)G.maxSteps + 2) { return 5; }
			std::vector<uint8_t> &active = flags[launches & 1], &next = flags[(launches & 1) ^ 1];
			changed = false;
			for (int64_t i = 0; i < tiles; i++) {
				const int64_t t = ((reversed ? tiles - 1 - i : i) * stride + 1) % tiles;
				if (!active[t]) { continue; }
				active[t] = 0;
				visits++;
				changed = cvxb::SpreadTileHost(G, dist.data(), bits.data(), t, next.data()) || changed;
			}
			launches++;
		}
		std::vector<int32_t> out(G.Elements());
		int32_t reached = 0, largest = -1;
		for (int64_t bx = 0; bx < G.box.size[0]; bx++) {
			for (int64_t bz = 0; bz < G.box.size[2]; bz++) {
				for (int64_t by = 0; by < G.box.size[1]; by++) {
					const uint64_t i = G.Index(bx, by, bz);
					out[i] = cvxb::SpreadResult(G.Bit(bits.data(), bx, by, bz), dist[i]);
					if (out[i] >= 0) {
						reached++;
						largest = out[i] > largest ? out[i] : largest;
					}
				}
			}
		}
		std::fwrite(out.data(), 4, out.size(), f);
		const int32_t summary[6] = { (int32_t)passable, reached, largest, seedsUsed, (int32_t)launches, (int32_t)visits };
		std::fwrite(summary, 4, 6, f);
	}
	std::fclose(f);
	return 0;
}

static void Line(cvx_context *ctx, int code) { std::printf("%d|%s\n", code, ctx && code != CVX_OK ? cvx_last_error(ctx) : ""); }

static int Args()
{
	cvx_context *ctx = new cvx_context();
	const cvx_spread_params good = { { 0, 0, 0 }, { 2, 2, 2 }, CVX_SPREAD_AIR, 0x3F, 10, 0 };
	std::vector<cvx_spread_seed> seeds(CVX_SPREAD_MAX_SEEDS + 1, cvx_spread_seed{ { 0, 0, 0 }, 0 });
	int32_t out[8] = {};
	auto with = [&](auto change) {
		cvx_spread_params p = good;
		change(p);
		return p;
	};
	auto call = [&](const cvx_spread_params &p, int seedCount, bool device = false) {
		Line(ctx, device ? cvx_world_spread_device(ctx, &p, seeds.data(), seedCount, out, nullptr, nullptr) : cvx_world_spread(ctx, &p, seeds.data(), seedCount, out, nullptr, nullptr));
	};
	// no context: the code alone
	Line(nullptr, cvx_world_spread(nullptr, &good, seeds.data(), 1, out, nullptr, nullptr));
	Line(nullptr, cvx_world_spread_device(nullptr, &good, seeds.data(), 1, out, nullptr, nullptr));
	// NULL params / seeds / out
	Line(ctx, cvx_world_spread(ctx, nullptr, seeds.data(), 1, out, nullptr, nullptr));
	Line(ctx, cvx_world_spread(ctx, &good, nullptr, 1, out, nullptr, nullptr));
	Line(ctx, cvx_world_spread(ctx, &good, seeds.data(), 1, nullptr, nullptr, nullptr));
	Line(ctx, cvx_world_spread_device(ctx, &good, seeds.data(), 1, nullptr, nullptr, nullptr));
	// the box: empty, beyond 2^30, 2^31 voxels (2048 * 2048 * 512)
	call(with([](cvx_spread_params &p) { p.boxMax[1] = 0; }), 1);
	call(with([](cvx_spread_params &p) { p.boxMin[0] = -(1 << 30) - 1; }), 1);
	call(with([](cvx_spread_params &p) { p.boxMax[2] = (1 << 30) + 1; }), 1, true);
	call(with([](cvx_spread_params &p) {
		     p.boxMin[0] = p.boxMin[1] = p.boxMin[2] = -1024;
		     p.boxMax[0] = p.boxMax[1] = 1024;
		     p.boxMax[2] = -512;
	     }), 1);
	// medium, stepFaces, maxSteps, seedCount, start
	call(with([](cvx_spread_params &p) { p.medium = 2; }), 1);
	call(with([](cvx_spread_params &p) { p.medium = -1; }), 1, true);
	call(with([](cvx_spread_params &p) { p.stepFaces = 0; }), 1);
	call(with([](cvx_spread_params &p) { p.stepFaces = 0x40; }), 1);
	call(with([](cvx_spread_params &p) { p.maxSteps = 0; }), 1);
	call(with([](cvx_spread_params &p) { p.maxSteps = 65535; }), 1, true);
	call(good, 0);
	call(good, CVX_SPREAD_MAX_SEEDS + 1);
	seeds[5].start = 11;
	call(good, 7);
	seeds[5].start = -1;
	call(good, 7, true);
	// the order of the checks: a bad medium is named before a bad start, a bad box before a bad medium
	call(with([](cvx_spread_params &p) { p.medium = 7; }), 7);
	call(with([](cvx_spread_params &p) { p.medium = 7; p.boxMax[0] = 0; }), 7);
	seeds[5].start = 0;
	// valid (no world yet): maxSteps 1 and 65534, start == maxSteps, 4096 seeds, the 2^31 - 2048 * 2048 voxel box
	call(with([](cvx_spread_params &p) { p.maxSteps = 1; }), 1);
	call(with([](cvx_spread_params &p) { p.maxSteps = 65534; }), 1, true);
	seeds[3].start = 10;
	call(good, 4);
	seeds[3].start = 0;
	call(good, CVX_SPREAD_MAX_SEEDS);
	call(with([](cvx_spread_params &p) {
		     p.boxMin[0] = p.boxMin[1] = p.boxMin[2] = -1024;
		     p.boxMax[0] = p.boxMax[1] = 1024;
		     p.boxMax[2] = -513;
	     }), 1);
	call(with([](cvx_spread_params &p) { p.medium = CVX_SPREAD_SOLID; p.stepFaces = 0x01; p.boxMin[0] = -(1 << 30); p.boxMax[0] = -(1 << 30) + 1; }), 1);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 9 && std::strcmp(argv[1], "fields") == 0) { return Fields(argv); }
	std::fprintf(stderr, "usage: spread_rules fields <blob> <dimX> <dimY> <dimZ> <columnCount> <queries> <out> | args\n");
	return 2;
}
