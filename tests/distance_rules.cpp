// Host build of the distance-field rules (cpuvox_amd/csrc/cvx_distance.h) for tests/test_world_distance_cpu.py.
//   distance_rules fields <blob> <dimX> <dimY> <dimZ> <columnCount> <queries in> <fields out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host) and runs
//     cvxb::DistanceField, the three passes an element at a time with the functions the kernels call, for every query: nine int32 words
//     boxMin[3] boxSize[3] maxDistance mode solidOutside.  Out: the fields one after the other, int32, in the dense layout.
//   distance_rules args
//     The argument checks of the two calls on a context without a device or world: one return code per call.  Before them cvxb::DistanceSplit
//     is compared with plain 64-bit arithmetic on element indices around 2^31 and 2^32, where it changes from 32-bit to 64-bit divisions
//     (exit code 3 when they differ).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_distance.h"
#include "rules_world.h"
static int Fields(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvxb::CopyWorld &W = blob.W;
	const std::vector<uint8_t> queryBytes = ReadFile(argv[7]);
	const int32_t *q = reinterpret_cast<const int32_t *>(queryBytes.data());
	FILE *f = std::fopen(argv[8], "wb");
	if (!f) { return 2; }
	for (size_t k = 0; k + 9 <= queryBytes.size() / 4; k += 9) {
		cvxb::DistanceGrid G;
		for (int a = 0; a < 3; a++) {
			G.box.min[a] = q[k + a];
			G.box.size[a] = q[k + 3 + a];
		}
		G.R = q[k + 6];
		G.solidOutside = q[k + 8];
		std::vector<uint16_t> fromY(G.ElementsY(), 0xFFFFu), fromZ(G.ElementsZ(), 0xFFFFu);
		std::vector<int32_t> out(G.Elements(), -12345);
		cvxb::DistanceField(W, G, q[k + 7], fromY.data(), fromZ.data(), out.data());
		std::fwrite(out.data(), 4, out.size(), f);
	}
	std::fclose(f);
	return 0;
}

static bool SplitAgrees()
{
	const uint64_t sizes[][2] = { { 1, 1 }, { 7, 5 }, { 64, 766 }, { 8300, 511 }, { 65536, 3 }, { 2147483647ull, 2 } };
	const uint64_t around[] = { 0, 1, 12345, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 77, 0xFFFFFFFFull, 1ull << 32, (1ull << 32) + 1, (1ull << 40) + 123456789 };
	for (const auto &s : sizes) {
		for (uint64_t i : around) {
			uint64_t x, z, y;
			cvxb::DistanceSplit(i, s[0], s[1], &x, &z, &y);
			const uint64_t column = i / s[0];
			if (y != i % s[0] || z != column % s[1] || x != column / s[1]) { return false; }
		}
	}
	return true;
}

static int Args()
{
	if (!SplitAgrees()) { return 3; }
	cvx_context *ctx = new cvx_context();
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 2, 2, 2 }, emptyHi[3] = { 2, 0, 2 }, farLo[3] = { -(1 << 30) - 1, 0, 0 }, farHi[3] = { 2, (1 << 30) + 1, 2 };
	const int32_t hugeLo[3] = { -1024, -1024, -1024 }, hugeHi[3] = { 1024, 1024, -512 }; // 2048 * 2048 * 512 = 2^31 voxels
	int32_t out[8] = {};
	const int S = CVX_DISTANCE_TO_SOLID, O = CVX_SURFACE_OUTSIDE_DEFAULT;
	const int codes[] = {
		cvx_world_distance(nullptr, lo, hi, 4, S, O, out, nullptr), cvx_world_distance_device(nullptr, lo, hi, 4, S, O, out, nullptr),
		cvx_world_distance(ctx, nullptr, hi, 4, S, O, out, nullptr), cvx_world_distance(ctx, lo, nullptr, 4, S, O, out, nullptr),
		cvx_world_distance(ctx, lo, hi, 4, S, O, nullptr, nullptr), cvx_world_distance_device(ctx, lo, hi, 4, S, O, nullptr, nullptr),
		cvx_world_distance(ctx, lo, emptyHi, 4, S, O, out, nullptr), cvx_world_distance(ctx, hi, lo, 4, S, O, out, nullptr),
		cvx_world_distance(ctx, farLo, hi, 4, S, O, out, nullptr), cvx_world_distance(ctx, lo, farHi, 4, S, O, out, nullptr),
		cvx_world_distance(ctx, hugeLo, hugeHi, 4, S, O, out, nullptr),
		cvx_world_distance(ctx, lo, hi, 0, S, O, out, nullptr), cvx_world_distance(ctx, lo, hi, 256, S, O, out, nullptr),
		cvx_world_distance(ctx, lo, hi, -3, S, O, out, nullptr),
		cvx_world_distance(ctx, lo, hi, 4, 3, O, out, nullptr), cvx_world_distance(ctx, lo, hi, 4, -1, O, out, nullptr),
		cvx_world_distance(ctx, lo, hi, 4, S, 0x40, out, nullptr), cvx_world_distance_device(ctx, lo, hi, 4, S, -1, out, nullptr),
		// valid: no world yet
		cvx_world_distance(ctx, lo, hi, 1, CVX_DISTANCE_TO_SOLID, 0, out, nullptr), cvx_world_distance(ctx, lo, hi, 255, CVX_DISTANCE_SIGNED, 0x3F, out, nullptr),
		cvx_world_distance_device(ctx, lo, hi, 4, CVX_DISTANCE_TO_AIR, O, out, nullptr),
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 9 && std::strcmp(argv[1], "fields") == 0) { return Fields(argv); }
	std::fprintf(stderr, "usage: distance_rules fields <blob> <dimX> <dimY> <dimZ> <columnCount> <queries> <out> | args\n");
	return 2;
}
