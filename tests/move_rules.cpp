// Host build of the rule of cvx_world_move (cpuvox_amd/csrc/cvx_move.h) for tests/test_world_move_cpu.py, one lane per body (cvxb::MoveSolo).
//   move_rules cases <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then repeat bodyCount and the 12 words of every cvx_move_body.  Out per
//     body: the 4 words of its cvx_move_result (CVX_MOVED_INVALID for a body outside the limits, as the kernel answers).
//   move_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <repeat> <bodies in> <results out>
//     Uploads the LOD-0 blob into a context that never touches a device and moves the bodies of the file over its records.  Prints the layout
//     and the milliseconds of the moves alone (tools/move_bench.py: the host route).
//   move_rules lanes <bodies in>
//     Prints the largest leg region among the bodies of the file and the lanesPerBody the host-array call picks for it (cvxb::MoveLanesFor).
//   move_rules args
//     The argument checks of cvx_world_move / cvx_world_move_device on a context without a device or world: one return code per call.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_move.h"
#include "rules_world.h"

static cvx_move_result Move(const cvxb::CopyWorld &W, bool repeat, const cvx_move_body &b)
{
	return cvxb::MoveBodyValid(b) ? cvxb::MoveBody(W, repeat, b, cvxb::MoveSolo{}) : cvxb::MoveInvalid(b);
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<cvx_move_result> out;
	while (p < end) {
		CaseWorld C;
		p = C.Read(p);
		const cvxb::CopyWorld W = C.View(); // (occupancy only: the colours are never read)
		const bool repeat = *p++ != 0;
		const int bodyCount = *p++;
		for (int i = 0; i < bodyCount; i++) {
			cvx_move_body b;
			std::memcpy(&b, p, sizeof b);
			p += sizeof b / 4;
			out.push_back(Move(W, repeat, b));
		}
	}
	return WriteFile(outPath, out.data(), out.size() * sizeof(cvx_move_result));
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const bool repeat = std::atoi(argv[7]) != 0;
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	const std::vector<uint8_t> in = ReadFile(argv[8]);
	const size_t n = in.size() / sizeof(cvx_move_body);
	const cvx_move_body *bodies = reinterpret_cast<const cvx_move_body *>(in.data());
	std::vector<cvx_move_result> out(n);
	const auto t0 = std::chrono::steady_clock::now();
	for (size_t i = 0; i < n; i++) { out[i] = Move(W, repeat, bodies[i]); }
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	std::printf("colorShift %d listed %lld bodies %zu ms %.3f\n", H.colorShift, (long long)H.listedColumns, n, ms);
	return WriteFile(argv[9], out.data(), out.size() * sizeof(cvx_move_result));
}

static int Lanes(const char *path)
{
	const std::vector<uint8_t> in = ReadFile(path);
	const cvx_move_body *bodies = reinterpret_cast<const cvx_move_body *>(in.data());
	int64_t region = 0;
	for (size_t i = 0; i < in.size() / sizeof(cvx_move_body); i++) {
		const int64_t r = cvxb::MoveLegRegion(bodies[i]);
		region = r > region ? r : region;
	}
	std::printf("region %lld lanes %d\n", (long long)region, cvxb::MoveLanesFor(region));
	return 0;
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_move_body good{};
	good.size[0] = good.size[1] = good.size[2] = 100;
	good.delta[1] = -10;
	cvx_move_result result{};
	std::vector<int> codes;
	// the host-array call: no context, NULL arrays, a bad count
	codes.push_back(cvx_world_move(nullptr, 1, &good, &result));
	codes.push_back(cvx_world_move(ctx, 1, nullptr, &result));
	codes.push_back(cvx_world_move(ctx, 1, &good, nullptr));
	codes.push_back(cvx_world_move(ctx, 0, &good, &result));
	codes.push_back(cvx_world_move(ctx, -1, &good, &result));
	// ... and every limit of a body
	auto bad = [&](auto change) {
		cvx_move_body b[2] = { good, good };
		change(b[1]);
		codes.push_back(cvx_world_move(ctx, 2, b, &result));
	};
	bad([](cvx_move_body &b) { b.size[0] = 0; });
	bad([](cvx_move_body &b) { b.size[1] = -5; });
	bad([](cvx_move_body &b) { b.size[2] = 64 * 256 + 1; });
	bad([](cvx_move_body &b) { b.delta[0] = 256 * 256 + 1; });
	bad([](cvx_move_body &b) { b.delta[1] = -256 * 256 - 1; });
	bad([](cvx_move_body &b) { b.delta[2] = INT32_MIN; });
	bad([](cvx_move_body &b) { b.stepUp = -1; });
	bad([](cvx_move_body &b) { b.stepUp = 4 * 256 + 1; });
	bad([](cvx_move_body &b) { b.pos[0] = (1 << 28) + 1; });
	bad([](cvx_move_body &b) { b.pos[1] = -(1 << 28) - 1; });
	bad([](cvx_move_body &b) { b.pos[2] = INT32_MAX; });
	bad([](cvx_move_body &b) { b.flags = 4; });
	bad([](cvx_move_body &b) { b.flags = -1; });
	// the device call: no context, NULL arrays, a bad count, every lanesPerBody that is not 0, 1, 4, 16, 64
	codes.push_back(cvx_world_move_device(nullptr, 1, &good, &result, 0, nullptr));
	codes.push_back(cvx_world_move_device(ctx, 1, nullptr, &result, 0, nullptr));
	codes.push_back(cvx_world_move_device(ctx, 1, &good, nullptr, 0, nullptr));
	codes.push_back(cvx_world_move_device(ctx, 0, &good, &result, 0, nullptr));
	for (int lanes : { -1, 2, 3, 8, 32, 65, 128 }) { codes.push_back(cvx_world_move_device(ctx, 1, &good, &result, lanes, nullptr)); }
	// valid calls: the world is missing
	bad([](cvx_move_body &b) { b.size[0] = b.size[1] = b.size[2] = 64 * 256; b.delta[0] = 256 * 256; b.delta[2] = -256 * 256; b.stepUp = 4 * 256; b.pos[0] = 1 << 28; b.pos[2] = -(1 << 28); b.flags = 3; });
	for (int lanes : { 0, 1, 4, 16, 64 }) { codes.push_back(cvx_world_move_device(ctx, 1, &good, &result, lanes, nullptr)); }
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 3 && std::strcmp(argv[1], "lanes") == 0) { return Lanes(argv[2]); }
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 10 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: move_rules cases <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <repeat> <bodies in> <results out> | lanes <bodies in> | args\n");
	return 2;
}
