// Host build of the rule of cvx_world_move (cpuvox_amd/csrc/cvx_move.h) for tests/test_world_move_cpu.py, one lane per body (cvxb::MoveSolo).
//   move_rules cases <cases in> <results out>
//     Each case is a small world of gx x gz columns in the reference's layout (int32 words, the format of tests/light_rules.cpp): dimY gx gz
//     stride, per column (x-major) colorsBase runCount (colorsIndex length)* colourCount colour*, then repeat bodyCount and the 12 words of every
//     cvx_move_body.  Out per body: the 4 words of its cvx_move_result (CVX_MOVED_INVALID for a body outside the limits, as the kernel answers).
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

#include "cvx_context.h"
#include "cvx_move.h"

static std::vector<uint8_t> ReadFile(const char *path)
{
	std::vector<uint8_t> out;
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::exit(2); }
	uint8_t buffer[65536];
	for (size_t n; (n = std::fread(buffer, 1, sizeof buffer, f)) > 0;) { out.insert(out.end(), buffer, buffer + n); }
	std::fclose(f);
	return out;
}

static int WriteFile(const char *path, const void *data, size_t bytes)
{
	FILE *f = std::fopen(path, "wb");
	if (!f) { return 2; }
	std::fwrite(data, 1, bytes, f);
	std::fclose(f);
	return 0;
}

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
		const int dimY = *p++, gx = *p++, gz = *p++, stride = *p++;
		int rowShift = 0;
		while ((1 << rowShift) < gz) { rowShift++; }
		std::vector<uint4> records((size_t)gx << rowShift, uint4{ 0u, 0u, 0u, 0u });
		std::vector<uint32_t> runs(8, 0u);
		for (int c = 0; c < gx * gz; c++) {
			const int colorsBase = *p++, runCount = *p++;
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
			p += colourCount; // (occupancy only: the colours are never read)
			const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)(lowest < 0 ? 0 : lowest) << 16), (uint32_t)(highest < 0 ? 0 : highest) };
			uint4 rec{ 0u, 0u, 0u, 0u };
			if (runCount > 0 && highest >= 0) {
				const cvxe::ColumnWords w = cvxe::BuildColumnWords(header, elements.data(), 0, dimY);
				rec = uint4{ w.x | (uint32_t)colorsBase, w.y, w.z, w.w };
				if (w.code == 0u) {
					const size_t entry = runs.size() / 2;
					rec.z = (uint32_t)entry;
					runs.resize(runs.size() + 2u * w.solid + 8u, 0u);
					cvxe::BuildListedRuns(header, elements.data(), 0, dimY, runs.data() + 2 * entry);
				}
			}
			records[((size_t)(c / gz) << rowShift) + (size_t)(c % gz)] = rec;
		}
		cvxb::CopyWorld W;
		W.records = reinterpret_cast<const uint32_t *>(records.data());
		W.runs = runs.data();
		W.colourSlots = nullptr;
		W.rowShift = rowShift;
		W.colorShift = stride == 1 ? 2 : 7;
		W.dimX = gx;
		W.dimY = dimY;
		W.dimZ = gz;
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
	std::vector<uint8_t> blob = ReadFile(argv[2]);
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const bool repeat = std::atoi(argv[7]) != 0;
	cvx_context *ctx = new cvx_context();
	const int rc = cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size(), dimX, dimY, dimZ, columnCount);
	if (rc != CVX_OK) { std::printf("upload failed %d: %s\n", rc, ctx->error.c_str()); return 1; }
	const cvx_context::HostLevel &H = ctx->hostLevel[0];
	cvxb::CopyWorld W;
	W.records = reinterpret_cast<const uint32_t *>(H.records.data());
	W.runs = reinterpret_cast<const uint32_t *>(H.runs.data());
	W.colourSlots = H.elements.data();
	W.rowShift = H.rowShift;
	W.colorShift = H.colorShift;
	W.dimX = dimX;
	W.dimY = dimY;
	W.dimZ = dimZ;
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
