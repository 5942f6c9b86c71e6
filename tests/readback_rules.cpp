// Host build of the read-back rule (cpuvox_amd/csrc/cvx_readback.h) for tests/test_world_readback_cpu.py.
//   readback_rules column <cases in> <results out>
//     Each case is one column of a level in the reference's layout (int32 words): lod dimY stride colorsBase worldMin worldMax runCount
//     (colorsIndex length)* colourCount colour*.  The column gets its record and its colour slots as a case world's columns do
//     (tests/rules_world.h), with the stated bounds and at the level's scale, and goes through cvxr::ReadColumn.  Out per case: runCount colours
//     worldMin worldMax, the runs, the colours, then the three header words cvxr::ReadHeader makes with storageOffset 7.
//   readback_rules level <blob> <lod> <dimX> <dimY> <dimZ> <columnCount> <out>
//     Uploads the level into a context that never touches a device (cvx_world_upload lays it out on the host; an empty LOD 0 first for lod > 0)
//     and reads the whole level back from the host copy of its tables as cvx_world_read_level assembles it: World.ColumnCount headers, the pool
//     in column order.
//   readback_rules args
//     The argument checks of the new calls on a context that never touched a device (no world): one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_readback.h"
#include "rules_world.h"

static int Column(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		const int lod = *p++, dimY = *p++, stride = *p++, colorsBase = *p++, worldMin = *p++, worldMax = *p++, runCount = *p++;
		std::vector<uint32_t> elements, slots, runs(8, 0u);
		p = ReadCaseRuns(p, runCount, dimY, &elements);
		p = ReadCaseColours(p, colorsBase, stride, &slots);
		const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)worldMin << 16), (uint32_t)worldMax };
		const uint4 rec = runCount > 0 ? CaseRecord(header, elements, lod, dimY, colorsBase, &runs) : uint4{ 0u, 0u, 0u, 0u };
		const cvxb::ArenaColumn col{ rec.x, rec.y, rec.z, rec.w, runs.data() };
		const int colorShift = CaseColorShift(stride);
		const cvxr::ReadResult r = cvxr::ReadColumn(col, slots.data(), colorShift, lod, dimY, nullptr, nullptr);
		std::vector<uint32_t> newRuns(r.runCount + 1u), newColours(r.colours + 1u);
		const cvxr::ReadResult again = cvxr::ReadColumn(col, slots.data(), colorShift, lod, dimY, newRuns.data(), newColours.data());
		if (again.runCount != r.runCount || again.colours != r.colours) { return 3; }
		out.push_back(r.runCount);
		out.push_back(r.colours);
		out.push_back(r.worldMin);
		out.push_back(r.worldMax);
		out.insert(out.end(), newRuns.begin(), newRuns.begin() + r.runCount);
		out.insert(out.end(), newColours.begin(), newColours.begin() + r.colours);
		uint32_t h[3];
		cvxr::ReadHeader(r, 7u, h);
		out.insert(out.end(), h, h + 3);
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int Level(char **argv)
{
	const std::vector<uint8_t> blob = ReadFile(argv[2]);
	const int lod = std::atoi(argv[3]), dimX = std::atoi(argv[4]), dimY = std::atoi(argv[5]), dimZ = std::atoi(argv[6]), columnCount = std::atoi(argv[7]);
	cvx_context *ctx = new cvx_context();
	if (lod > 0) { UploadBlobLevel(ctx, 0, std::vector<uint8_t>((size_t)dimX * dimZ * 12, 0u), dimX, dimY, dimZ, dimX * dimZ); }
	UploadBlobLevel(ctx, lod, blob, dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = ctx->hostLevel[lod];
	const int usedX = dimX >> lod, usedZ = dimZ >> lod;
	const int64_t count = ((int64_t)dimX * dimZ) / ((int64_t)(lod + 1) * (lod + 1)); // World.ColumnCount
	// count, scan, write: what read_count_kernel / ExclusiveScan / read_write_kernel do
	std::vector<uint32_t> headers((size_t)count * 3, 0u), pool;
	for (int cx = 0; cx < usedX; cx++) {
		for (int cz = 0; cz < usedZ; cz++) {
			const uint4 r = H.records[((size_t)cx << H.rowShift) + (size_t)cz];
			const cvxb::ArenaColumn col{ r.x, r.y, r.z, r.w, reinterpret_cast<const uint32_t *>(H.runs.data()) };
			const cvxr::ReadResult res = cvxr::ReadColumn(col, H.elements.data(), H.colorShift, lod, dimY, nullptr, nullptr);
			const uint32_t off = (uint32_t)pool.size();
			cvxr::ReadHeader(res, off, headers.data() + 3 * ((size_t)cx * usedZ + cz));
			if (res.runCount == 0u) { continue; }
			pool.resize(pool.size() + cvxr::ReadElements(res), 0u);
			cvxr::ReadColumn(col, H.elements.data(), H.colorShift, lod, dimY, pool.data() + off + 1, pool.data() + off + res.runCount + 2);
		}
	}
	std::vector<uint8_t> out(headers.size() * 4 + pool.size() * 4);
	std::memcpy(out.data(), headers.data(), headers.size() * 4);
	if (!pool.empty()) { std::memcpy(out.data() + headers.size() * 4, pool.data(), pool.size() * 4); }
	std::printf("colorShift %d listed %lld\n", H.colorShift, (long long)H.listedColumns);
	return WriteFile(argv[8], out.data(), out.size());
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	void *blob = nullptr;
	int64_t bytes = 0;
	int32_t columns = 0;
	int64_t reclaimed = 0;
	float ms = 0.f;
	const int codes[] = {
		cvx_world_read_region(ctx, 0, 0, 0, 1, 1, nullptr, &bytes, &columns), cvx_world_read_region(ctx, 0, 0, 0, 1, 1, &blob, nullptr, &columns),
		cvx_world_read_region(ctx, 0, 0, 0, 1, 1, &blob, &bytes, nullptr), cvx_world_read_region(ctx, -1, 0, 0, 1, 1, &blob, &bytes, &columns),
		cvx_world_read_region(ctx, 6, 0, 0, 1, 1, &blob, &bytes, &columns), cvx_world_read_region(ctx, 0, -1, 0, 1, 1, &blob, &bytes, &columns),
		cvx_world_read_region(ctx, 0, 0, 0, 0, 1, &blob, &bytes, &columns),
		cvx_world_read_level(ctx, 0, nullptr, &bytes, &columns), cvx_world_read_level(ctx, 6, &blob, &bytes, &columns),
		cvx_world_read_region(ctx, 0, 0, 0, 1, 1, &blob, &bytes, &columns), // valid: no world yet
		cvx_world_read_level(ctx, 3, &blob, &bytes, &columns),
		cvx_world_compact(ctx, &reclaimed, &ms),
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return blob == nullptr ? 0 : 4;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "column") == 0) { return Column(argv[2], argv[3]); }
	if (argc == 9 && std::strcmp(argv[1], "level") == 0) { return Level(argv); }
	std::fprintf(stderr, "usage: readback_rules column <in> <out> | level <blob> <lod> <dimX> <dimY> <dimZ> <columnCount> <out> | args\n");
	return 2;
}
