// Host build of the snapshot comparison's rule (cpuvox_amd/csrc/cvx_snapshot.h) for tests/test_world_snapshot_cpu.py.
//   snapshot_rules column <cases in> <results out>
//     Each case is a pair of columns (int32 words): dimY stride colorsBase ignoreColour, then the ARENA's column in the reference's layout --
//     worldMin worldMax runCount (colorsIndex length)* colourCount colour* -- and the SNAPSHOT's -- runCount (colorsIndex length)* colourCount
//     colour*.  The arena's column gets its record and its colour slots as a case world's columns do (tests/rules_world.h), with the stated
//     bounds, as tests/readback_rules.cpp builds it; the snapshot's column becomes a blob column behind 5 other elements.  Out per case: voxels
//     yMin yMax of cvxs::DiffColumn.
//   snapshot_rules world <arena blob> <dimX> <dimY> <dimZ> <columnCount> <snapshot blob> <x0> <z0> <sizeX> <sizeZ> <ignoreColour> <out>
//     Uploads LOD 0 into a context that never touches a device (cvx_world_upload lays it out on the host) and compares the rectangle with the
//     columns of the second blob, a sub-world of sizeX x sizeZ columns, as the kernels do: count, scan, write.  Out: changedColumns changedVoxels
//     min[3] max[3] (64-bit totals as two words each), then x z yMin yMax per changed column.
//   snapshot_rules args
//     The argument checks of the calls on a context that never touched a device: `code|message` per call.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cpuvox_gpu_snapshot.h"
#include "cvx_snapshot.h"
#include "rules_world.h"

static int Column(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		const int dimY = *p++, stride = *p++, colorsBase = *p++, ignoreColour = *p++;
		// the arena's column
		const int worldMin = *p++, worldMax = *p++, runCount = *p++;
		std::vector<uint32_t> elements, slots, runs(8, 0u);
		p = ReadCaseRuns(p, runCount, dimY, &elements);
		p = ReadCaseColours(p, colorsBase, stride, &slots);
		const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)worldMin << 16), (uint32_t)worldMax };
		const uint4 rec = runCount > 0 ? CaseRecord(header, elements, 0, dimY, colorsBase, &runs) : uint4{ 0u, 0u, 0u, 0u };
		const cvxb::ArenaColumn col{ rec.x, rec.y, rec.z, rec.w, runs.data() };
		// the snapshot's column
		const int snapRuns = *p++;
		std::vector<uint32_t> pool(5, 0xDEADBEEFu);
		pool.push_back(0u);
		for (int r = 0; r < snapRuns; r++) {
			const int32_t ci = *p++, length = *p++;
			pool.push_back(((uint32_t)ci & 0xFFFFu) | ((uint32_t)length << 16));
		}
		pool.push_back(0u);
		const int snapColours = *p++;
		for (int k = 0; k < snapColours; k++) { pool.push_back((uint32_t)*p++); }
		const uint32_t snapHeader[3] = { snapRuns ? 5u : 0u, (uint32_t)snapRuns, 0u };
		const cvxs::ColumnDiff d = cvxs::DiffColumn(col, slots.data(), CaseColorShift(stride), dimY, snapHeader, pool.data(), ignoreColour != 0);
		out.push_back(d.voxels);
		out.push_back(d.yMin);
		out.push_back(d.yMax);
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const std::vector<uint8_t> snap = ReadFile(argv[7]);
	const int x0 = std::atoi(argv[8]), z0 = std::atoi(argv[9]), sizeX = std::atoi(argv[10]), sizeZ = std::atoi(argv[11]), ignoreColour = std::atoi(argv[12]);
	const BlobWorld arena = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *arena.H;
	const int n = sizeX * sizeZ;
	const uint32_t *headers = reinterpret_cast<const uint32_t *>(snap.data());
	const uint32_t *elements = headers + 3 * (size_t)n;
	// count, scan, write: what snapshot_diff_count_kernel / ExclusiveScan / snapshot_diff_write_kernel do
	std::vector<cvxs::ColumnDiff> diffs((size_t)n);
	int64_t columns = 0, voxels = 0;
	int lo[3] = { INT_MAX, INT_MAX, INT_MAX }, hi[3] = { INT_MIN, INT_MIN, INT_MIN };
	for (int i = 0; i < n; i++) {
		const int x = x0 + i / sizeZ, z = z0 + i % sizeZ;
		const uint4 r = H.records[((size_t)x << H.rowShift) + (size_t)z];
		const cvxb::ArenaColumn col{ r.x, r.y, r.z, r.w, reinterpret_cast<const uint32_t *>(H.runs.data()) };
		const cvxs::ColumnDiff d = cvxs::DiffColumn(col, H.elements.data(), H.colorShift, dimY, headers + 3 * (size_t)i, elements, ignoreColour != 0);
		diffs[(size_t)i] = d;
		if (!d.voxels) { continue; }
		columns++;
		voxels += d.voxels;
		const int v[3] = { x, (int)d.yMin, z }, t[3] = { x + 1, (int)d.yMax, z + 1 };
		for (int a = 0; a < 3; a++) {
			lo[a] = v[a] < lo[a] ? v[a] : lo[a];
			hi[a] = t[a] > hi[a] ? t[a] : hi[a];
		}
	}
	std::vector<int32_t> out;
	out.push_back((int32_t)columns);
	out.push_back((int32_t)(columns >> 32));
	out.push_back((int32_t)voxels);
	out.push_back((int32_t)(voxels >> 32));
	for (int a = 0; a < 3; a++) { out.push_back(columns ? lo[a] : 0); }
	for (int a = 0; a < 3; a++) { out.push_back(columns ? hi[a] : 0); }
	for (int i = 0; i < n; i++) {
		if (!diffs[(size_t)i].voxels) { continue; }
		out.push_back(x0 + i / sizeZ);
		out.push_back(z0 + i % sizeZ);
		out.push_back((int32_t)diffs[(size_t)i].yMin);
		out.push_back((int32_t)diffs[(size_t)i].yMax);
	}
	std::printf("colorShift %d listed %lld\n", H.colorShift, (long long)H.listedColumns);
	return WriteFile(argv[13], out.data(), out.size() * 4);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_snapshot *snap = reinterpret_cast<cvx_snapshot *>(ctx); // never dereferenced: every call below fails before it looks at a snapshot
	cvx_snapshot *out = snap;
	cvx_snapshot_info info{};
	cvx_snapshot_change change{};
	float ms = 0.f;
	auto say = [&](int code, bool onContext) { std::printf("%d|%s\n", code, onContext ? cvx_last_error(ctx) : ""); };
	say(cvx_world_snapshot(nullptr, 0, 0, 1, 1, 0, &out, &ms), false);
	say(cvx_world_snapshot(ctx, 0, 0, 1, 1, 0, nullptr, &ms), true);
	say(cvx_world_snapshot(ctx, 0, 0, 1, 1, 6, &out, &ms), true);
	say(cvx_world_snapshot(ctx, 0, 0, 1, 1, -1, &out, &ms), true);
	say(cvx_world_snapshot(ctx, 0, 0, 1, 1, 0, &out, &ms), true); // valid: no world yet
	say(cvx_snapshot_info_get(nullptr, &info), false);
	say(cvx_snapshot_info_get(snap, nullptr), false);
	say(cvx_world_snapshot_restore(nullptr, snap, &ms), false);
	say(cvx_world_snapshot_restore(ctx, nullptr, &ms), true);
	say(cvx_world_snapshot_diff(nullptr, snap, 0, &change, 1, nullptr, &ms), false);
	say(cvx_world_snapshot_diff(ctx, nullptr, 0, &change, 1, nullptr, &ms), true);
	say(cvx_world_snapshot_diff_device(ctx, nullptr, 0, nullptr, 0, nullptr, nullptr), true);
	cvx_snapshot_destroy(nullptr);
	return out == nullptr ? 0 : 4; // (a failed capture leaves *out NULL)
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "column") == 0) { return Column(argv[2], argv[3]); }
	if (argc == 14 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: snapshot_rules column <in> <out> | world <arena blob> <dimX> <dimY> <dimZ> <columnCount> <snapshot blob> <x0> <z0> <sizeX> <sizeZ> "
	                     "<ignoreColour> <out> | args\n");
	return 2;
}
