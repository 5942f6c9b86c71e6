// Host build of the copy rule (cpuvox_amd/csrc/cvx_copy.h) for tests/test_world_copy_cpu.py.
//   copy_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then placementCount and the placements (cvx_copy_placement, 12 words each).
//     Every column of the world goes through cvxb::CopyColumn.  Out per case and column: the edited-column block (tests/rules_world.h).
//   copy_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <placements> <x0> <z0> <sizeX> <sizeZ> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host), runs cvxb::CopyColumn
//     on every column of the rectangle and writes the sub-world blob cvx_copy.hip's write kernel makes (12-byte headers, then the element pool).
//   copy_rules args
//     cvx_world_copy's argument checks on a context without a device or world: one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rules_world.h"

static int Columns(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		CaseWorld C;
		p = C.Read(p);
		const int n = *p++;
		std::vector<cvx_copy_placement> placements((size_t)n);
		std::memcpy(placements.data(), p, (size_t)n * sizeof(cvx_copy_placement));
		p += (size_t)n * sizeof(cvx_copy_placement) / 4;
		const cvxb::CopyWorld W = C.View();
		for (int c = 0; c < C.gx * C.gz; c++) {
			const int64_t cx = c / C.gz, cz = c % C.gz;
			if (!AppendEditedColumn(&out, [&](uint32_t *runs, uint32_t *colours) { return cvxb::CopyColumn(W, placements.data(), n, cx, cz, runs, colours); })) { return 3; }
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const std::vector<uint8_t> placementBytes = ReadFile(argv[7]);
	const int x0 = std::atoi(argv[8]), z0 = std::atoi(argv[9]), sizeX = std::atoi(argv[10]), sizeZ = std::atoi(argv[11]);
	const BlobWorld B = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = *B.H;
	const cvxb::CopyWorld &W = B.W;
	const int n = (int)(placementBytes.size() / sizeof(cvx_copy_placement));
	const cvx_copy_placement *placements = reinterpret_cast<const cvx_copy_placement *>(placementBytes.data());
	// count, scan, write: what copy_count_kernel, cvxi::ExclusiveScan and copy_write_kernel do
	const int columns = sizeX * sizeZ;
	std::vector<uint32_t> headers(3 * (size_t)columns, 0u), pool;
	int over = 0;
	for (int i = 0; i < columns; i++) {
		const int64_t cx = x0 + i / sizeZ, cz = z0 + i % sizeZ;
		const cvxb::BrushResult r = cvxb::CopyColumn(W, placements, n, cx, cz, nullptr, nullptr);
		over |= r.overLimit ? 1 : 0;
		if (r.runCount == 0u) { continue; }
		const size_t off = pool.size();
		pool.resize(off + r.runCount + 2u + r.colours, 0u);
		cvxb::CopyColumn(W, placements, n, cx, cz, pool.data() + off + 1, pool.data() + off + r.runCount + 2u);
		headers[3 * (size_t)i] = (uint32_t)off;
		headers[3 * (size_t)i + 1] = r.runCount | (r.worldMin << 16);
		headers[3 * (size_t)i + 2] = r.worldMax;
	}
	headers.insert(headers.end(), pool.begin(), pool.end());
	std::printf("colorShift %d listed %lld over %d\n", H.colorShift, (long long)H.listedColumns, over);
	return WriteFile(argv[12], headers.data(), headers.size() * 4);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	const cvx_copy_placement ok{ { 0, 0, 0 }, { 1, 1, 1 }, { 2, 0, 0 }, 0, CVX_COPY_REPLACE, 0 };
	cvx_copy_placement badOp = ok, badMove = ok, badTransform = ok, empty = ok, negative = ok, far = ok;
	badOp.op = 4;
	badMove.move = 2;
	badTransform.transform = 16;
	empty.srcMax[1] = 0;
	negative.srcMin[2] = -1;
	far.dst[0] = (1 << 30) + 1;
	std::vector<cvx_copy_placement> many(CVX_COPY_MAX_PLACEMENTS + 1, ok);
	const int codes[] = {
		cvx_world_copy(nullptr, &ok, 1, 0, nullptr),
		cvx_world_copy(ctx, &ok, 0, 0, nullptr), cvx_world_copy(ctx, nullptr, 1, 0, nullptr), cvx_world_copy(ctx, many.data(), (int)many.size(), 0, nullptr),
		cvx_world_copy(ctx, &ok, 1, -1, nullptr), cvx_world_copy(ctx, &ok, 1, 6, nullptr), cvx_world_copy(ctx, &badOp, 1, 0, nullptr),
		cvx_world_copy(ctx, &badMove, 1, 0, nullptr), cvx_world_copy(ctx, &badTransform, 1, 0, nullptr), cvx_world_copy(ctx, &empty, 1, 0, nullptr),
		cvx_world_copy(ctx, &negative, 1, 0, nullptr), cvx_world_copy(ctx, &far, 1, 0, nullptr),
		cvx_world_copy(ctx, many.data(), CVX_COPY_MAX_PLACEMENTS, 5, nullptr), // valid: no world yet
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 13 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: copy_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <placements> <x0> <z0> <sizeX> <sizeZ> <out> | args\n");
	return 2;
}
