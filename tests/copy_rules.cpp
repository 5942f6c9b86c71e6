// Host build of the copy rule (cpuvox_amd/csrc/cvx_copy.h) for tests/test_world_copy_cpu.py.
//   copy_rules columns <cases in> <results out>
//     Each case is a small world of gx x gz columns in the reference's layout plus a placement list (int32 words): dimY gx gz stride, per column
//     (x-major) colorsBase runCount (colorsIndex length)* colourCount colour*, then placementCount and the placements (cvx_copy_placement, 12 words
//     each).  Every column gets its record from the edit's record rule (cvx_edit.h; a listed column its run-list block), its colours at
//     colorsBase + k * stride, and every column of the world goes through cvxb::CopyColumn.  Out per case and column: overLimit runCount colours
//     worldMin worldMax, then (unless over the limits) the runs and the colours.
//   copy_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <placements> <x0> <z0> <sizeX> <sizeZ> <blob out>
//     Uploads the LOD-0 blob into a context that never touches a device (cvx_world_upload lays the level out on the host), runs cvxb::CopyColumn
//     on every column of the rectangle and writes the sub-world blob cvx_copy.hip's write kernel makes (12-byte headers, then the element pool).
//   copy_rules args
//     cvx_world_copy's argument checks on a context without a device or world: one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_copy.h"

static std::vector<uint8_t> ReadFile(const char *path)
{
	std::vector<uint8_t> out;
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::exit(2); }
	for (int c; (c = std::fgetc(f)) != EOF;) { out.push_back((uint8_t)c); }
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

static int Columns(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		const int dimY = *p++, gx = *p++, gz = *p++, stride = *p++;
		int rowShift = 0;
		while ((1 << rowShift) < gz) { rowShift++; }
		std::vector<uint4> records((size_t)gx << rowShift, uint4{ 0u, 0u, 0u, 0u });
		std::vector<uint32_t> runs(8, 0u), slots(64, 0u);
		for (int c = 0; c < gx * gz; c++) {
			const int colorsBase = *p++, runCount = *p++;
			// the column as a blob: header {0, runCount | worldMin << 16, worldMax}, elements [guard][runs][guard]
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
			if (slots.size() < (size_t)colorsBase + (size_t)stride * (colourCount + 1) + 64) { slots.resize((size_t)colorsBase + (size_t)stride * (colourCount + 1) + 64, 0u); }
			for (int k = 0; k < colourCount; k++) { slots[(size_t)colorsBase + (size_t)k * stride] = (uint32_t)*p++; }
			const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)(lowest < 0 ? 0 : lowest) << 16), (uint32_t)(highest < 0 ? 0 : highest) };
			uint4 rec{ 0u, 0u, 0u, 0u };
			if (runCount > 0) {
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
		const int n = *p++;
		std::vector<cvx_copy_placement> placements((size_t)n);
		std::memcpy(placements.data(), p, (size_t)n * sizeof(cvx_copy_placement));
		p += (size_t)n * sizeof(cvx_copy_placement) / 4;
		cvxb::CopyWorld W;
		W.records = reinterpret_cast<const uint32_t *>(records.data());
		W.runs = runs.data();
		W.colourSlots = slots.data();
		W.rowShift = rowShift;
		W.colorShift = stride == 1 ? 2 : 7;
		W.dimX = gx;
		W.dimY = dimY;
		W.dimZ = gz;
		for (int c = 0; c < gx * gz; c++) {
			const int64_t cx = c / gz, cz = c % gz;
			const cvxb::BrushResult r = cvxb::CopyColumn(W, placements.data(), n, cx, cz, nullptr, nullptr);
			out.push_back(r.overLimit ? 1u : 0u);
			out.push_back(r.runCount);
			out.push_back(r.colours);
			out.push_back(r.worldMin);
			out.push_back(r.worldMax);
			if (!r.overLimit) {
				std::vector<uint32_t> newRuns(r.runCount + 1u), newColours(r.colours + 1u);
				const cvxb::BrushResult again = cvxb::CopyColumn(W, placements.data(), n, cx, cz, newRuns.data(), newColours.data());
				if (again.runCount != r.runCount || again.colours != r.colours) { return 3; }
				out.insert(out.end(), newRuns.begin(), newRuns.begin() + r.runCount);
				out.insert(out.end(), newColours.begin(), newColours.begin() + r.colours);
			}
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static int World(char **argv)
{
	std::vector<uint8_t> blob = ReadFile(argv[2]);
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	const std::vector<uint8_t> placementBytes = ReadFile(argv[7]);
	const int x0 = std::atoi(argv[8]), z0 = std::atoi(argv[9]), sizeX = std::atoi(argv[10]), sizeZ = std::atoi(argv[11]);
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
