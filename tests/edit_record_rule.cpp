// Host build of the edit kernels' record rule (cpuvox_amd/csrc/cvx_edit.h) against what cvx_world_upload writes (tests/test_world_edit_cpu.py).
// Usage: edit_record_rule <blob file> <dimX> <dimY> <dimZ> <lod> <columnCount>.  Uploads the blob into a context that never touches a device
// (cvx_world_upload lays the level out on the host) and compares, column by column, the words the rule builds with the upload's: the record
// apart from colorsBase and a listed column's run-list block, the counts entry, the run-list block's entries, and the colours / run-list entries
// the edit reads back from a record.  Prints "columns <n> listed <m> mismatches <k>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rules_world.h"

int main(int argc, char **argv)
{
	if (argc != 7) { std::fprintf(stderr, "usage\n"); return 2; }
	const std::vector<uint8_t> blob = ReadFile(argv[1]);
	const int dimX = std::atoi(argv[2]), dimY = std::atoi(argv[3]), dimZ = std::atoi(argv[4]), lod = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	cvx_context *ctx = new cvx_context();
	if (lod > 0) { // (upload checks the other levels against LOD 0's dimensions)
		ctx->levelSet[0] = true;
		ctx->hostWorld.dimX = dimX;
		ctx->hostWorld.dimY = dimY;
		ctx->hostWorld.dimZ = dimZ;
	}
	UploadBlobLevel(ctx, lod, blob, dimX, dimY, dimZ, columnCount);
	const cvx_context::HostLevel &H = ctx->hostLevel[lod];
	const uint32_t *headers = reinterpret_cast<const uint32_t *>(blob.data());
	const uint32_t *elements = reinterpret_cast<const uint32_t *>(blob.data() + (size_t)columnCount * 12);
	const uint32_t *runs = reinterpret_cast<const uint32_t *>(H.runs.data());
	const int usedX = dimX >> lod, usedZ = dimZ >> lod;
	long columns = 0, listed = 0, bad = 0;
	for (int x = 0; x < usedX; x++) {
		for (int z = 0; z < usedZ; z++) {
			const uint32_t *h = headers + 3 * ((size_t)x * usedZ + z);
			const size_t at = ((size_t)x << H.rowShift) + (size_t)z;
			const uint4 r = H.records[at];
			const uint2 n = H.counts[at];
			const cvxe::ColumnWords c = cvxe::BuildColumnWords(h, elements, lod, dimY);
			const bool isListed = r.x != 0u && (r.x >> 30) == 0u;
			bool ok = (r.x & 0xC0000000u) == c.x && r.y == c.y && r.w == c.w && (isListed || r.z == c.z) && n.x == c.c0 && n.y == c.c1;
			if ((h[1] & 0xFFFFu) != 0u) {
				columns++;
				ok = ok && (r.x & 0x3FFFFFFFu) != 0u;
				if (isListed) {
					listed++;
					std::vector<uint32_t> block(2 * (size_t)c.solid + 2, 0u);
					cvxe::BuildListedRuns(h, elements, lod, dimY, block.data());
					for (uint32_t k = 0; k < 2 * c.solid; k++) { ok = ok && runs[2 * (size_t)r.z + k] == block[k]; }
				}
				ok = ok && cvxe::RecordColours(r.x, r.y, r.z, r.w, runs, lod) == c.colours;
				ok = ok && cvxe::RecordRunEntries(r.x, r.w) == (isListed ? ((c.solid + 1u) & ~1u) : 0u);
				// the colours the rule counts are the ones the upload placed (stride: the level's colour layout)
				const uint32_t base = r.x & 0x3FFFFFFFu, stride = H.colorShift == 7 ? CVX_COLOR_STRIDE : 1u;
				const uint32_t src = h[0] + (h[1] & 0xFFFFu) + 2u;
				for (uint32_t k = 0; k < c.colours; k++) { ok = ok && H.elements[base + (size_t)k * stride] == elements[src + k]; }
			} else {
				ok = ok && r.x == 0u && r.y == 0u && r.z == 0u && r.w == 0u;
			}
			if (!ok) {
				if (bad < 5) { std::printf("column (%d, %d): record %08x %08x %08x %08x, rule %08x %08x %08x %08x\n", x, z, r.x, r.y, r.z, r.w, c.x, c.y, c.z, c.w); }
				bad++;
			}
		}
	}
	std::printf("columns %ld listed %ld mismatches %ld\n", columns, listed, bad);
	delete ctx;
	return bad ? 1 : 0;
}
