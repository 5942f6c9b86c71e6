// cvx_copy.h -- the column rule of cvx_world_copy (cvx_copy.hip): copying, moving and rotating voxel boxes inside the device-resident world.
//
// Written once for the device AND the host (tests/test_world_copy_cpu.py compiles it with g++ through tests/copy_rules.cpp and compares it with
// the dense numpy model of tests/copymodel.py):
//   CopyWorld         LOD 0 of the arena: records, run list and colours, so that any column can be read as a cvxb::ArenaColumn
//   CopySourceColumn  T^-1 of a placement on (x, z): the source column a destination column reads
//   CopyColumn        a column after a list of placements, emitted as BrushColumn emits it (the builder's encoding)
// Every read is from the arena as it is before the call (the snapshot): nothing writes it before cvxi::EditFromDevice takes the new columns.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_brush.h"

namespace cvxb {

struct CopyWorld {
	const uint32_t *records;     // LOD 0's records (4 words each), row-major with 2^rowShift per row
	const uint32_t *runs;        // the level's run list, 2 words per entry
	const uint32_t *colourSlots; // the colour array, 4-byte slots
	int rowShift, colorShift;
	int dimX, dimY, dimZ;
};

CVX_HD inline ArenaColumn CopyColumnAt(const CopyWorld &W, int64_t x, int64_t z)
{
	const Record r = *reinterpret_cast<const Record *>(W.records + 4 * ((x << W.rowShift) + z));
	return ArenaColumn{ r.x, r.y, r.z, r.w, W.runs };
}

// The destination box's extent in X and Z: an odd number of quarter turns swaps the source's.
CVX_HD inline void CopyDestinationSize(const cvx_copy_placement &p, int64_t *sizeX, int64_t *sizeZ)
{
	const int64_t a = (int64_t)p.srcMax[0] - p.srcMin[0], b = (int64_t)p.srcMax[2] - p.srcMin[2];
	const bool odd = (p.transform & 1) != 0;
	*sizeX = odd ? b : a;
	*sizeZ = odd ? a : b;
}

// T^-1 on the column: the source column (*outX, *outZ) destination column (cx, cz) reads; false: the destination box does not cover (cx, cz).
// The turns are undone last first, each one (p, r, sx, sz) <- (r, sx-1-p, sz, sx) on the turned sizes, then the mirror.
CVX_HD inline bool CopySourceColumn(const cvx_copy_placement &p, int64_t cx, int64_t cz, int64_t *outX, int64_t *outZ)
{
	int64_t sx, sz;
	CopyDestinationSize(p, &sx, &sz);
	int64_t u = cx - p.dst[0], r = cz - p.dst[2];
	if (u < 0 || u >= sx || r < 0 || r >= sz) { return false; }
	for (int t = 0; t < (p.transform & 3); t++) {
		const int64_t nu = r, nr = sx - 1 - u, s = sx;
		u = nu;
		r = nr;
		sx = sz;
		sz = s;
	}
	if (p.transform & 4) { u = sx - 1 - u; }
	*outX = p.srcMin[0] + u;
	*outZ = p.srcMin[2] + r;
	return true;
}

CVX_HD inline bool CopyMovesColumn(const cvx_copy_placement &p, int64_t cx, int64_t cz)
{
	return p.move != 0 && cx >= p.srcMin[0] && cx < p.srcMax[0] && cz >= p.srcMin[2] && cz < p.srcMax[2];
}

// The first run (0 = the top one) whose bottom is at or below y: runs 0 .. k-1 lie wholly above y.  Bottoms fall with k: a binary search.
CVX_HD inline uint32_t RunAtOrBelow(const ArenaColumn &col, int64_t y)
{
	uint32_t lo = 0, hi = col.Count();
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if ((int64_t)col.Run(mid).bottom > y) { lo = mid + 1u; } else { hi = mid; }
	}
	return lo;
}

// Walks the column (cx, cz) top-down after the `n` placements (the contract in include/cpuvox_gpu.h, cvx_world_copy).  Within a y span where
// the column's own runs, the moving placements' source intervals, the covering placements' destination intervals and the solid / air state of
// every covering placement's source voxel do not change, every voxel has the same fate (solid or air, and which column's voxel gives its
// colour): the walk goes span by span, the span ending at the next of those boundaries below y.  A covering placement's source voxel is found
// with a binary search of its source column's runs, so a column costs spans x covering placements, not voxels.
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult CopyColumn(const CopyWorld &W, const cvx_copy_placement *pl, int n, int64_t cx, int64_t cz, uint32_t *outRuns,
                                     uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	// the placements that can touch the column: first .. last (integer compares on the footprints)
	int first = n, last = -1;
	for (int i = 0; i < n; i++) {
		int64_t sx, sz;
		if (CopyMovesColumn(pl[i], cx, cz) || CopySourceColumn(pl[i], cx, cz, &sx, &sz)) {
			first = first < i ? first : i;
			last = i;
		}
	}
	const ArenaColumn own = CopyColumnAt(W, cx, cz);
	const uint32_t solidRuns = own.Count();
	const int64_t dimY = W.dimY;
	uint32_t k = 0;                      // the column's own run at or below y
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0; // the run being emitted
	int64_t lowest = -1, highest = -1;   // solid voxels
	int64_t y = dimY - 1;
	while (y >= 0) {
		// the column itself: solid run k or the air above it
		while (k < solidRuns && (int64_t)own.Run(k).bottom > y) { k++; }
		SolidRun run{ 0u, 0u, 0u };
		bool solid = false;
		int64_t bottom = 0;
		if (k < solidRuns) {
			run = own.Run(k);
			solid = (int64_t)run.top > y;
			bottom = solid ? (int64_t)run.bottom : (int64_t)run.top;
		}
		// where the colour of a solid span comes from: voxel fromBase + fromSign * v of fromCol's run fromRun
		ArenaColumn from = own;
		SolidRun fromRun = run;
		int64_t fromBase = 0, fromSign = 1;
		// 1. the moves carve their source boxes
		for (int i = first; i <= last; i++) {
			if (!CopyMovesColumn(pl[i], cx, cz)) { continue; }
			const int64_t lo = pl[i].srcMin[1], hi = pl[i].srcMax[1];
			if (lo <= y && y < hi) {
				solid = false;
				bottom = lo > bottom ? lo : bottom;
			} else if (hi <= y) {
				bottom = hi > bottom ? hi : bottom;
			}
		}
		// 2. the placements in order, each reading its source voxel from the snapshot
		for (int i = first; i <= last; i++) {
			const cvx_copy_placement &p = pl[i];
			int64_t sx, sz;
			if (!CopySourceColumn(p, cx, cz, &sx, &sz)) { continue; }
			const int64_t sizeY = (int64_t)p.srcMax[1] - p.srcMin[1];
			const int64_t lo = p.dst[1] > 0 ? (int64_t)p.dst[1] : 0, hi = (int64_t)p.dst[1] + sizeY < dimY ? (int64_t)p.dst[1] + sizeY : dimY;
			if (lo >= hi || y < lo) { continue; }
			if (hi <= y) {
				bottom = hi > bottom ? hi : bottom;
				continue;
			}
			bottom = lo > bottom ? lo : bottom;
			const bool flip = (p.transform & 8) != 0;
			const int64_t base = flip ? (int64_t)p.srcMax[1] - 1 + p.dst[1] : (int64_t)p.srcMin[1] - p.dst[1], sign = flip ? -1 : 1;
			const int64_t srcY = base + sign * y;
			const ArenaColumn src = CopyColumnAt(W, sx, sz);
			const uint32_t count = src.Count(), at = RunAtOrBelow(src, srcY);
			const SolidRun below = at < count ? src.Run(at) : SolidRun{ 0u, 0u, 0u };
			const bool srcSolid = at < count && (int64_t)below.top > srcY;
			// the voxels from srcY on, in the walk's direction through the source (down, or up when flipped), in the same state
			int64_t extent;
			if (!flip) {
				extent = srcY + 1 - (int64_t)(srcSolid ? below.bottom : below.top);
			} else if (srcSolid) {
				extent = (int64_t)below.top - srcY;
			} else {
				extent = (at > 0u ? (int64_t)src.Run(at - 1u).bottom : dimY) - srcY;
			}
			bottom = y + 1 - extent > bottom ? y + 1 - extent : bottom;
			if (!srcSolid) {
				if (p.op == CVX_COPY_REPLACE) { solid = false; }
				continue;
			}
			if (p.op == CVX_BRUSH_CARVE) {
				solid = false;
				continue;
			}
			if (p.op == CVX_BRUSH_PAINT && !solid) { continue; }
			solid = true; // REPLACE / FILL, or PAINT over a solid voxel
			from = src;
			fromRun = below;
			fromBase = base;
			fromSign = sign;
		}
		const int64_t length = y + 1 - bottom;
		if (solid != curSolid || curLength == 0) {
			if (curLength > 0) {
				if (outRuns) { outRuns[res.runCount] = (curSolid ? (uint32_t)curIndex : 0xFFFFu) | ((uint32_t)curLength << 16); }
				if (curLength > 32767) { res.overLimit = true; }
				res.runCount++;
			}
			curSolid = solid;
			curLength = 0;
			curIndex = res.colours;
			if (solid && curIndex > 32767) { res.overLimit = true; }
		}
		curLength += length;
		if (solid) {
			if (outColours) {
				for (int64_t v = y; v >= bottom; v--) {
					const uint32_t s = (uint32_t)(fromBase + fromSign * v);
					outColours[res.colours + (uint32_t)(y - v)] = W.colourSlots[from.ColorsBase() + ((fromRun.colorsIndex + (fromRun.top - 1u - s)) << (W.colorShift - 2))];
				}
			}
			res.colours += (uint32_t)length;
			if (highest < 0) { highest = y + 1; }
			lowest = bottom;
		}
		y = bottom - 1;
	}
	if (curLength > 0) {
		if (outRuns) { outRuns[res.runCount] = (curSolid ? (uint32_t)curIndex : 0xFFFFu) | ((uint32_t)curLength << 16); }
		if (curLength > 32767) { res.overLimit = true; }
		res.runCount++;
	}
	if (res.colours == 0u) { // the empty column: RunCount 0, no elements
		res.runCount = 0u;
		res.overLimit = false;
		return res;
	}
	if (res.runCount > 65535u) { res.overLimit = true; }
	res.worldMin = (uint32_t)lowest & 0xFFFFu;
	res.worldMax = (uint32_t)highest & 0xFFFFu;
	return res;
}

} // namespace cvxb
