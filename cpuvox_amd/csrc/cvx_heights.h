// cvx_heights.h -- the rules of cvx_world_read_heights / cvx_world_write_heights (cvx_heights.hip): terrain as height maps out of and into the
// device-resident world.
//
// Written once for the device AND the host (tests/test_world_heights_cpu.py compiles it with g++ through tests/heights_rules.cpp and compares it
// with the numpy model of tests/heightsmodel.py):
//   HeightsBox     the footprint [x0, x0 + sizeX) x [z0, z0 + sizeZ) and the window [y0, y1); column (x, z) of it is element
//                  (x - x0) * sizeZ + (z - z0) of the arrays
//   HeightsSpan    a footprint column's [b, H) and its two colours, read from the arrays (the neighbour rule of include/cpuvox_gpu_heights.h included)
//   HeightsTop     the read: the highest solid voxel of a column inside the window, its colour, and how far down the solid goes from it
//   HeightsColumn  a column after a write, emitted as BrushColumn emits it (the builder's encoding).  The write is DEFINED as
//                  cvx_world_write_voxels of the expanded arrays: the bytes must equal cvxb::DenseColumn's on them.  The walk goes span by
//                  span (the shape of BrushColumnOver): between the boundaries of the arena's runs, of the window and of [b, H) every voxel
//                  has the same fate.
// Every read is from the arena as it is before the call: nothing writes it before cvxi::EditFromDevice takes the new columns.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu_heights.h"
#include "cvx_copy.h"

namespace cvxb {

struct HeightsBox {
	int32_t x0, z0;
	int32_t sizeX, sizeZ; // > 0, sizeX * sizeZ < 2^31
	int32_t y0, y1;       // the window, y0 < y1
};

// The arrays of a write and how they are read
struct HeightsArrays {
	const int32_t *heights;
	const uint32_t *argb;     // null: a CARVE that needs no colours
	const uint32_t *sideArgb; // null: argb all the way down
	int thickness;            // 0: solid down to y0; t: a crust of t voxels, thicker at cliffs
	int flags;                // CVX_HEIGHTS_*
};

struct HeightsInterval {
	int64_t b, H;       // the set voxels of the column: b <= y < H (unclipped by the world; y0 <= b <= H <= y1)
	uint32_t top, side; // the colour of voxel H - 1 and of the ones below it
};

CVX_HD inline int64_t HeightsClamp(const HeightsBox &box, int32_t h) { return h < box.y0 ? box.y0 : (h > box.y1 ? box.y1 : h); }

// Column (bx, bz) of the footprint (0 <= bx < sizeX, 0 <= bz < sizeZ): at most five loads of the heights, adjacent in z and in rows.
CVX_HD inline HeightsInterval HeightsSpan(const HeightsBox &box, const HeightsArrays &A, int64_t bx, int64_t bz)
{
	const int64_t at = bx * box.sizeZ + bz;
	HeightsInterval s;
	s.H = HeightsClamp(box, A.heights[at]);
	s.b = box.y0;
	if (A.thickness > 0) {
		// the lowest of the four edge neighbours; one outside the footprint counts as the column itself, or as y0 under WALLED
		const int64_t outside = (A.flags & CVX_HEIGHTS_WALLED) ? (int64_t)box.y0 : s.H;
		const int64_t n0 = bx > 0 ? HeightsClamp(box, A.heights[at - box.sizeZ]) : outside;
		const int64_t n1 = bx + 1 < box.sizeX ? HeightsClamp(box, A.heights[at + box.sizeZ]) : outside;
		const int64_t n2 = bz > 0 ? HeightsClamp(box, A.heights[at - 1]) : outside;
		const int64_t n3 = bz + 1 < box.sizeZ ? HeightsClamp(box, A.heights[at + 1]) : outside;
		int64_t low = s.H;
		low = n0 < low ? n0 : low;
		low = n1 < low ? n1 : low;
		low = n2 < low ? n2 : low;
		low = n3 < low ? n3 : low;
		const int64_t b = low - A.thickness;
		s.b = b > box.y0 ? b : (int64_t)box.y0;
	}
	s.top = A.argb ? A.argb[at] : 0u;
	s.side = A.sideArgb ? A.sideArgb[at] : s.top;
	return s;
}

struct HeightsRead {
	int32_t height; // 1 + the y of the highest solid voxel in the window; y0: none
	uint32_t argb;  // that voxel's colour word; 0: none
	int32_t bottom; // the lowest b >= max(y0, 0) with [b, height) all solid; y0: none
};

// Column (x, z), anywhere: outside the world it holds nothing.  One binary search of the column's runs, no voxel scan.
CVX_HD inline HeightsRead HeightsTop(const CopyWorld &W, const HeightsBox &box, int64_t x, int64_t z)
{
	const HeightsRead none{ box.y0, 0u, box.y0 };
	const int64_t lo = box.y0 < 0 ? 0 : box.y0, hi = box.y1 > W.dimY ? W.dimY : box.y1;
	if (x < 0 || x >= W.dimX || z < 0 || z >= W.dimZ || lo >= hi) { return none; }
	const ArenaColumn col = CopyColumnAt(W, x, z);
	const uint32_t count = col.Count();
	uint32_t at = RunAtOrBelow(col, hi - 1);
	if (at >= count) { return none; }
	SolidRun run = col.Run(at);
	const int64_t height = (int64_t)run.top < hi ? (int64_t)run.top : hi;
	if (height <= lo) { return none; }
	HeightsRead r;
	r.height = (int32_t)height;
	r.argb = W.colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - (uint32_t)height)) << (W.colorShift - 2))];
	int64_t bottom = run.bottom;
	while (bottom > lo && at + 1u < count) { // (runs of a foreign encoding may touch: the solid goes on through them)
		run = col.Run(at + 1u);
		if ((int64_t)run.top != bottom) { break; }
		bottom = run.bottom;
		at++;
	}
	r.bottom = (int32_t)(bottom > lo ? bottom : lo);
	return r;
}

// Walks the column (cx, cz) top-down after the write (the contract in include/cpuvox_gpu_heights.h, cvx_world_write_heights).  Inside the footprint and
// the window [y0, y1) a voxel is SET iff b <= y < H; the op decides as in the dense write: REPLACE -> set ? solid : air, FILL: set -> solid,
// CARVE: set -> air, PAINT: set and solid -> recoloured; everything else is the arena's.  A column outside the footprint is the arena's,
// re-emitted.  The span below y ends at the next boundary of an arena run, of the window or of [b, H).
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult HeightsColumn(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const HeightsBox &box, const HeightsArrays &A,
                                        int op, int64_t cx, int64_t cz, int dimY, uint32_t *outRuns, uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	// the window and the set interval of this column, clipped to the world; empty ones never match
	int64_t winLo = 0, winHi = 0, setLo = 0, setHi = 0, cap = -1;
	uint32_t topColour = 0u, sideColour = 0u;
	const int64_t bx = cx - box.x0, bz = cz - box.z0;
	if (bx >= 0 && bx < box.sizeX && bz >= 0 && bz < box.sizeZ) {
		const HeightsInterval s = HeightsSpan(box, A, bx, bz);
		winLo = box.y0 < 0 ? 0 : box.y0;
		winHi = box.y1 > dimY ? dimY : box.y1;
		setLo = s.b < 0 ? 0 : s.b;
		setHi = s.H > dimY ? dimY : s.H;
		cap = s.H - 1; // the voxel that takes argb (outside the world when H is)
		topColour = s.top;
		sideColour = s.side;
	}
	const bool window = winLo < winHi, interval = window && setLo < setHi;
	const uint32_t solidRuns = col.Count();
	uint32_t k = 0;                      // the arena run at or below y
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0; // the run being emitted
	int64_t lowest = -1, highest = -1;   // solid voxels
	int64_t y = (int64_t)dimY - 1;
	while (y >= 0) {
		// the arena: solid run k or the air above it
		while (k < solidRuns && (int64_t)col.Run(k).bottom > y) { k++; }
		SolidRun run{ 0u, 0u, 0u };
		bool origSolid = false;
		int64_t bottom = 0;
		if (k < solidRuns) {
			run = col.Run(k);
			origSolid = (int64_t)run.top > y;
			bottom = origSolid ? (int64_t)run.bottom : (int64_t)run.top;
		}
		bool inWindow = false, set = false;
		if (window) {
			if (winLo <= y && y < winHi) {
				inWindow = true;
				bottom = winLo > bottom ? winLo : bottom;
			} else if (winHi <= y) {
				bottom = winHi > bottom ? winHi : bottom;
			}
		}
		if (interval) {
			if (setLo <= y && y < setHi) {
				set = true;
				bottom = setLo > bottom ? setLo : bottom;
			} else if (setHi <= y) {
				bottom = setHi > bottom ? setHi : bottom;
			}
		}
		bool solid = origSolid, painted = false;
		if (op == CVX_COPY_REPLACE) {
			if (inWindow) { solid = set; painted = set; }
		} else if (set) {
			if (op == CVX_BRUSH_FILL) { solid = true; painted = true; }
			else if (op == CVX_BRUSH_CARVE) { solid = false; }
			else { painted = origSolid; }
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
					outColours[res.colours + (uint32_t)(y - v)] = painted ? (v == cap ? topColour : sideColour)
					                                                        : colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - (uint32_t)v)) << (colorShift - 2))];
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
