// cvx_dense.h -- the rules of cvx_world_read_voxels / cvx_world_write_voxels (cvx_dense.hip): dense voxel boxes out of and into the
// device-resident world.
//
// Written once for the device AND the host (tests/test_world_dense_cpu.py compiles it with g++ through tests/dense_rules.cpp and compares it with
// the dense numpy model of tests/densemodel.py):
//   DenseBox      the box [min, min + size) and where voxel (x, y, z) of it lies in the arrays: ((x - min.x) * size.z + (z - min.z)) * size.y + (y - min.y)
//   ArenaVoxel    what the arena holds at height y of a column (a binary search of its runs)
//   DenseVoxel    what one box voxel reads as: the arena's voxel inside the world, air outside it
//   DenseFinal    what a voxel of a column is after a write: the op applied to the dense arrays inside the box, the arena elsewhere
//   DenseColumn   a column after a write, emitted as BrushColumn emits it (the builder's encoding).  This scalar walk, a voxel at a time, is the
//                 specification: the wave-wide kernels of cvx_dense.hip evaluate DenseFinal per lane and must give the same bytes.
// Every read is from the arena as it is before the call: nothing writes it before cvxi::EditFromDevice takes the new columns.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_box.h"
#include "cvx_copy.h"

namespace cvxb {

struct DenseBox {
	int32_t min[3];
	int32_t size[3]; // > 0, size[0] * size[1] * size[2] < 2^31
};

// The box of a call that hands out a value per voxel: given, within +-2^30, no empty axis, fewer than 2^31 voxels (BoxCheck's return and message).
// *elements receives its voxels.
inline int DenseBoxCheck(const int32_t boxMin[3], const int32_t boxMax[3], DenseBox *box, int64_t *elements, char *message, size_t size)
{
	const int rc = BoxCheck(boxMin, boxMax, kBoxWithin | kBoxVoxels, message, size);
	*elements = 1;
	for (int a = 0; a < 3 && rc == 0; a++) {
		box->min[a] = boxMin[a];
		box->size[a] = boxMax[a] - boxMin[a];
		*elements *= box->size[a];
	}
	return rc;
}

struct Voxel {
	bool solid;
	uint32_t argb; // 0 for air
};

// Height y (0 <= y < dimY) of a column of the arena.
CVX_HD inline Voxel ArenaVoxel(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, int64_t y)
{
	const uint32_t count = col.Count(), at = RunAtOrBelow(col, y);
	if (at < count) {
		const SolidRun run = col.Run(at);
		if ((int64_t)run.top > y) {
			return Voxel{ true, colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - (uint32_t)y)) << (colorShift - 2))] };
		}
	}
	return Voxel{ false, 0u };
}

// What voxel (x, y, z) reads as: everything outside the world is air.
CVX_HD inline Voxel DenseVoxel(const CopyWorld &W, int64_t x, int64_t y, int64_t z)
{
	if (x < 0 || x >= W.dimX || y < 0 || y >= W.dimY || z < 0 || z >= W.dimZ) { return Voxel{ false, 0u }; }
	return ArenaVoxel(CopyColumnAt(W, x, z), W.colourSlots, W.colorShift, y);
}

// The box's part of column (cx, cz): whether the box covers it, its y interval [*lo, *hi) clipped to [0, dimY), and *base such that voxel y of
// it is element *base + y of the arrays.
CVX_HD inline bool DenseSpan(const DenseBox &box, int64_t cx, int64_t cz, int64_t dimY, int64_t *lo, int64_t *hi, int64_t *base)
{
	const int64_t bx = cx - box.min[0], bz = cz - box.min[2];
	*lo = *hi = *base = 0;
	if (bx < 0 || bx >= box.size[0] || bz < 0 || bz >= box.size[2]) { return false; }
	const int64_t l = box.min[1], h = (int64_t)box.min[1] + box.size[1];
	*lo = l < 0 ? 0 : l;
	*hi = h > dimY ? dimY : h;
	*base = (bx * box.size[2] + bz) * box.size[1] - box.min[1];
	return *lo < *hi;
}

// Voxel y of a column after the write; `inBox`: the box covers it, `at` its element of the arrays (the contract in include/cpuvox_gpu.h,
// cvx_world_write_voxels).  A voxel is SET iff solid[at] != 0 when there is a mask, else iff argb[at] != 0; argb may be null for a CARVE.
CVX_HD inline Voxel DenseFinal(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, bool inBox, int64_t at, const uint32_t *argb,
                               const uint8_t *solid, int op, int64_t y)
{
	if (inBox) {
		const uint32_t c = argb ? argb[at] : 0u;
		const bool set = solid ? solid[at] != 0 : c != 0u;
		if (op == CVX_COPY_REPLACE) { return Voxel{ set, set ? c : 0u }; }
		if (set) {
			if (op == CVX_BRUSH_FILL) { return Voxel{ true, c }; }
			if (op == CVX_BRUSH_CARVE) { return Voxel{ false, 0u }; }
			return ArenaVoxel(col, colourSlots, colorShift, y).solid ? Voxel{ true, c } : Voxel{ false, 0u }; // PAINT
		}
	}
	return ArenaVoxel(col, colourSlots, colorShift, y);
}

// Walks the column (cx, cz) top-down, a voxel at a time, after the write.
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult DenseColumn(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const DenseBox &box, const uint32_t *argb,
                                      const uint8_t *solid, int op, int64_t cx, int64_t cz, int dimY, uint32_t *outRuns, uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	int64_t lo, hi, base;
	DenseSpan(box, cx, cz, dimY, &lo, &hi, &base);
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0; // the run being emitted
	int64_t lowest = -1, highest = -1;   // solid voxels
	for (int64_t y = (int64_t)dimY - 1; y >= 0; y--) {
		const Voxel v = DenseFinal(col, colourSlots, colorShift, lo <= y && y < hi, base + y, argb, solid, op, y);
		if (v.solid != curSolid || curLength == 0) {
			if (curLength > 0) {
				if (outRuns) { outRuns[res.runCount] = (curSolid ? (uint32_t)curIndex : 0xFFFFu) | ((uint32_t)curLength << 16); }
				if (curLength > 32767) { res.overLimit = true; }
				res.runCount++;
			}
			curSolid = v.solid;
			curLength = 0;
			curIndex = res.colours;
			if (v.solid && curIndex > 32767) { res.overLimit = true; }
		}
		curLength++;
		if (v.solid) {
			if (outColours) { outColours[res.colours] = v.argb; }
			res.colours++;
			if (highest < 0) { highest = y + 1; }
			lowest = y;
		}
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

// ---- the same column 64 voxels at a time (cvx_dense.hip's wave; tests/dense_rules.cpp runs the steps on the host, lane after lane) ------------
// A step covers the voxels yTop - l, l = 0 .. valid - 1 (lane l, bit l of the masks).  `mask`: the solid ones (DenseFinal per lane, a ballot on
// the device).  A lane STARTS a run when its voxel differs from the one above it, the column's top voxel always does; a run that starts and
// ends inside the step is written by its start lane (DenseLaneRun), the run that is open at the end of a step is carried in DenseWalk and
// written by whoever passes outRuns to DenseAdvance / DenseAdvanceAir / DenseFinish (one lane) when a later step, or the column, ends it.

struct DenseWalk {
	uint32_t runs = 0u, colours = 0u; // so far
	int32_t lowest = -1, highest = -1; // solid voxels
	bool overLimit = false;
	bool openSolid = false;           // the open run: its kind, colour index and length so far (0: before the first step)
	uint32_t openIndex = 0u, openLength = 0u;
};

CVX_HD inline uint32_t DenseRunWord(bool solid, uint32_t index, uint32_t length) { return (solid ? index : 0xFFFFu) | (length << 16); }

// How many steps from the one at yTop on hold nothing but air whatever the op; 0: the step [yTop - 63, yTop] has to be evaluated.  The highest
// voxel at or below yTop that can be solid is the top of the box's span [lo, hi) of the column or of a run of the arena: *k is a cursor into the
// column's `count` runs, 0 before the first step; the steps go down and it only advances, to the first run whose bottom is at or below yTop.
// The wave takes the air steps in one go (DenseAdvanceAir): a tall column of a thin-shelled world costs its few live steps, not its height.
CVX_HD inline int DenseAirSteps(const ArenaColumn &col, uint32_t count, uint32_t *k, int64_t lo, int64_t hi, int yTop)
{
	while (*k < count && (int64_t)col.Run(*k).bottom > yTop) { (*k)++; }
	int64_t next = -1;
	if (*k < count) {
		const int64_t top = (int64_t)col.Run(*k).top - 1;
		next = top < yTop ? top : yTop;
	}
	if (lo < hi && lo <= yTop) {
		const int64_t top = hi - 1 < yTop ? hi - 1 : yTop;
		next = top > next ? top : next;
	}
	if (next > (int64_t)yTop - 64) { return 0; }
	const int steps = (int)((yTop - next) / 64), left = yTop / 64 + 1;
	return steps < left ? steps : left;
}

CVX_HD inline uint64_t DenseStarts(const DenseWalk &w, uint64_t mask, uint32_t valid)
{
	const uint64_t validMask = valid >= 64u ? ~0ull : (1ull << valid) - 1ull;
	const uint64_t starts = (mask ^ ((mask << 1) | (w.openSolid ? 1ull : 0ull))) & validMask;
	return w.openLength == 0u ? starts | 1ull : starts;
}

// Lane `lane` of the step, before DenseAdvance: startsBelow / solidBelow = the bits of starts / mask below the lane (prefix popcounts).
CVX_HD inline void DenseLaneRun(const DenseWalk &w, uint64_t mask, uint64_t starts, int lane, uint32_t startsBelow, uint32_t solidBelow, uint32_t *outRuns)
{
	if (((starts >> lane) & 1ull) == 0ull) { return; }
	const uint64_t rest = lane >= 63 ? 0ull : starts >> (lane + 1);
	if (rest == 0ull) { return; } // the step's last start: its run stays open
	outRuns[w.runs + startsBelow] = DenseRunWord(((mask >> lane) & 1ull) != 0ull, w.colours + solidBelow, 1u + (uint32_t)__builtin_ctzll(rest));
}

// The step's wave-uniform part.  outRuns: null in every lane but the one that writes the run the step ends.
CVX_HD inline void DenseAdvance(DenseWalk &w, uint64_t mask, uint64_t starts, uint32_t valid, int yTop, uint32_t *outRuns)
{
	if (starts != 0ull) {
		const uint32_t first = (uint32_t)__builtin_ctzll(starts), last = 63u - (uint32_t)__builtin_clzll(starts);
		if (w.openLength > 0u) { // the open run ends at this step's first start
			const uint32_t length = w.openLength + first;
			if (outRuns) { outRuns[w.runs - 1u] = DenseRunWord(w.openSolid, w.openIndex, length); }
			if (length > 32767u) { w.overLimit = true; }
		}
		const uint64_t solidStarts = starts & mask; // colour indices grow with the lane: the last solid start has the largest
		if (solidStarts != 0ull) {
			const uint32_t at = 63u - (uint32_t)__builtin_clzll(solidStarts);
			if (w.colours + (uint32_t)__builtin_popcountll(mask & ((1ull << at) - 1ull)) > 32767u) { w.overLimit = true; }
		}
		w.openSolid = ((mask >> last) & 1ull) != 0ull;
		w.openIndex = w.colours + (uint32_t)__builtin_popcountll(mask & ((1ull << last) - 1ull));
		w.openLength = valid - last;
		w.runs += (uint32_t)__builtin_popcountll(starts);
	} else {
		w.openLength += valid;
	}
	if (mask != 0ull) {
		if (w.highest < 0) { w.highest = yTop - (int32_t)__builtin_ctzll(mask) + 1; }
		w.lowest = yTop - (63 - (int32_t)__builtin_clzll(mask));
	}
	w.colours += (uint32_t)__builtin_popcountll(mask);
}

// DenseAdvance for `voxels` voxels of air, however many steps they span: they continue an open air run, or end a solid one and start theirs.
CVX_HD inline void DenseAdvanceAir(DenseWalk &w, uint32_t voxels, uint32_t *outRuns)
{
	if (w.openLength > 0u && !w.openSolid) {
		w.openLength += voxels;
		return;
	}
	if (w.openLength > 0u) {
		if (outRuns) { outRuns[w.runs - 1u] = DenseRunWord(true, w.openIndex, w.openLength); }
		if (w.openLength > 32767u) { w.overLimit = true; }
	}
	w.openSolid = false;
	w.openIndex = w.colours;
	w.openLength = voxels;
	w.runs++;
}

// After the last step: the open run ends with the column; the result is DenseColumn's.
CVX_HD inline BrushResult DenseFinish(DenseWalk &w, uint32_t *outRuns)
{
	if (w.openLength > 0u) {
		if (outRuns) { outRuns[w.runs - 1u] = DenseRunWord(w.openSolid, w.openIndex, w.openLength); }
		if (w.openLength > 32767u) { w.overLimit = true; }
	}
	if (w.colours == 0u) { return BrushResult{ 0u, 0u, 0u, 0u, false }; } // the empty column: RunCount 0, no elements
	return BrushResult{ w.runs, w.colours, (uint32_t)w.lowest & 0xFFFFu, (uint32_t)w.highest & 0xFFFFu, w.overLimit || w.runs > 65535u };
}

} // namespace cvxb
