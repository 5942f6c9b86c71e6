// cvx_settle.h -- the rules of cvx_world_settle (cvx_settle.hip): the floating pieces of the device-resident world fall until they rest.
//
// Written once for the device AND the host (tests/test_world_settle_cpu.py compiles it with g++ through tests/settle_rules.cpp, drives it with a
// sequential union-find and a Bellman-Ford and compares it with the dense step-by-step model of tests/settlemodel.py):
//   SettleBelow     one node's constraint: what the next solid voxel below it in its column is, and how much air lies between
//   SettleResolve   ... resolved with the pieces of the two nodes: static (a bound on the piece's drop), another floating piece (an edge of the
//                   piece graph), or the piece itself (no constraint)
//   SettleColumn    a column with its nodes moved down by their pieces' drops, emitted as PiecesRemoveColumn emits it (the builder's encoding)
// The nodes are those of cvx_pieces.h: a column's solid runs clipped to the box's y range, top-down.
#pragma once

#include <stdint.h>

#include "cvx_pieces.h"

namespace cvxb {

enum { SETTLE_STATIC = 0, SETTLE_NODE = 1, SETTLE_SELF = 2 };

struct SettleConstraint {
	uint32_t kind; // SETTLE_STATIC: `gap` bounds the drop; SETTLE_NODE: the node below it in the column (node j + 1) comes first, `gap` above it
	uint32_t gap;  // voxels of air between the node's lowest voxel and the next solid voxel below it
};

// Node j of the column's `nodes` nodes inside [y0, y1).  Below the last node comes whatever the column holds under the box -- the rest of the node's
// own run when the box's bottom cuts it (gap 0: the piece holds still), the next run, or the floor, which counts as static with gap = the node's lo.
CVX_HD inline SettleConstraint SettleBelow(const ArenaColumn &col, int64_t y0, int64_t y1, uint32_t j, uint32_t nodes)
{
	uint32_t first, end;
	PiecesRunRange(col, y0, y1, &first, &end);
	const uint32_t k = first + j;
	const SolidRun run = col.Run(k);
	if (j + 1u < nodes) { return SettleConstraint{ SETTLE_NODE, run.bottom - col.Run(k + 1u).top }; }
	if ((int64_t)run.bottom < y0) { return SettleConstraint{ SETTLE_STATIC, 0u }; }
	if (k + 1u < col.Count()) { return SettleConstraint{ SETTLE_STATIC, run.bottom - col.Run(k + 1u).top }; }
	return SettleConstraint{ SETTLE_STATIC, run.bottom };
}

// A SETTLE_NODE constraint of a node of piece `root` with the node below it: of piece `rootBelow`, which floats or not.
CVX_HD inline uint32_t SettleResolve(uint32_t kind, uint32_t root, uint32_t rootBelow, bool belowFloats)
{
	if (kind == SETTLE_STATIC || !belowFloats) { return SETTLE_STATIC; }
	return root == rootBelow ? SETTLE_SELF : SETTLE_NODE;
}

// Column (cx, cz) with node j moved down by drop[j] voxels (0: it stays; the column has `nodes` nodes inside [y0, y1); a column outside the box has
// none), emitted as PiecesRemoveColumn emits it: maximal runs from the top, colours verbatim, runs that come to touch merged.  The walk goes
// top-down over the column's runs; a run that is a node is cut at the box's y range and only the part inside it moves.  The drops of a settle
// keep the vertical order of a column's voxels; drops that do not (never from cvx_world_settle) set overLimit.
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult SettleColumn(const CopyWorld &W, int64_t cx, int64_t cz, int64_t y0, int64_t y1, const uint32_t *drop, uint32_t nodes, uint32_t *outRuns,
                                       uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	const ArenaColumn col = CopyColumnAt(W, cx, cz);
	const uint32_t solidRuns = col.Count();
	uint32_t first = 0, end = 0;
	if (nodes) { PiecesRunRange(col, y0, y1, &first, &end); }
	bool curSolid = false, crossed = false;
	int64_t curLength = 0, curIndex = 0;
	int64_t lowest = -1, highest = -1;
	int64_t y = (int64_t)W.dimY - 1; // the next voxel to emit
	// one span of `length` voxels from y down, all air or all solid with the colours of the run's voxels from srcTop - 1 down
	auto span = [&](bool solid, int64_t length, const SolidRun &run, int64_t srcTop) {
		if (length <= 0) { return; }
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
				for (int64_t k = 0; k < length; k++) {
					outColours[res.colours + (uint32_t)k] = W.colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - (uint32_t)(srcTop - k))) << (W.colorShift - 2))];
				}
			}
			res.colours += (uint32_t)length;
			if (highest < 0) { highest = y + 1; }
			lowest = y + 1 - length;
		}
		y -= length;
	};
	// the voxels [lo, hi) of `run`, `by` voxels further down
	auto part = [&](int64_t hi, int64_t lo, int64_t by, const SolidRun &run) {
		if (hi <= lo) { return; }
		if (hi - by > y + 1 || lo - by < 0) { // (it would pass what lies below it, or the floor)
			crossed = true;
			return;
		}
		span(false, y + 1 - (hi - by), run, 0);
		span(true, hi - lo, run, hi);
	};
	for (uint32_t k = 0; k < solidRuns; k++) {
		const SolidRun run = col.Run(k);
		const int64_t by = k >= first && k < end ? (int64_t)drop[k - first] : 0;
		if (by == 0) {
			part(run.top, run.bottom, 0, run);
			continue;
		}
		const int64_t hi = (int64_t)run.top > y1 ? y1 : (int64_t)run.top, lo = (int64_t)run.bottom < y0 ? y0 : (int64_t)run.bottom;
		part(run.top, hi, 0, run);
		part(hi, lo, by, run);
		part(lo, run.bottom, 0, run);
	}
	span(false, y + 1, SolidRun{ 0u, 0u, 0u }, 0);
	if (curLength > 0) {
		if (outRuns) { outRuns[res.runCount] = (curSolid ? (uint32_t)curIndex : 0xFFFFu) | ((uint32_t)curLength << 16); }
		if (curLength > 32767) { res.overLimit = true; }
		res.runCount++;
	}
	if (res.colours == 0u) { // the empty column: RunCount 0, no elements
		res.runCount = 0u;
		res.overLimit = crossed;
		return res;
	}
	if (res.runCount > 65535u || crossed) { res.overLimit = true; }
	res.worldMin = (uint32_t)lowest & 0xFFFFu;
	res.worldMax = (uint32_t)highest & 0xFFFFu;
	return res;
}

} // namespace cvxb
