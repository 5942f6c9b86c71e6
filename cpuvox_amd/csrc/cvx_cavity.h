// cvx_cavity.h -- the rules of cvx_world_cavities (cvx_cavity.hip): the enclosed cavities of the device-resident world.
//
// Written once for the device AND the host (tests/test_world_cavities_cpu.py compiles it with g++ through tests/cavity_rules.cpp, drives it with
// a sequential union-find and compares it with the dense model of tests/cavitymodel.py).  The counterpart of cvx_pieces.h on the AIR side:
//   CavityNextNode    the nodes of a column: its maximal air intervals [lo, hi) inside the box's y range, top-down -- the complement of the union
//                     of its solid runs (a foreign column's split solid span leaves no zero-length node between its halves; an empty column is
//                     one node; a column solid throughout the range has none)
//   CavityNodeCount / CavityNodes   their number and their [lo, hi) intervals
//   CavityNodeOpen    the faces of the clipped box a node lets air escape through (all six bits, whatever the call asks for)
//   CavityFillColumn  a column with its selected nodes solid, emitted as BrushColumn and PiecesRemoveColumn emit (the builder's encoding)
// The box (PiecesBox, PiecesClipBox) and the edge rule between nodes of face-neighbouring columns (PiecesTouch) are cvx_pieces.h's; nodes of one
// column are never connected.  The nodes of the box are numbered in column order, top-down inside a column: the smallest node index of a region
// is its seed.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_pieces.h"

namespace cvxb {

// The walk over a column's air intervals inside [y0, y1): `cursor` is one past the highest voxel not yet accounted for, `k` the next solid run.
struct CavityWalk {
	uint32_t k, count;
	int64_t cursor;
};

CVX_HD inline CavityWalk CavityWalkFrom(const ArenaColumn &col, int64_t y1)
{
	return CavityWalk{ RunAtOrBelow(col, y1 - 1), col.Count(), y1 }; // (the runs before k lie wholly at or above y1)
}

// The next node from the top: true and [*lo, *hi), or false when the range holds no more air.
CVX_HD inline bool CavityNextNode(const ArenaColumn &col, int64_t y0, CavityWalk *w, uint32_t *lo, uint32_t *hi)
{
	while (w->cursor > y0) {
		if (w->k >= w->count) { // the air below the lowest run
			*lo = (uint32_t)y0;
			*hi = (uint32_t)w->cursor;
			w->cursor = y0;
			return true;
		}
		const SolidRun run = col.Run(w->k++);
		const int64_t top = (int64_t)run.top, above = w->cursor;
		if ((int64_t)run.bottom < w->cursor) { w->cursor = (int64_t)run.bottom; }
		if (top < above) {
			*lo = (uint32_t)(top > y0 ? top : y0);
			*hi = (uint32_t)above;
			return true;
		}
	}
	return false;
}

CVX_HD inline uint32_t CavityNodeCount(const ArenaColumn &col, int64_t y0, int64_t y1)
{
	CavityWalk w = CavityWalkFrom(col, y1);
	uint32_t n = 0, lo, hi;
	while (CavityNextNode(col, y0, &w, &lo, &hi)) { n++; }
	return n;
}

// out[2 j], out[2 j + 1] = lo, hi of node j; returns the node count
CVX_HD inline uint32_t CavityNodes(const ArenaColumn &col, int64_t y0, int64_t y1, uint32_t *out)
{
	CavityWalk w = CavityWalkFrom(col, y1);
	uint32_t n = 0;
	while (CavityNextNode(col, y0, &w, out + 2u * n, out + 2u * n + 1u)) { n++; }
	return n;
}

// whether column `col` holds an air voxel in [lo, hi)
CVX_HD inline bool CavityAirIn(const ArenaColumn &col, int64_t lo, int64_t hi)
{
	CavityWalk w = CavityWalkFrom(col, hi);
	uint32_t a, b;
	return CavityNextNode(col, lo, &w, &a, &b);
}

// The open bits of node [lo, hi) of column (x, z): bit f (0..5 = -X, +X, -Y, +Y, -Z, +Z) is set when the node holds a voxel on face f of the
// clipped box and the voxel across that face is air.  Outside the world is air, below y = 0 and above dimY too; inside it the arena decides.
CVX_HD inline int CavityNodeOpen(const CopyWorld &W, const PiecesBox &B, int64_t x, int64_t z, uint32_t lo, uint32_t hi)
{
	int bits = 0;
	if (x == B.x0 && (x == 0 || CavityAirIn(CopyColumnAt(W, x - 1, z), lo, hi))) { bits |= 1; }
	if (x == B.x1 - 1 && (x + 1 >= W.dimX || CavityAirIn(CopyColumnAt(W, x + 1, z), lo, hi))) { bits |= 2; }
	if ((int64_t)lo == B.y0 && (B.y0 == 0 || CavityAirIn(CopyColumnAt(W, x, z), (int64_t)B.y0 - 1, B.y0))) { bits |= 4; }
	if ((int64_t)hi == B.y1 && (B.y1 >= W.dimY || CavityAirIn(CopyColumnAt(W, x, z), B.y1, (int64_t)B.y1 + 1))) { bits |= 8; }
	if (z == B.z0 && (z == 0 || CavityAirIn(CopyColumnAt(W, x, z - 1), lo, hi))) { bits |= 16; }
	if (z == B.z1 - 1 && (z + 1 >= W.dimZ || CavityAirIn(CopyColumnAt(W, x, z + 1), lo, hi))) { bits |= 32; }
	return bits;
}

// Column (cx, cz) with the nodes whose flag is set made solid with `argb` (selected[j] != 0 for node j of the column inside [y0, y1); null: a
// column outside the box, which has none), emitted as BrushColumn emits it: maximal runs from the top, the old colours verbatim.  The walk
// goes top-down over the column's runs; the air above a run is cut at the box's y range, and the part inside it is node j, j counting from the
// top exactly as CavityNextNode counts.
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult CavityFillColumn(const CopyWorld &W, int64_t cx, int64_t cz, int64_t y0, int64_t y1, const uint32_t *selected, uint32_t argb,
                                           uint32_t *outRuns, uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	const ArenaColumn col = CopyColumnAt(W, cx, cz);
	const uint32_t solidRuns = col.Count();
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0;
	int64_t lowest = -1, highest = -1;
	int64_t y = (int64_t)W.dimY - 1; // the next voxel to emit
	uint32_t node = 0;               // the next node of the column
	// one span of `length` voxels from y down: air, the run's own voxels, or filled ones
	auto span = [&](bool solid, bool filled, int64_t length, const SolidRun &run) {
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
				for (int64_t v = y; v > y - length; v--) {
					outColours[res.colours + (uint32_t)(y - v)] =
						filled ? argb : W.colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - (uint32_t)v)) << (W.colorShift - 2))];
				}
			}
			res.colours += (uint32_t)length;
			if (highest < 0) { highest = y + 1; }
			lowest = y + 1 - length;
		}
		y -= length;
	};
	// the air from y down to `floor` (exclusive below): the part inside [y0, y1) is a node
	auto gap = [&](int64_t floor, const SolidRun &run) {
		const int64_t hi = y + 1 < y1 ? y + 1 : y1, lo = floor > y0 ? floor : y0;
		if (!selected || lo >= hi) {
			span(false, false, y + 1 - floor, run);
			return;
		}
		const bool fill = selected[node++] != 0u;
		span(false, false, y + 1 - hi, run);
		span(fill, fill, hi - lo, run);
		span(false, false, lo - floor, run);
	};
	for (uint32_t k = 0; k < solidRuns; k++) {
		const SolidRun run = col.Run(k);
		gap((int64_t)run.top, run);
		span(true, false, (int64_t)run.top - run.bottom, run);
	}
	gap(0, SolidRun{ 0u, 0u, 0u });
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
