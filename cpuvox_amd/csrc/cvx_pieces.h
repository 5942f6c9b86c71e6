// cvx_pieces.h -- the rules of cvx_world_pieces (cvx_pieces.hip): the floating pieces of the device-resident world.
//
// Written once for the device AND the host (tests/test_world_pieces_cpu.py compiles it with g++ through tests/pieces_rules.cpp, drives it with
// a sequential union-find and compares it with the dense model of tests/piecesmodel.py):
//   PiecesBox           the call's box clipped to the world, and its columns in (x, then z) order
//   PiecesRunCount      the nodes of a column: its solid runs clipped to the box's y range, top-down (a foreign column's split run gives two)
//   PiecesClippedRuns   their [lo, hi) intervals
//   PiecesTouch         the edge rule between nodes of face-neighbouring columns; PiecesStacked: between consecutive nodes of one column
//   PiecesNodeAnchors   CVX_ANCHOR_GROUND / CVX_ANCHOR_OUTSIDE of one node
//   PiecesRemoveColumn  a column without its floating nodes, emitted as BrushColumn emits it (the builder's encoding)
// The nodes of the box are numbered in column order, top-down inside a column: the smallest node index of a piece is its seed.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_box.h" // BoxCheck: what a box must keep before it is clipped
#include "cvx_copy.h"

namespace cvxb {

struct PiecesBox {
	int x0, y0, z0, x1, y1, z1; // [min, max) inside the world

	CVX_HD int SizeX() const { return x1 - x0; }
	CVX_HD int SizeZ() const { return z1 - z0; }
	CVX_HD int64_t Columns() const { return (int64_t)SizeX() * SizeZ(); }
	CVX_HD bool Holds(int64_t x, int64_t z) const { return x >= x0 && x < x1 && z >= z0 && z < z1; }
	CVX_HD int64_t Column(int64_t x, int64_t z) const { return (x - x0) * SizeZ() + (z - z0); }
};

// boxMin / boxMax clipped to the world; false: nothing of the box is inside it
CVX_HD inline bool PiecesClipBox(const int32_t boxMin[3], const int32_t boxMax[3], int dimX, int dimY, int dimZ, PiecesBox *out)
{
	const int dim[3] = { dimX, dimY, dimZ };
	int lo[3], hi[3];
	for (int a = 0; a < 3; a++) {
		lo[a] = boxMin[a] < 0 ? 0 : boxMin[a];
		hi[a] = boxMax[a] > dim[a] ? dim[a] : boxMax[a];
		if (lo[a] >= hi[a]) { return false; }
	}
	*out = PiecesBox{ lo[0], lo[1], lo[2], hi[0], hi[1], hi[2] };
	return true;
}

// The first and one past the last run of the column that hold a voxel of [y0, y1): the nodes are runs first .. end - 1.
CVX_HD inline void PiecesRunRange(const ArenaColumn &col, int64_t y0, int64_t y1, uint32_t *first, uint32_t *end)
{
	const uint32_t count = col.Count();
	uint32_t k = RunAtOrBelow(col, y1 - 1); // runs before k lie wholly at or above y1
	*first = k;
	while (k < count && (int64_t)col.Run(k).top > y0) { k++; }
	*end = k;
}

CVX_HD inline uint32_t PiecesRunCount(const ArenaColumn &col, int64_t y0, int64_t y1)
{
	uint32_t first, end;
	PiecesRunRange(col, y0, y1, &first, &end);
	return end - first;
}

// out[2 j], out[2 j + 1] = lo, hi of node j: the run's voxels lo .. hi - 1 inside [y0, y1); returns the node count
CVX_HD inline uint32_t PiecesClippedRuns(const ArenaColumn &col, int64_t y0, int64_t y1, uint32_t *out)
{
	uint32_t first, end;
	PiecesRunRange(col, y0, y1, &first, &end);
	for (uint32_t k = first; k < end; k++) {
		const SolidRun run = col.Run(k);
		out[2u * (k - first)] = (int64_t)run.bottom < y0 ? (uint32_t)y0 : run.bottom;
		out[2u * (k - first) + 1u] = (int64_t)run.top > y1 ? (uint32_t)y1 : run.top;
	}
	return end - first;
}

// Nodes of two columns that share a face in X or Z are connected when their intervals share a y.
CVX_HD inline bool PiecesTouch(uint32_t lo, uint32_t hi, uint32_t lo2, uint32_t hi2) { return (lo > lo2 ? lo : lo2) < (hi < hi2 ? hi : hi2); }
// Node j and node j + 1 of one column (the one below) are connected when the column's encoding split one solid span into the two.
CVX_HD inline bool PiecesStacked(uint32_t lo, uint32_t hiBelow) { return lo == hiBelow; }

// whether column `col` holds a solid voxel in [lo, hi)
CVX_HD inline bool PiecesSolidIn(const ArenaColumn &col, int64_t lo, int64_t hi)
{
	const uint32_t k = RunAtOrBelow(col, hi - 1);
	return k < col.Count() && (int64_t)col.Run(k).top > lo;
}

// The anchor bits of node [lo, hi) of column (x, z), whatever the call asks for: GROUND, a voxel with y = 0; OUTSIDE, a voxel with a solid face
// neighbour inside the world and outside the box (above or below the box's y range in its own column, or in a column beside the box).
CVX_HD inline int PiecesNodeAnchors(const CopyWorld &W, const PiecesBox &B, int64_t x, int64_t z, uint32_t lo, uint32_t hi)
{
	int bits = lo == 0u ? CVX_ANCHOR_GROUND : 0;
	bool outside = false;
	if ((int64_t)hi == B.y1 && B.y1 < W.dimY) { outside = outside || PiecesSolidIn(CopyColumnAt(W, x, z), B.y1, (int64_t)B.y1 + 1); }
	if ((int64_t)lo == B.y0 && B.y0 > 0) { outside = outside || PiecesSolidIn(CopyColumnAt(W, x, z), (int64_t)B.y0 - 1, B.y0); }
	if (x == B.x0 && x > 0) { outside = outside || PiecesSolidIn(CopyColumnAt(W, x - 1, z), lo, hi); }
	if (x == B.x1 - 1 && x + 1 < W.dimX) { outside = outside || PiecesSolidIn(CopyColumnAt(W, x + 1, z), lo, hi); }
	if (z == B.z0 && z > 0) { outside = outside || PiecesSolidIn(CopyColumnAt(W, x, z - 1), lo, hi); }
	if (z == B.z1 - 1 && z + 1 < W.dimZ) { outside = outside || PiecesSolidIn(CopyColumnAt(W, x, z + 1), lo, hi); }
	return bits | (outside ? CVX_ANCHOR_OUTSIDE : 0);
}

// Column (cx, cz) without the nodes whose flag is set (floating[j] != 0 for node j; the column has `nodes` of them inside [y0, y1); a column
// outside the box has none), emitted as BrushColumn emits it: maximal runs from the top, colours verbatim.  The walk goes top-down over the
// column's runs; a run that is a node is cut at the box's y range, and the part inside it is solid unless the node floats.
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult PiecesRemoveColumn(const CopyWorld &W, int64_t cx, int64_t cz, int64_t y0, int64_t y1, const uint32_t *floating, uint32_t nodes,
                                             uint32_t *outRuns, uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	const ArenaColumn col = CopyColumnAt(W, cx, cz);
	const uint32_t solidRuns = col.Count();
	uint32_t first = 0, end = 0;
	if (nodes) { PiecesRunRange(col, y0, y1, &first, &end); }
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0;
	int64_t lowest = -1, highest = -1;
	int64_t y = (int64_t)W.dimY - 1; // the next voxel to emit
	// one span of `length` voxels from y down, all solid (colours: the run's) or all air
	auto span = [&](bool solid, int64_t length, const SolidRun &run) {
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
					outColours[res.colours + (uint32_t)(y - v)] = W.colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - (uint32_t)v)) << (W.colorShift - 2))];
				}
			}
			res.colours += (uint32_t)length;
			if (highest < 0) { highest = y + 1; }
			lowest = y + 1 - length;
		}
		y -= length;
	};
	for (uint32_t k = 0; k < solidRuns; k++) {
		const SolidRun run = col.Run(k);
		span(false, y + 1 - (int64_t)run.top, run);
		const bool gone = k >= first && k < end && floating[k - first] != 0u;
		if (!gone) {
			span(true, (int64_t)run.top - run.bottom, run);
			continue;
		}
		const int64_t hi = (int64_t)run.top > y1 ? y1 : (int64_t)run.top, lo = (int64_t)run.bottom < y0 ? y0 : (int64_t)run.bottom;
		span(true, (int64_t)run.top - hi, run);
		span(false, hi - lo, run);
		span(true, lo - (int64_t)run.bottom, run);
	}
	span(false, y + 1, SolidRun{ 0u, 0u, 0u });
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
