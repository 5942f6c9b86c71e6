// cvx_readback.h -- reading the device-resident world back (cvx_world_read_region / cvx_world_read_level) and compacting its arena
// (cvx_world_compact, cvx_readback.hip).
//
// The per-column rule, written once for the device AND the host (tests/test_world_readback_cpu.py compiles it with g++ through
// tests/readback_rules.cpp):
//   LevelRun     solid run k of a record of ANY level in that level's own voxels: cvxb::ArenaColumn reads the spans in LOD-0 voxels
//                (cvx_device.h: topY = dimY - (voxels above << lod)) and, for records with 1 .. 3 runs, derives the colour index from them in
//                LOD-0 voxels too; both are shifted back here (exact: every span of a level is a multiple of 2^lod).
//   ReadColumn   the column in the builder's encoding (WordBuilder.cs:181-268, what cvxb::BrushColumn emits): maximal runs from the top,
//                the top air run first, air runs with ColorsIndex -1, ColorsIndex of a solid run = solid voxels above it, and worldMin /
//                worldMax as the RLEColumn constructor computes them (World.cs:190-234), in LOD-0 voxels.  Adjacent solid runs of the
//                record merge and every voxel keeps the colour its run addresses, so a column uploaded in another encoding comes back with the
//                same voxels and colours in builder form; a column with no solid voxel comes back empty (RunCount 0).
#pragma once

#include <stdint.h>

#include "cvx_brush.h"

namespace cvxr {

// Solid run k (0 = the top one) of a column with col.Count() > k, in voxels of level `lod`: [bottom, top), colour of voxel y = colorsIndex + (top - 1 - y)
CVX_HD inline cvxb::SolidRun LevelRun(const cvxb::ArenaColumn &col, uint32_t k, int lod)
{
	const cvxb::SolidRun r = col.Run(k);
	const bool listed = (col.x >> 30) == 0u; // (a run-list block keeps the blob's colour index, in the level's voxels)
	return cvxb::SolidRun{ r.bottom >> lod, r.top >> lod, listed ? r.colorsIndex : (r.colorsIndex >> lod) };
}

struct ReadResult {
	uint32_t runCount;         // elements between the guards (0: the empty column)
	uint32_t colours;          // solid voxels
	uint32_t worldMin, worldMax;
};

// Elements a column takes in a blob: [guard][runs][guard][colours], nothing for the empty column
CVX_HD inline uint32_t ReadElements(const ReadResult &r) { return r.runCount ? r.runCount + 2u + r.colours : 0u; }

// Out (may be null): runs[r] = colorsIndex | length << 16 (colorsIndex 0xFFFF for air); colours[k] = the k-th solid voxel's colour from the top
// (colourSlots: the level's colour array, 4-byte slots, read at the column's colorsBase + index << (colorShift - 2)).  dimY: the world's height
// (LOD-0 voxels).
CVX_HD inline ReadResult ReadColumn(const cvxb::ArenaColumn &col, const uint32_t *colourSlots, int colorShift, int lod, int dimY, uint32_t *outRuns,
                                    uint32_t *outColours)
{
	ReadResult res{ 0u, 0u, 0u, 0u };
	const uint32_t solidRuns = col.Count();
	uint32_t y = (uint32_t)dimY >> lod;     // top of what is not emitted yet (the level's voxels, exclusive)
	uint32_t curLength = 0, curIndex = 0;   // the solid run being merged
	uint32_t lowest = 0, highest = 0;
	for (uint32_t k = 0; k < solidRuns; k++) {
		const cvxb::SolidRun run = LevelRun(col, k, lod);
		if (run.top <= run.bottom) { continue; }
		if (run.top < y) { // air above this run: the open solid run ends, an air run follows
			if (curLength) {
				if (outRuns) { outRuns[res.runCount] = curIndex | (curLength << 16); }
				res.runCount++;
				curLength = 0;
			}
			if (outRuns) { outRuns[res.runCount] = 0xFFFFu | ((y - run.top) << 16); }
			res.runCount++;
		}
		if (curLength == 0u) { curIndex = res.colours; }
		if (res.colours == 0u) { highest = run.top; }
		const uint32_t length = run.top - run.bottom;
		if (outColours) {
			for (uint32_t j = 0; j < length; j++) {
				outColours[res.colours + j] = colourSlots[col.ColorsBase() + ((run.colorsIndex + j) << (colorShift - 2))];
			}
		}
		res.colours += length;
		curLength += length;
		lowest = run.bottom;
		y = run.bottom;
	}
	if (res.colours == 0u) { // the empty column (also a record that holds no solid voxel)
		res.runCount = 0u;
		return res;
	}
	if (outRuns) { outRuns[res.runCount] = curIndex | (curLength << 16); }
	res.runCount++;
	if (y > 0u) {
		if (outRuns) { outRuns[res.runCount] = 0xFFFFu | (y << 16); }
		res.runCount++;
	}
	res.worldMin = (lowest << lod) & 0xFFFFu;
	res.worldMax = (highest << lod) & 0xFFFFu;
	return res;
}

// The three header words of a read-back column (World.RLEColumn, World.cs:161-169): storageOffset, runCount | worldMin << 16, worldMax (pad 0)
CVX_HD inline void ReadHeader(const ReadResult &r, uint32_t storageOffset, uint32_t *h)
{
	if (r.runCount == 0u) {
		h[0] = h[1] = h[2] = 0u;
		return;
	}
	h[0] = storageOffset;
	h[1] = r.runCount | (r.worldMin << 16);
	h[2] = r.worldMax;
}

} // namespace cvxr
