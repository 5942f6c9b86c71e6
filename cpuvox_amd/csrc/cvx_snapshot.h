// cvx_snapshot.h -- comparing the device-resident world with a snapshot of it (cvx_world_snapshot_diff, cvx_snapshot.hip).
//
// The per-column rule, written once for the device AND the host (tests/test_world_snapshot_cpu.py compiles it with g++ through
// tests/snapshot_rules.cpp and compares it with the dense model of tests/snapshotmodel.py):
//   DiffColumn   walks two run lists top-down in step.  One is the arena's LOD-0 column through cvxb::ArenaColumn, in whatever encoding its
//                record has (1 .. 3 runs in the record, a run-list block, a tail-moved block; a foreign column's touching solid runs and shared
//                colours); the other is the snapshot's column in the blob layout, [guard][runs][guard][colours], runs colorsIndex | length << 16
//                with the top air run first (what cvxr::ReadColumn writes).  A span ends at the next run boundary of either side.  A span
//                that is solid on one side and air on the other differs whole; a span solid on both compares the colour words voxel by
//                voxel, unless colours are ignored.  The encodings never show: only voxels and colour words are compared.
#pragma once

#include <stdint.h>

#include "cvx_brush.h"

namespace cvxs {

struct ColumnDiff {
	uint32_t voxels;     // differing voxels of the column
	uint32_t yMin, yMax; // they lie in [yMin, yMax), both ends tight; 0, 0 when nothing differs
};

// col, colourSlots, colorShift: the arena's LOD-0 column (cvx_brush.h).  header: the snapshot column's three words (storageOffset, runCount |
// worldMin << 16, worldMax); elements: the snapshot blob's pool.  dimY: the world's height.
CVX_HD inline ColumnDiff DiffColumn(const cvxb::ArenaColumn &col, const uint32_t *colourSlots, int colorShift, int dimY, const uint32_t *header,
                                    const uint32_t *elements, bool ignoreColour)
{
	ColumnDiff d{ 0u, 0u, 0u };
	const uint32_t solidRuns = col.Count();
	const uint32_t runCount = header[1] & 0xFFFFu;
	const uint32_t *runs = elements + header[0] + 1u;             // behind the first guard
	const uint32_t *colours = elements + header[0] + runCount + 2u; // behind the second one
	uint32_t k = 0;          // the arena's run at or below y
	cvxb::SolidRun run{ 0u, 0u, 0u };
	bool haveRun = false;
	uint32_t r = 0;          // the snapshot's run that holds y - 1
	uint32_t sTop = (uint32_t)dimY, sBottom = (uint32_t)dimY, sIndex = 0;
	bool sSolid = false;
	uint32_t y = (uint32_t)dimY; // top of what is not compared yet (exclusive)
	while (y > 0u) {
		// the arena's side of [.., y)
		while (!haveRun && k < solidRuns) {
			run = col.Run(k);
			if (run.top > run.bottom && run.bottom < y) { haveRun = true; } else { k++; }
		}
		const bool aSolid = haveRun && run.top >= y;
		const uint32_t aNext = haveRun ? (aSolid ? run.bottom : run.top) : 0u;
		// the snapshot's side
		while (sBottom >= y && r < runCount) {
			const uint32_t raw = runs[r++];
			sTop = sBottom;
			sBottom = sTop - (raw >> 16);
			sSolid = (int16_t)(raw & 0xFFFFu) >= 0;
			sIndex = raw & 0xFFFFu;
		}
		const bool inRun = sBottom < y; // (else: the empty column, or below the last run -- air to the ground)
		const bool bSolid = inRun && sSolid;
		const uint32_t bNext = inRun ? sBottom : 0u;
		const uint32_t next = aNext > bNext ? aNext : bNext;
		if (aSolid != bSolid) {
			if (d.voxels == 0u) { d.yMax = y; }
			d.voxels += y - next;
			d.yMin = next;
		} else if (aSolid && !ignoreColour) {
			for (uint32_t v = y; v-- > next;) {
				const uint32_t a = colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - v)) << (colorShift - 2))];
				const uint32_t b = colours[sIndex + (sTop - 1u - v)];
				if (a != b) {
					if (d.voxels == 0u) { d.yMax = v + 1u; }
					d.voxels++;
					d.yMin = v;
				}
			}
		}
		y = next;
		if (haveRun && run.bottom >= y) {
			haveRun = false;
			k++;
		}
	}
	return d;
}

} // namespace cvxs
