// cvx_nav.h -- the rules of cvx_world_nav_build / cvx_nav_query (cvx_nav.hip): walking-distance fields over the device-resident world.
//
// Written once for the device AND the host (tests/test_world_nav_cpu.py compiles it with g++ through tests/nav_rules.cpp, drives it with a
// sequential Bellman-Ford and compares it with the dense model of tests/navmodel.py, which knows no intervals).  A body is a box of w x h x w
// voxels, a cell the voxel of its min corner, and cell column (x, z) stands for the w x w arena columns (x .. x + w - 1, z .. z + w - 1):
//   NavNextInterval   the maximal air intervals [lo, hi) of the UNION of the solid runs of a cell column's arena columns, top-down; the topmost
//                     one is open upwards (hi = kNavSky: everything at y >= dimY is air), below y = 0 is the floor
//   NavNextNode       the intervals that are nodes: hi - lo >= h and y0 <= lo < y1; the stand cell of a node is (x, lo, z)
//   NavStep           the step predicate between nodes of face-neighbouring cell columns (directed: a cliff is descended, not climbed)
//   NavForEachStep    the targets of the steps from one node into a neighbour column's node list, top-down
//   NavResolve        the node a goal or a query position falls to in its column's node list
//   NavChooseNext     the `next` of a reached node from the final distances: first direction in -X, +X, -Z, +Z, there the highest target
// The cell grid (NavGrid) is the clipped box shrunk by w - 1 in X and Z; its columns are numbered in (x, then z) order and the nodes in column
// order, top-down inside a column, as pieces and cavities number theirs.  Node lists are read through any type with Lo(i) and Hi(i).
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_pieces.h"

namespace cvxb {

constexpr uint32_t kNavSky = 0xFFFFFFFFu;       // hi of the topmost interval: above every int32 position
constexpr uint32_t kNavUnreached = 0xFFFFFFFFu; // a node's distance before anything reaches it
constexpr uint32_t kNavNoNext = 0xFFFFFFFFu;    // a node's packed `next`: unreached
constexpr uint32_t kNavAtGoal = 0xFFFFFFFEu;    // ... a goal: the cell itself
constexpr int kNavMaxWidth = 8, kNavMaxHeight = 64, kNavMaxDrop = 4096;

struct NavRule {
	int w, h, s, m; // width, height, stepUp, maxDrop
};

// The cells of a field: x0 <= x < x0 + sizeX, z0 <= z < z0 + sizeZ (sizes 0: the box is narrower than the body), floors in [y0, y1).
struct NavGrid {
	int x0, z0, sizeX, sizeZ, y0, y1;

	CVX_HD int64_t Columns() const { return (int64_t)sizeX * sizeZ; }
	CVX_HD bool Holds(int64_t x, int64_t z) const { return x >= x0 && x < (int64_t)x0 + sizeX && z >= z0 && z < (int64_t)z0 + sizeZ; }
	CVX_HD int64_t Column(int64_t x, int64_t z) const { return (x - x0) * sizeZ + (z - z0); }
};

CVX_HD inline NavGrid NavGridOf(const PiecesBox &B, int w)
{
	const int sx = B.SizeX() - w + 1, sz = B.SizeZ() - w + 1;
	const bool none = sx <= 0 || sz <= 0;
	return NavGrid{ B.x0, B.z0, none ? 0 : sx, none ? 0 : sz, B.y0, B.y1 };
}

CVX_HD inline bool NavRuleValid(const NavRule &R)
{
	return R.w >= 1 && R.w <= kNavMaxWidth && R.h >= 1 && R.h <= kNavMaxHeight && R.s >= 0 && R.s <= R.h && R.m >= 0 && R.m <= kNavMaxDrop;
}

// The walk over the air intervals of cell column (x, z): `cursor` is one past the highest voxel not yet accounted for.  The walk keeps no state
// per arena column: every move searches the w x w columns' runs again (a binary search each), so its registers do not grow with w.
struct NavWalk {
	int64_t cursor;
	bool sky; // the next interval is the topmost one
};

CVX_HD inline NavWalk NavWalkFrom(const CopyWorld &W) { return NavWalk{ (int64_t)W.dimY, true }; }

// The next interval from the top: true and [*lo, *hi), or false when the column holds no more air.
CVX_HD inline bool NavNextInterval(const CopyWorld &W, int64_t x, int64_t z, int w, NavWalk *walk, uint32_t *lo, uint32_t *hi)
{
	while (walk->cursor > 0 || walk->sky) {
		const int64_t above = walk->cursor;
		// the highest solid voxel below the cursor in any of the columns: its top
		int64_t top = 0;
		for (int i = 0; i < w && above > 0; i++) {
			for (int k = 0; k < w; k++) {
				const ArenaColumn col = CopyColumnAt(W, x + i, z + k);
				const uint32_t r = RunAtOrBelow(col, above - 1);
				if (r < col.Count()) {
					const int64_t t = (int64_t)col.Run(r).top;
					const int64_t clipped = t < above ? t : above;
					top = clipped > top ? clipped : top;
				}
			}
		}
		// the union's solid block [bottom, top): every pass takes in the runs that hold the voxel under it, until none does
		int64_t bottom = top;
		for (bool lowered = top > 0; lowered && bottom > 0;) {
			lowered = false;
			for (int i = 0; i < w; i++) {
				for (int k = 0; k < w; k++) {
					const ArenaColumn col = CopyColumnAt(W, x + i, z + k);
					const uint32_t r = RunAtOrBelow(col, bottom - 1);
					if (r >= col.Count()) { continue; }
					const SolidRun run = col.Run(r);
					if ((int64_t)run.top >= bottom && (int64_t)run.bottom < bottom) {
						bottom = (int64_t)run.bottom;
						lowered = true;
					}
				}
			}
		}
		const bool sky = walk->sky;
		walk->cursor = bottom;
		walk->sky = false;
		if (top < above || sky) {
			*lo = (uint32_t)top;
			*hi = sky ? kNavSky : (uint32_t)above;
			return true;
		}
	}
	return false;
}

CVX_HD inline bool NavIsNode(uint32_t lo, uint32_t hi, int h, int64_t y0, int64_t y1)
{
	return (int64_t)hi - (int64_t)lo >= h && (int64_t)lo >= y0 && (int64_t)lo < y1;
}

// The next node from the top.  Intervals whose floor lies below y0 end the walk: every later one lies lower still.
CVX_HD inline bool NavNextNode(const CopyWorld &W, const NavGrid &G, int64_t x, int64_t z, const NavRule &R, NavWalk *walk, uint32_t *lo, uint32_t *hi)
{
	while (NavNextInterval(W, x, z, R.w, walk, lo, hi)) {
		if ((int64_t)*lo < G.y0) { return false; }
		if (NavIsNode(*lo, *hi, R.h, G.y0, G.y1)) { return true; }
	}
	return false;
}

CVX_HD inline uint32_t NavNodeCount(const CopyWorld &W, const NavGrid &G, int64_t x, int64_t z, const NavRule &R)
{
	NavWalk walk = NavWalkFrom(W);
	uint32_t n = 0, lo, hi;
	while (NavNextNode(W, G, x, z, R, &walk, &lo, &hi)) { n++; }
	return n;
}

// A step from node [loA, hiA) to node [loB, hiB) of a face-neighbouring cell column: the floors differ by at most stepUp up and maxDrop down,
// and both intervals are clear up to the higher floor + h (the body rises in place or falls in the destination through clear air).
CVX_HD inline bool NavStep(uint32_t loA, uint32_t hiA, uint32_t loB, uint32_t hiB, const NavRule &R)
{
	const int64_t d = (int64_t)loB - (int64_t)loA;
	if (d > R.s || d < -(int64_t)R.m) { return false; }
	const int64_t need = (int64_t)(loA > loB ? loA : loB) + R.h;
	return (int64_t)(hiA < hiB ? hiA : hiB) >= need;
}

// The first node of [first, end) whose floor is at or below y (floors fall with the index): a binary search.
template <typename Nodes> CVX_HD inline uint32_t NavFirstAtOrBelow(const Nodes &N, uint32_t first, uint32_t end, int64_t y)
{
	uint32_t a = first, b = end;
	while (a < b) {
		const uint32_t mid = (a + b) >> 1;
		if ((int64_t)N.Lo(mid) > y) { a = mid + 1u; } else { b = mid; }
	}
	return a;
}

// f(b) for the target b of every step from node [loA, hiA) into the node list [first, end) of a neighbour column, top-down; f returns true to
// stop.  The candidates are the nodes with a floor in (loA, loA + s] and the ONE node below them: a lower target must hold the level loA + h - 1
// itself (its interval reaches up to the source's headroom), and the intervals of a column are disjoint.  The loop is bounded by `end`.
template <typename Nodes, typename F>
CVX_HD inline void NavForEachStep(const Nodes &N, uint32_t loA, uint32_t hiA, uint32_t first, uint32_t end, const NavRule &R, F f)
{
	for (uint32_t b = NavFirstAtOrBelow(N, first, end, (int64_t)loA + R.s); b < end; b++) {
		const uint32_t loB = N.Lo(b);
		if (NavStep(loA, hiA, loB, N.Hi(b), R) && f(b)) { return; }
		if (loB <= loA) { return; }
	}
}

// The node of [first, end) position y falls to: the one whose interval holds y (the floor the body would fall to through clear air); `end`: none
// (y in solid, below the floor, or in an interval that is no node).
template <typename Nodes> CVX_HD inline uint32_t NavResolve(const Nodes &N, uint32_t first, uint32_t end, int64_t y)
{
	if (y < 0) { return end; }
	const uint32_t i = NavFirstAtOrBelow(N, first, end, y);
	return i < end && y < (int64_t)N.Hi(i) ? i : end;
}

// the pick's face numbers of the four step directions, in the order of the choice; and the neighbour column of each
CVX_HD inline int NavDirection(int k) { return k < 2 ? k : k + 2; } // 0, 1, 4, 5 = -X, +X, -Z, +Z
CVX_HD inline int NavDirX(int k) { return k == 0 ? -1 : (k == 1 ? 1 : 0); }
CVX_HD inline int NavDirZ(int k) { return k == 2 ? -1 : (k == 3 ? 1 : 0); }

CVX_HD inline uint32_t NavPackNext(int k, uint32_t y) { return ((uint32_t)NavDirection(k) << 24) | y; }

// The packed `next` of a reached node at distance d > 0 of cell column (x, z): `range(c, &first, &end)` gives a column's node list, `dist(b)` a
// node's final distance.  kNavNoNext when no step leads to distance d - 1 (never, for a distance the relaxation made).
template <typename Nodes, typename Range, typename Dist>
CVX_HD inline uint32_t NavChooseNext(const Nodes &N, const NavGrid &G, int64_t x, int64_t z, uint32_t lo, uint32_t hi, uint32_t d, const NavRule &R, Range range,
                                     Dist dist)
{
	for (int k = 0; k < 4; k++) {
		const int64_t nx = x + NavDirX(k), nz = z + NavDirZ(k);
		if (!G.Holds(nx, nz)) { continue; }
		uint32_t first, end, found = kNavNoNext;
		range(G.Column(nx, nz), &first, &end);
		NavForEachStep(N, lo, hi, first, end, R, [&](uint32_t b) {
			if (dist(b) != d - 1u) { return false; }
			found = NavPackNext(k, N.Lo(b));
			return true;
		});
		if (found != kNavNoNext) { return found; }
	}
	return kNavNoNext;
}

// What a query gives for the node at (x, lo, z) with distance d and packed next, or (found = false) for a position that resolves to nothing.
CVX_HD inline cvx_nav_step NavStepRecord(bool found, int64_t x, uint32_t lo, int64_t z, uint32_t d, uint32_t next)
{
	cvx_nav_step s;
	s.cell[0] = s.cell[1] = s.cell[2] = -1;
	s.distance = -1;
	s.next[0] = s.next[1] = s.next[2] = -1;
	s.direction = -1;
	if (!found) { return s; }
	s.cell[0] = (int32_t)x;
	s.cell[1] = (int32_t)lo;
	s.cell[2] = (int32_t)z;
	if (d == kNavUnreached) { return s; }
	s.distance = (int32_t)d;
	if (next == kNavAtGoal || next == kNavNoNext) {
		s.next[0] = s.cell[0];
		s.next[1] = s.cell[1];
		s.next[2] = s.cell[2];
		return s;
	}
	const int direction = (int)(next >> 24);
	s.direction = direction;
	s.next[0] = (int32_t)x + (direction == 0 ? -1 : (direction == 1 ? 1 : 0));
	s.next[1] = (int32_t)(next & 0xFFFFFFu);
	s.next[2] = (int32_t)z + (direction == 4 ? -1 : (direction == 5 ? 1 : 0));
	return s;
}

} // namespace cvxb
