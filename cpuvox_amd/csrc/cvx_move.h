// cvx_move.h -- the rule of cvx_world_move (cvx_move.hip): moving boxes through the device-resident world, with collision, sliding and step-up.
//
// Written once for the device AND the host (tests/test_world_move_cpu.py compiles it with g++ through tests/move_rules.cpp and compares it with
// the dense numpy model of tests/movemodel.py).  Integers only; the contract is in include/cpuvox_gpu.h (cvx_world_move).
//   MoveOcc       occupancy of LOD 0 of the arena with the rules for voxels outside the tile, asked a column at a time from its solid runs
//   MoveSolo      the group of lanes that owns a body, on the host and for a thread per body: one lane, nothing to reduce
//   MoveBody      a body's whole move: slide, step-up, the flags
// A leg is a reduction over columns, not a walk: a Y leg takes the nearest solid voxel above / below the box over the footprint's columns, an X
// or Z leg the nearest slab whose cross-section holds a solid voxel over the columns of the swept rectangle.  The lanes of a group take those
// columns Size() at a time (column base + Lane()) and reduce with Min / Max; everything else is computed redundantly by every lane of the group
// from the reduced values, so the control flow is uniform inside a group and the result does not depend on its size.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_copy.h"

namespace cvxb {

constexpr int kMoveShift = 8; // log2 CVX_MOVE_UNIT: v >> kMoveShift is floor(v / 256) for negatives too
static_assert((1 << kMoveShift) == CVX_MOVE_UNIT, "CVX_MOVE_UNIT is 2^kMoveShift");
constexpr int32_t kMoveMaxSize = 64 * CVX_MOVE_UNIT, kMoveMaxDelta = 256 * CVX_MOVE_UNIT, kMoveMaxStepUp = 4 * CVX_MOVE_UNIT, kMoveMaxPos = 1 << 28;
constexpr int32_t kMoveNone = INT32_MAX;

// What the host-array call rejects and the kernel answers with CVX_MOVED_INVALID; these limits bound every loop below.
CVX_HD inline bool MoveBodyValid(const cvx_move_body &b)
{
	for (int a = 0; a < 3; a++) {
		if (b.size[a] < 1 || b.size[a] > kMoveMaxSize) { return false; }
		if (b.delta[a] < -kMoveMaxDelta || b.delta[a] > kMoveMaxDelta) { return false; }
		if (b.pos[a] < -kMoveMaxPos || b.pos[a] > kMoveMaxPos) { return false; }
	}
	return b.stepUp >= 0 && b.stepUp <= kMoveMaxStepUp && (b.flags & ~(CVX_MOVE_SOLID_BELOW | CVX_MOVE_SOLID_SIDES)) == 0;
}

// ---- occupancy, a column at a time ---------------------------------------------------------------------------------------------------------------

struct MoveOcc {
	CopyWorld W;
	bool repeat;
	bool solidBelow, solidSides;

	// the column of the tile voxel column (x, z) reads; false: outside the tile (bounded world)
	CVX_HD bool Column(int32_t x, int32_t z, ArenaColumn *col) const
	{
		if (repeat) {
			x %= W.dimX;
			z %= W.dimZ;
			x += x < 0 ? W.dimX : 0;
			z += z < 0 ? W.dimZ : 0;
		} else if (x < 0 || x >= W.dimX || z < 0 || z >= W.dimZ) {
			return false;
		}
		*col = CopyColumnAt(W, x, z);
		return true;
	}

	// any solid voxel in column (x, z) with y0 <= y <= y1
	CVX_HD bool Any(int32_t x, int32_t z, int32_t y0, int32_t y1) const
	{
		if (y0 < 0) {
			if (solidBelow) { return true; }
			y0 = 0;
		}
		y1 = y1 < W.dimY ? y1 : W.dimY - 1;
		if (y0 > y1) { return false; }
		ArenaColumn col;
		if (!Column(x, z, &col)) { return solidSides; }
		const uint32_t k = RunAtOrBelow(col, y1); // the highest run that reaches down to y1 or below
		return k < col.Count() && (int64_t)col.Run(k).top > y0;
	}

	// the lowest solid voxel of column (x, z) in y0 .. y1, kMoveNone: none
	CVX_HD int32_t LowestIn(int32_t x, int32_t z, int32_t y0, int32_t y1) const
	{
		if (y0 < 0) {
			if (solidBelow) { return y0; }
			y0 = 0;
		}
		y1 = y1 < W.dimY ? y1 : W.dimY - 1;
		if (y0 > y1) { return kMoveNone; }
		ArenaColumn col;
		if (!Column(x, z, &col)) { return solidSides ? y0 : kMoveNone; }
		const uint32_t k = RunAtOrBelow(col, y0);
		if (k < col.Count() && (int64_t)col.Run(k).top > y0) { return y0; }
		if (k == 0u) { return kMoveNone; }
		const int64_t bottom = col.Run(k - 1u).bottom; // the run just above y0
		return bottom <= y1 ? (int32_t)bottom : kMoveNone;
	}

	// the highest solid voxel of column (x, z) in y0 .. y1, -kMoveNone: none
	CVX_HD int32_t HighestIn(int32_t x, int32_t z, int32_t y0, int32_t y1) const
	{
		y1 = y1 < W.dimY ? y1 : W.dimY - 1;
		if (y0 > y1) { return -kMoveNone; }
		if (y1 < 0) { return solidBelow ? y1 : -kMoveNone; }
		const int32_t floor = y0 > 0 ? y0 : 0;
		ArenaColumn col;
		if (!Column(x, z, &col)) {
			if (solidSides) { return y1; }
		} else {
			const uint32_t k = RunAtOrBelow(col, y1);
			if (k < col.Count()) {
				const int64_t top = (int64_t)col.Run(k).top - 1;
				const int64_t y = top < y1 ? top : y1;
				if (y >= floor) { return (int32_t)y; }
			}
		}
		return y0 < 0 && solidBelow ? -1 : -kMoveNone;
	}
};

// ---- the lanes that own a body --------------------------------------------------------------------------------------------------------------------

struct MoveSolo {
	CVX_HD int Lane() const { return 0; }
	CVX_HD int Size() const { return 1; }
	CVX_HD int32_t Min(int32_t v) const { return v; }
	CVX_HD int32_t Max(int32_t v) const { return v; }
};

// ---- the reductions of a leg ------------------------------------------------------------------------------------------------------------------------

// The first of the `count` slabs k0, k0 + step, ... on axis `axis` (0: X, 2: Z) with a solid voxel in the cross-section c0 .. c1 (the other
// horizontal axis) x y0 .. y1, as its number 0 .. count - 1; kMoveNone: none.  Columns in slab-major order, a group's worth per trip: a trip with
// a hit ends the search, since every earlier slab lay in an earlier trip or in this one.
template <class Occ, class Group>
CVX_HD inline int32_t FirstBlockedSlab(const Occ &occ, const Group &g, int axis, int32_t k0, int32_t step, int32_t count, int32_t c0, int32_t c1, int32_t y0,
                                       int32_t y1)
{
	const int32_t across = c1 - c0 + 1, columns = count * across;
	for (int32_t base = 0; base < columns; base += g.Size()) {
		const int32_t i = base + g.Lane();
		int32_t hit = kMoveNone;
		if (i < columns) {
			const int32_t s = i / across, k = k0 + step * s, c = c0 + (i - s * across);
			if (axis == 0 ? occ.Any(k, c, y0, y1) : occ.Any(c, k, y0, y1)) { hit = s; }
		}
		hit = g.Min(hit);
		if (hit != kMoveNone) { return hit; }
	}
	return kMoveNone;
}

// The lowest (up) / highest solid voxel in y0 .. y1 over the columns x0 .. x1, z0 .. z1; kMoveNone / -kMoveNone: none
template <class Occ, class Group>
CVX_HD inline int32_t NearestInFootprint(const Occ &occ, const Group &g, bool up, int32_t x0, int32_t x1, int32_t z0, int32_t z1, int32_t y0, int32_t y1)
{
	const int32_t across = z1 - z0 + 1, columns = (x1 - x0 + 1) * across;
	int32_t best = up ? kMoveNone : -kMoveNone;
	for (int32_t base = 0; base < columns; base += g.Size()) {
		const int32_t i = base + g.Lane();
		if (i < columns) {
			const int32_t x = x0 + i / across, z = z0 + i % across;
			const int32_t y = up ? occ.LowestIn(x, z, y0, y1) : occ.HighestIn(x, z, y0, y1);
			best = up ? (y < best ? y : best) : (y > best ? y : best);
		}
	}
	return up ? g.Min(best) : g.Max(best);
}

// ---- legs, slide, step-up ------------------------------------------------------------------------------------------------------------------------------

struct MoveBox {
	int32_t pos[3], size[3];
	CVX_HD int32_t First(int a) const { return pos[a] >> kMoveShift; }
	CVX_HD int32_t Last(int a) const { return (pos[a] + size[a] - 1) >> kMoveShift; }
};

// One leg on `axis` by d != 0: moves the box, returns the direction's blocked bit or 0.
template <class Occ, class Group>
CVX_HD inline uint32_t MoveLeg(const Occ &occ, const Group &g, MoveBox &b, int axis, int32_t d)
{
	const bool plus = d > 0;
	const int32_t length = plus ? d : -d;
	// the slabs entered: `count` of them from k0 in the leg's direction
	const int32_t k0 = plus ? b.Last(axis) + 1 : b.First(axis) - 1;
	const int32_t kEnd = plus ? (b.pos[axis] + b.size[axis] + d - 1) >> kMoveShift : (b.pos[axis] + d) >> kMoveShift;
	const int32_t count = plus ? kEnd - k0 + 1 : k0 - kEnd + 1;
	int32_t moved = length;
	if (count > 0) {
		int32_t k = kMoveNone; // the slab that stops the box
		if (axis == 1) {
			const int32_t y = NearestInFootprint(occ, g, plus, b.First(0), b.Last(0), b.First(2), b.Last(2), plus ? k0 : kEnd, plus ? kEnd : k0);
			if (y != kMoveNone && y != -kMoveNone) { k = y; }
		} else {
			const int other = 2 - axis;
			const int32_t s = FirstBlockedSlab(occ, g, axis, k0, plus ? 1 : -1, count, b.First(other), b.Last(other), b.First(1), b.Last(1));
			if (s != kMoveNone) { k = plus ? k0 + s : k0 - s; }
		}
		if (k != kMoveNone) {
			const int64_t flush = plus ? (int64_t)CVX_MOVE_UNIT * k - ((int64_t)b.pos[axis] + b.size[axis]) : (int64_t)b.pos[axis] - (int64_t)CVX_MOVE_UNIT * ((int64_t)k + 1);
			moved = flush < length ? (int32_t)flush : length;
		}
	}
	b.pos[axis] += plus ? moved : -moved;
	return moved < length ? 1u << (2 * axis + (plus ? 1 : 0)) : 0u;
}

// a solid voxel in slab `k` of Y under the box's XZ footprint
template <class Occ, class Group>
CVX_HD inline bool MoveFootprintSolid(const Occ &occ, const Group &g, const MoveBox &b, int32_t y0, int32_t y1)
{
	return FirstBlockedSlab(occ, g, 0, b.First(0), 1, b.Last(0) - b.First(0) + 1, b.First(2), b.Last(2), y0, y1) != kMoveNone;
}

template <class Occ, class Group>
CVX_HD inline bool MoveResting(const Occ &occ, const Group &g, const MoveBox &b)
{
	if ((b.pos[1] & (CVX_MOVE_UNIT - 1)) != 0) { return false; }
	const int32_t k = (b.pos[1] >> kMoveShift) - 1;
	return MoveFootprintSolid(occ, g, b, k, k);
}

CVX_HD inline int64_t MoveAbs(int64_t v) { return v < 0 ? -v : v; }

// The whole move of a valid body over world `W` (the body's flags choose what lies outside the tile).
template <class Group>
CVX_HD inline cvx_move_result MoveBody(const CopyWorld &W, bool repeat, const cvx_move_body &body, const Group &g)
{
	const MoveOcc occ{ W, repeat, (body.flags & CVX_MOVE_SOLID_BELOW) != 0, (body.flags & CVX_MOVE_SOLID_SIDES) != 0 };
	MoveBox start;
	for (int a = 0; a < 3; a++) {
		start.pos[a] = body.pos[a];
		start.size[a] = body.size[a];
	}
	const int32_t dx = body.delta[0], dy = body.delta[1], dz = body.delta[2];
	uint32_t flags = MoveFootprintSolid(occ, g, start, start.First(1), start.Last(1)) ? (uint32_t)CVX_MOVED_STARTS_SOLID : 0u;
	// slide A: Y, X, Z
	MoveBox A = start;
	uint32_t blocked = 0u;
	if (dy) { blocked |= MoveLeg(occ, g, A, 1, dy); }
	if (dx) { blocked |= MoveLeg(occ, g, A, 0, dx); }
	if (dz) { blocked |= MoveLeg(occ, g, A, 2, dz); }
	MoveBox end = A;
	const uint32_t sideBits = 0x33u; // -X, +X, -Z, +Z
	if (body.stepUp > 0 && dy <= 0 && (blocked & sideBits) != 0u) {
		const bool grounded = dy < 0 ? (blocked & (1u << 2)) != 0u : MoveResting(occ, g, start);
		if (grounded) {
			MoveBox B = start;
			(void)MoveLeg(occ, g, B, 1, body.stepUp);
			const int32_t raised = B.pos[1] - start.pos[1];
			uint32_t blockedB = 0u;
			if (dx) { blockedB |= MoveLeg(occ, g, B, 0, dx); }
			if (dz) { blockedB |= MoveLeg(occ, g, B, 2, dz); }
			if (raised - dy > 0) { blockedB |= MoveLeg(occ, g, B, 1, -(raised - dy)); }
			const int64_t wayA = MoveAbs((int64_t)A.pos[0] - start.pos[0]) + MoveAbs((int64_t)A.pos[2] - start.pos[2]);
			const int64_t wayB = MoveAbs((int64_t)B.pos[0] - start.pos[0]) + MoveAbs((int64_t)B.pos[2] - start.pos[2]);
			if (wayB > wayA) {
				end = B;
				blocked = blockedB | (uint32_t)CVX_MOVED_STEPPED;
			}
		}
	}
	flags |= blocked;
	if (MoveResting(occ, g, end)) { flags |= (uint32_t)CVX_MOVED_RESTING; }
	cvx_move_result out;
	out.pos[0] = end.pos[0];
	out.pos[1] = end.pos[1];
	out.pos[2] = end.pos[2];
	out.flags = (int32_t)flags;
	return out;
}

CVX_HD inline cvx_move_result MoveInvalid(const cvx_move_body &body)
{
	cvx_move_result out;
	out.pos[0] = body.pos[0];
	out.pos[1] = body.pos[1];
	out.pos[2] = body.pos[2];
	out.flags = (int32_t)CVX_MOVED_INVALID;
	return out;
}

// ---- how many lanes a body is worth (the host-array call) ------------------------------------------------------------------------------------------------

// The columns of the body's largest leg region from its start: the footprint (the overlap and ground queries, the Y legs) and the swept
// rectangles of the X and Z legs (slabs entered x cross-section).
inline int64_t MoveLegRegion(const cvx_move_body &b)
{
	int64_t covered[3], entered[3];
	for (int a = 0; a < 3; a++) {
		const int64_t lo = b.pos[a], hi = (int64_t)b.pos[a] + b.size[a] - 1, d = b.delta[a];
		covered[a] = (hi >> kMoveShift) - (lo >> kMoveShift) + 1;
		entered[a] = d > 0 ? ((hi + d) >> kMoveShift) - (hi >> kMoveShift) : (lo >> kMoveShift) - ((lo + d) >> kMoveShift);
	}
	const int64_t foot = covered[0] * covered[2], sweepX = entered[0] * covered[2], sweepZ = entered[2] * covered[0];
	const int64_t sweep = sweepX > sweepZ ? sweepX : sweepZ;
	return foot > sweep ? foot : sweep;
}

// The lanes per body for a call whose largest leg region is `region` columns.  Thresholds: see DESIGN.md section 3 (cvx_world_move).
// ONE value serves the whole call, chosen by its LARGEST body: a single vehicle among thousands of one-voxel boxes gives every box 64 lanes, 63 of
// them idle.  A host with bodies of very different sizes makes one call per size class (or uses cvx_world_move_device and says lanesPerBody itself).
// The region is taken at the start position and leaves the step-up legs out: it is a launch heuristic, the result never depends on it.
inline int MoveLanesFor(int64_t region)
{
	return region <= 4 ? 1 : region <= 32 ? 4 : region <= 128 ? 16 : 64;
}

} // namespace cvxb
