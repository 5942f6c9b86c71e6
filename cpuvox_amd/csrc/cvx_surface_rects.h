// cvx_surface_rects.h -- the rules of cvx_world_surface_rects (cvx_surface_rects.hip): cvx_world_surface's quads merged into rectangles.
//
// Written once for the device AND the host (tests/test_world_surface_rects_cpu.py compiles it with g++ through tests/surface_rects_rules.cpp and
// compares it with the dense model of tests/surfacerectsmodel.py), on top of cvxb::SurfaceWalk (cvx_surface.h): the strips ARE that walk's quads.
//   RectStrip      a strip as the passes keep it: bottom, length, colour.  Column and face follow from the pair the strip is listed under.
//   RectsPass      one merge pass over the listed strips: Follows, the contract's predicate (the position along the pass axis is the pair the
//                  second strip was found in), and the functions of one (column, face) pair,
//     Merge        which items of the pair are the first of their chain and how long the chain is: the pair one column back and the pair one
//                  column on are walked beside it with a cursor each (Seek): the lists descend in y, as SurfaceWalk subtracts a neighbour column
//     Chain        how long the chain of a first item is: a column forward at a time, from the third column on the strip of the same top is
//                  found by bisection (Find)
//   RectsMergePair every strip of the pair gets its extent along the pass axis, 0 when it was merged into the item before it
//   RectOf         the rectangle of a strip and its extents; RectCorners, the corners cvx_surface_rect_triangles winds like SurfaceCorners
// The pairs of a box are numbered column * 6 + face in its (x, then z) column order, as in cvx_surface.h: the next column along z is 6 pairs on,
// the next along x 6 * SizeZ.  A pass only reads what the pass before it wrote and writes one word per strip of its own pair: the pairs of a
// pass are independent of each other.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu_surface_rects.h"
#include "cvx_surface.h"

namespace cvxb {

struct RectStrip {
	int32_t bottom, length; // voxels bottom .. bottom + length - 1 of the pair's column
	uint32_t argb;
};

// faces 0, 1 merge along z; 2 .. 5 along x; the rows of faces 2, 3 then stack along z
CVX_HD inline bool RectsFirstPassAlongZ(int face) { return face < 2; }
CVX_HD inline bool RectsHasRowPass(int face) { return face == 2 || face == 3; }

// where a pair stands along a pass axis
struct RectsAxis {
	int64_t step;        // pairs from a column to the next one along the axis
	int64_t back, ahead; // columns of the box before and behind this one along the axis
};

CVX_HD inline RectsAxis RectsAxisOf(const PiecesBox &B, int64_t column, bool alongZ)
{
	const int64_t sizeZ = B.SizeZ(), xi = column / sizeZ, zi = column % sizeZ;
	return alongZ ? RectsAxis{ 6, zi, sizeZ - 1 - zi } : RectsAxis{ 6 * sizeZ, xi, (int64_t)B.SizeX() - 1 - xi };
}

struct RectsPass {
	const RectStrip *strips;   // every strip of the box in pair order, top-down inside a pair
	const uint32_t *offsets;   // pairs + 1: the first strip of every pair
	const uint32_t *rowExtent; // null in a first pass.  The row pass: what the pass along x gave every strip; its items are the strips with an
	                           // extent above 0 (the rows), and the extent is part of their identity
	bool ignoreColour;

	CVX_HD bool Item(uint32_t k) const { return !rowExtent || rowExtent[k] != 0u; }
	CVX_HD int32_t Top(uint32_t k) const { return strips[k].bottom + strips[k].length; }

	// item q, of the pair one column behind item p's along the pass axis, follows p (same face: the pairs are `step` apart)
	CVX_HD bool Follows(uint32_t p, uint32_t q) const
	{
		const RectStrip a = strips[p], b = strips[q];
		if (a.bottom != b.bottom || a.length != b.length) { return false; }
		if (rowExtent && (rowExtent[p] == 0u || rowExtent[p] != rowExtent[q])) { return false; }
		return ignoreColour || a.argb == b.argb;
	}

	// the strip with top `top` among the strips cursor .. end - 1 of a pair, or ~0u: the tops of a pair descend, and so do the tops asked for
	// while a pair is walked, so the cursor only moves forward
	CVX_HD uint32_t Seek(uint32_t *cursor, uint32_t end, int32_t top) const
	{
		while (*cursor < end && Top(*cursor) > top) { (*cursor)++; }
		return *cursor < end && Top(*cursor) == top ? *cursor : ~0u;
	}

	// the strip of `pair` whose top is `top`, or ~0u, by bisection
	CVX_HD uint32_t Find(int64_t pair, int32_t top) const
	{
		uint32_t lo = offsets[pair], hi = offsets[pair + 1];
		while (lo < hi) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			const int32_t t = Top(mid);
			if (t == top) { return mid; }
			if (t > top) { lo = mid + 1u; } else { hi = mid; }
		}
		return ~0u;
	}

	// The items of the chain that first item k of `pair` starts.  `next`: the strip of k's top in the pair one column on, or ~0u (the caller
	// walks that pair with a cursor, as it walks the one behind); the columns after it are searched.
	CVX_HD uint32_t Chain(int64_t pair, const RectsAxis &A, uint32_t k, uint32_t next) const
	{
		const int32_t top = Top(k);
		uint32_t n = 1u, last = k;
		for (int64_t c = 1; c <= A.ahead; c++) {
			const uint32_t q = c == 1 ? next : Find(pair + c * A.step, top);
			if (q == ~0u || !Follows(last, q)) { break; }
			last = q;
			n++;
		}
		return n;
	}

	// extent(k, n) for every strip k of `pair`, top-down: n = the items of its chain when k is an item that follows nothing, else 0.  The pair one
	// column back and the pair one column on are walked beside it with a cursor each.  Returns the first items.
	template <class Extent>
	CVX_HD uint32_t Merge(int64_t pair, const RectsAxis &A, Extent &&extent) const
	{
		const uint32_t begin = offsets[pair], end = offsets[pair + 1];
		uint32_t back = 0u, backEnd = 0u, on = 0u, onEnd = 0u, firsts = 0u;
		if (A.back > 0 && begin < end) {
			back = offsets[pair - A.step];
			backEnd = offsets[pair - A.step + 1];
		}
		if (A.ahead > 0 && begin < end) {
			on = offsets[pair + A.step];
			onEnd = offsets[pair + A.step + 1];
		}
		for (uint32_t k = begin; k < end; k++) {
			uint32_t n = 0u;
			if (Item(k)) {
				const int32_t top = Top(k);
				const uint32_t before = Seek(&back, backEnd, top);
				if (before == ~0u || !Follows(before, k)) { n = Chain(pair, A, k, Seek(&on, onEnd, top)); }
			}
			extent(k, n);
			firsts += n ? 1u : 0u;
		}
		return firsts;
	}
};

// One pass over one pair: extent[k] = the chain's items for a first item, 0 for every other strip of the pair.  Returns the first items.
CVX_HD inline uint32_t RectsMergePair(const RectsPass &P, int64_t pair, const RectsAxis &A, uint32_t *extent)
{
	return P.Merge(pair, A, [&](uint32_t k, uint32_t n) { extent[k] = n; });
}

// The rectangle of strip s of column (x, z), face `face`: `along` is its extent from the first pass, `rows` from the row pass (faces 2, 3).
CVX_HD inline cvx_surface_rect RectOf(const RectStrip &s, int32_t x, int32_t z, int face, uint32_t along, uint32_t rows)
{
	cvx_surface_rect r{ { x, s.bottom, z }, { 1, s.length, 1 }, face, s.argb };
	if (RectsFirstPassAlongZ(face)) {
		r.size[2] = (int32_t)along;
	} else {
		r.size[0] = (int32_t)along;
		if (RectsHasRowPass(face)) { r.size[2] = (int32_t)rows; }
	}
	return r;
}

// The corners of the rectangle on its face plane: c0, c0 + u, c0 + u + v, c0 + v with u x v along the face's outward axis, u and v those of
// SurfaceCorners stretched to the rectangle.
CVX_HD inline void RectCorners(const cvx_surface_rect &r, float out[4][3])
{
	const float sx = (float)r.size[0], sy = (float)r.size[1], sz = (float)r.size[2];
	float p[3] = { (float)r.voxel[0], (float)r.voxel[1], (float)r.voxel[2] }, u[3] = { 0.f, 0.f, 0.f }, v[3] = { 0.f, 0.f, 0.f };
	switch (r.face) {
	case 0: u[2] = sz; v[1] = sy; break;
	case 1: p[0] += 1.f; u[1] = sy; v[2] = sz; break;
	case 2: u[0] = sx; v[2] = sz; break;
	case 3: p[1] += 1.f; u[2] = sz; v[0] = sx; break;
	case 4: u[1] = sy; v[0] = sx; break;
	default: p[2] += 1.f; u[0] = sx; v[1] = sy; break;
	}
	for (int a = 0; a < 3; a++) {
		out[0][a] = p[a];
		out[1][a] = p[a] + u[a];
		out[2][a] = p[a] + u[a] + v[a];
		out[3][a] = p[a] + v[a];
	}
}

} // namespace cvxb
