// cvx_surface.h -- the rules of cvx_world_surface (cvx_surface.hip): the exposed faces of the device-resident world as coloured quads.
//
// Written once for the device AND the host (tests/test_world_surface_cpu.py compiles it with g++ through tests/surface_rules.cpp and compares it
// with the dense model of tests/surfacemodel.py; tools/surface_bench.py times the same walk as the host route):
//   SurfaceWalk       the quads of one (column, face) pair of the clipped box, top-down, handed to a sink: the count pass and the write pass of
//                     cvx_surface.hip call it with different sinks, so they cannot disagree
//   SurfaceCorners    the four corners of a quad's rectangle, wound so that (c1 - c0) x (c2 - c0) points out of the solid (cvx_surface_triangles)
//   SurfaceVertexRgba the vertex colour for which cvx_world_stamp_mesh (cvx_stamp.h, TriangleColour) writes the quad's colour word
// The box (PiecesBox, PiecesClipBox) is cvx_pieces.h's; the pairs of a box are numbered column * 6 + face in its (x, then z) column order, so the
// quads in pair order, top-down inside a pair, are in the order of the contract with no sort.
// A side face (-X, +X, -Z, +Z) subtracts the neighbour column's solid runs from the column's own with two cursors: the cost is runs, not voxels,
// and a colour is read only for a voxel whose face is exposed.  A -Y / +Y face looks at the two ends of every run.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_pieces.h"

namespace cvxb {

// the colour word of voxel v of `run`, from where PickColour reads it
CVX_HD inline uint32_t SurfaceColour(const CopyWorld &W, const ArenaColumn &col, const SolidRun &run, uint32_t v)
{
	return W.colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - v)) << (W.colorShift - 2))];
}

// The quads of one side pair as they grow: exposed spans arrive top-down; a span that starts where the last one ended continues the open quad
// (two runs of a foreign column that touch in space), a colour change ends it unless the call ignores colours.
template <class Sink>
struct SurfaceQuads {
	const CopyWorld &W;
	const ArenaColumn &col;
	int32_t x, z, face;
	bool ignoreColour;
	Sink &sink;
	bool open;
	int64_t top, bottom; // the open quad: voxels bottom .. top - 1
	uint32_t argb;

	CVX_HD void Flush()
	{
		if (open) { sink(cvx_surface_quad{ { x, (int32_t)bottom, z }, face, (int32_t)(top - bottom), argb }); }
		open = false;
	}
	// the voxels a .. b - 1 of `run`, all exposed
	CVX_HD void Span(const SolidRun &run, int64_t a, int64_t b)
	{
		if (open && b != bottom) { Flush(); }
		if (ignoreColour) {
			if (!open) {
				open = true;
				top = b;
				argb = SurfaceColour(W, col, run, (uint32_t)(b - 1));
			}
			bottom = a;
			return;
		}
		for (int64_t v = b - 1; v >= a; v--) {
			const uint32_t c = SurfaceColour(W, col, run, (uint32_t)v);
			if (open && c != argb) { Flush(); }
			if (!open) {
				open = true;
				top = v + 1;
				argb = c;
			}
			bottom = v;
		}
	}
};

// sink(const cvx_surface_quad &) for every quad of face `face` (0..5 = -X, +X, -Y, +Y, -Z, +Z) of column (x, z) of the clipped box B, by
// descending y.  The voxel across a face is read from the arena wherever it lies inside the world, inside the box or not; outside the world it
// is solid iff bit `face` of solidOutside is set.
template <class Sink>
CVX_HD inline void SurfaceWalk(const CopyWorld &W, const PiecesBox &B, int64_t x, int64_t z, int face, int solidOutside, int flags, Sink &&sink)
{
	const ArenaColumn col = CopyColumnAt(W, x, z);
	const uint32_t count = col.Count();
	if (count == 0u) { return; }
	const int64_t y0 = B.y0, y1 = B.y1;
	const bool outsideSolid = ((solidOutside >> face) & 1) != 0;
	uint32_t first, end;
	PiecesRunRange(col, y0, y1, &first, &end);
	if (face == 2 || face == 3) {
		for (uint32_t k = first; k < end; k++) {
			const SolidRun run = col.Run(k);
			int64_t v;
			bool solid;
			if (face == 3) { // the run's top voxel against the voxel above it: the run before, if it touches
				v = (int64_t)run.top - 1;
				solid = (int64_t)run.top >= W.dimY ? outsideSolid : (k > 0u && col.Run(k - 1u).bottom == run.top);
			} else {
				v = (int64_t)run.bottom;
				solid = v == 0 ? outsideSolid : (k + 1u < count && col.Run(k + 1u).top == run.bottom);
			}
			if (solid || v < y0 || v >= y1) { continue; }
			sink(cvx_surface_quad{ { (int32_t)x, (int32_t)v, (int32_t)z }, face, 1, SurfaceColour(W, col, run, (uint32_t)v) });
		}
		return;
	}
	const int64_t nx = x + (face == 0 ? -1 : face == 1 ? 1 : 0), nz = z + (face == 4 ? -1 : face == 5 ? 1 : 0);
	const bool inside = nx >= 0 && nx < W.dimX && nz >= 0 && nz < W.dimZ;
	if (!inside && outsideSolid) { return; }
	const ArenaColumn beside = inside ? CopyColumnAt(W, nx, nz) : ArenaColumn{ 0u, 0u, 0u, 0u, W.runs };
	const uint32_t besideCount = beside.Count();
	uint32_t j = RunAtOrBelow(beside, y1 - 1); // the neighbour's run at or below the cursor: the runs before j lie wholly above it
	SurfaceQuads<Sink> quads{ W, col, (int32_t)x, (int32_t)z, face, (flags & CVX_SURFACE_IGNORE_COLOUR) != 0, sink, false, 0, 0, 0u };
	for (uint32_t k = first; k < end; k++) {
		const SolidRun run = col.Run(k);
		const int64_t lo = (int64_t)run.bottom < y0 ? y0 : (int64_t)run.bottom;
		int64_t y = (int64_t)run.top > y1 ? y1 : (int64_t)run.top; // voxels lo .. y - 1 of the run are still to be decided
		while (y > lo) {
			while (j < besideCount && (int64_t)beside.Run(j).bottom >= y) { j++; }
			if (j >= besideCount) { // nothing of the neighbour at or below: the rest is exposed
				quads.Span(run, lo, y);
				break;
			}
			const SolidRun other = beside.Run(j);
			if ((int64_t)other.top >= y) { // covered down to the neighbour run's bottom
				y = (int64_t)other.bottom > lo ? (int64_t)other.bottom : lo;
			} else {
				const int64_t a = (int64_t)other.top > lo ? (int64_t)other.top : lo;
				quads.Span(run, a, y);
				y = a;
			}
		}
	}
	quads.Flush();
}

// The corners of the quad's rectangle on its face plane: c0, c0 + u, c0 + u + v, c0 + v with u x v along the face's outward axis.
CVX_HD inline void SurfaceCorners(const cvx_surface_quad &q, float out[4][3])
{
	const float x = (float)q.voxel[0], y = (float)q.voxel[1], z = (float)q.voxel[2], l = (float)q.length;
	float p[3] = { x, y, z }, u[3] = { 0.f, 0.f, 0.f }, v[3] = { 0.f, 0.f, 0.f };
	switch (q.face) {
	case 0: u[2] = 1.f; v[1] = l; break;
	case 1: p[0] = x + 1.f; u[1] = l; v[2] = 1.f; break;
	case 2: u[0] = 1.f; v[2] = 1.f; break;
	case 3: p[1] = y + l; u[2] = 1.f; v[0] = 1.f; break;
	case 4: u[1] = l; v[0] = 1.f; break;
	default: p[2] = z + 1.f; u[0] = 1.f; v[1] = l; break;
	}
	for (int a = 0; a < 3; a++) {
		out[0][a] = p[a];
		out[1][a] = p[a] + u[a];
		out[2][a] = p[a] + u[a] + v[a];
		out[3][a] = p[a] + v[a];
	}
}

// TriangleColour packs a | r << 8 | g << 16 | b << 24 with a = 0xFF: the vertex colour that gives back the word's r, g, b
CVX_HD inline void SurfaceVertexRgba(uint32_t argb, uint8_t rgba[4])
{
	rgba[0] = (uint8_t)(argb >> 8);
	rgba[1] = (uint8_t)(argb >> 16);
	rgba[2] = (uint8_t)(argb >> 24);
	rgba[3] = 0xFFu;
}

} // namespace cvxb
