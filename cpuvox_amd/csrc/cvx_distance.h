// cvx_distance.h -- the rules of cvx_world_distance (cvx_distance.hip): exact squared-distance fields of boxes of the device-resident world.
//
// Written once for the device AND the host (tests/test_world_distance_cpu.py compiles it with g++ through tests/distance_rules.cpp and compares
// it with the dense numpy model of tests/distancemodel.py):
//   DistanceColumn   column (x, z) as the rule sees it: the arena's column inside the world, an empty one plus the outside rule beyond it
//   DistanceAlongY   pass 1, straight from the runs: how far voxel y of a column is from the column's nearest solid (or air) voxel, capped
//   DistanceGrid     the box, its footprint grown by R and where an element lies in the two 16-bit intermediate arrays
//   DistancePassY / DistancePassZ / DistancePassX   one element of each pass; the kernels of cvx_distance.hip are these, a thread per element
//   DistanceMinPlus  h(j) = min over |d| <= R of g(j + d) + d^2, scanned outward from d = 0 until d^2 >= the best so far
//   DistanceField    the three passes over a box, an element at a time: the specification
// The transform is separable: with gY(x, z, y) the distance along Y inside column (x, z),
//   D(v) = min over (dx, dz) of gY(x + dx, z + dz, y)^2 + dx^2 + dz^2,
// and a term with |dx| > R, |dz| > R or gY > R is above R^2 whatever the rest, so windows of R and a cap just above R^2 lose nothing.  Every
// intermediate value is min(value, R^2 + 1) <= 65026: 16 bits.  Values above R^2 become CVX_DISTANCE_FAR only at the end.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_dense.h"

namespace cvxb {

// A column of all of space: the arena's runs for 0 <= y < dimY (none outside the world in X or Z), solid or air below and above them, or
// solid at every height (beyond a face of the world in X or Z whose solidOutside bit is set).
struct DistanceColumn {
	ArenaColumn col;
	bool allSolid, solidBelow, solidAbove;
};

CVX_HD inline DistanceColumn DistanceColumnAt(const CopyWorld &W, int64_t x, int64_t z, int solidOutside)
{
	const bool below = (solidOutside & 0x04) != 0, above = (solidOutside & 0x08) != 0;
	if (x < 0 || x >= W.dimX || z < 0 || z >= W.dimZ) {
		const bool all = (x < 0 && (solidOutside & 0x01)) || (x >= W.dimX && (solidOutside & 0x02)) || (z < 0 && (solidOutside & 0x10)) ||
		                 (z >= W.dimZ && (solidOutside & 0x20));
		return DistanceColumn{ ArenaColumn{ 0u, 0u, 0u, 0u, W.runs }, all, below, above }; // (record 0: the empty column)
	}
	return DistanceColumn{ CopyColumnAt(W, x, z), false, below, above };
}

// The nearest solid / air voxel of the arena's column at or below / at or above y, 0 <= y < dimY; -1 / dimY: there is none inside the world.
// Runs that touch (a foreign encoding) are walked through.
CVX_HD inline int64_t SolidAtOrBelow(const ArenaColumn &col, int64_t y)
{
	const uint32_t k = RunAtOrBelow(col, y);
	if (k >= col.Count()) { return -1; }
	const int64_t top = (int64_t)col.Run(k).top;
	return top > y ? y : top - 1;
}

CVX_HD inline int64_t SolidAtOrAbove(const ArenaColumn &col, int64_t y, int64_t dimY)
{
	const uint32_t k = RunAtOrBelow(col, y);
	if (k < col.Count() && (int64_t)col.Run(k).top > y) { return y; }
	return k > 0u ? (int64_t)col.Run(k - 1u).bottom : dimY; // (run k - 1 lies wholly above y)
}

CVX_HD inline int64_t AirAtOrBelow(const ArenaColumn &col, int64_t y)
{
	const uint32_t count = col.Count();
	uint32_t k = RunAtOrBelow(col, y);
	if (k >= count || (int64_t)col.Run(k).top <= y) { return y; }
	int64_t a = (int64_t)col.Run(k).bottom - 1;
	while (k + 1u < count && (int64_t)col.Run(k + 1u).top > a) { a = (int64_t)col.Run(++k).bottom - 1; }
	return a;
}

CVX_HD inline int64_t AirAtOrAbove(const ArenaColumn &col, int64_t y, int64_t dimY)
{
	uint32_t k = RunAtOrBelow(col, y);
	if (k >= col.Count() || (int64_t)col.Run(k).top <= y) { return y; }
	int64_t a = (int64_t)col.Run(k).top;
	while (k > 0u && (int64_t)col.Run(k - 1u).bottom <= a) { a = (int64_t)col.Run(--k).top; }
	return a < dimY ? a : dimY;
}

// Pass 1.  min(|y' - y|, R + 1) over the voxels y' of the column that are solid (toAir: that are air); y is any height, inside the world or not.
CVX_HD inline uint32_t DistanceAlongY(const DistanceColumn &c, int64_t dimY, int64_t y, int R, bool toAir)
{
	const int64_t cap = (int64_t)R + 1;
	if (c.allSolid) { return toAir ? (uint32_t)cap : 0u; }
	const bool below = c.solidBelow != toAir, above = c.solidAbove != toAir; // the half lines y' < 0 and y' >= dimY hold what is looked for
	if ((y < 0 && below) || (y >= dimY && above)) { return 0u; }
	int64_t best = cap;
	if (y >= 0) { // downwards: the arena from min(y, dimY - 1), then the half line below it
		const int64_t from = y < dimY ? y : dimY - 1;
		const int64_t at = toAir ? AirAtOrBelow(c.col, from) : SolidAtOrBelow(c.col, from);
		if (at >= 0) {
			best = y - at < best ? y - at : best;
		} else if (below) {
			best = y + 1 < best ? y + 1 : best;
		}
	}
	if (y < dimY) { // upwards
		const int64_t from = y > 0 ? y : 0;
		const int64_t at = toAir ? AirAtOrAbove(c.col, from, dimY) : SolidAtOrAbove(c.col, from, dimY);
		if (at < dimY) {
			best = at - y < best ? at - y : best;
		} else if (above) {
			best = dimY - y < best ? dimY - y : best;
		}
	}
	return (uint32_t)best;
}

// h(j) = min over |d| <= R of g(j + d) + d^2 with g(j + d) = centre[d * stride], capped.  Outward from d = 0: once d^2 >= the best so far no
// later term can win.  Every element centre[-R * stride .. R * stride] exists (the halo).
CVX_HD inline uint32_t DistanceMinPlus(const uint16_t *centre, int64_t stride, int R, uint32_t cap)
{
	uint32_t best = centre[0];
	for (int d = 1; d <= R; d++) {
		const uint32_t dd = (uint32_t)(d * d);
		if (dd >= best) { break; }
		const uint32_t a = (uint32_t)centre[-(int64_t)d * stride] + dd, b = (uint32_t)centre[(int64_t)d * stride] + dd;
		best = a < best ? a : best;
		best = b < best ? b : best;
	}
	return best < cap ? best : cap;
}

// The box, R and the two intermediate arrays:
//   fromY  (size.x + 2R) x (size.z + 2R) x size.y  pass 1's result squared, over the footprint grown by R on all four sides
//   fromZ  (size.x + 2R) x size.z x size.y         pass 2's, still grown in X
// both in the dense layout (x, then z, y fastest) of their own extents.
struct DistanceGrid {
	DenseBox box;
	int R, solidOutside;

	CVX_HD int64_t GrownX() const { return (int64_t)box.size[0] + 2 * R; }
	CVX_HD int64_t GrownZ() const { return (int64_t)box.size[2] + 2 * R; }
	CVX_HD uint64_t ElementsY() const { return (uint64_t)GrownX() * (uint64_t)GrownZ() * (uint64_t)box.size[1]; }
	CVX_HD uint64_t ElementsZ() const { return (uint64_t)GrownX() * (uint64_t)box.size[2] * (uint64_t)box.size[1]; }
	CVX_HD uint64_t Elements() const { return (uint64_t)box.size[0] * (uint64_t)box.size[2] * (uint64_t)box.size[1]; }
	CVX_HD uint32_t Cap() const { return (uint32_t)(R * R) + 1u; }
};

// Element i of an array of `inner` columns per x and sizeY voxels per column: its x, z and y (32-bit divisions whenever i allows them).
CVX_HD inline void DistanceSplit(uint64_t i, uint64_t sizeY, uint64_t inner, uint64_t *x, uint64_t *z, uint64_t *y)
{
	if (i <= 0xFFFFFFFFull) {
		const uint32_t column = (uint32_t)i / (uint32_t)sizeY, cx = column / (uint32_t)inner;
		*y = (uint32_t)i - column * (uint32_t)sizeY;
		*x = cx;
		*z = column - cx * (uint32_t)inner;
		return;
	}
	const uint64_t column = i / sizeY;
	*y = i - column * sizeY;
	*x = column / inner;
	*z = column - *x * inner;
}

// Element i of fromY.
CVX_HD inline uint16_t DistancePassY(const CopyWorld &W, const DistanceGrid &G, uint64_t i, bool toAir)
{
	const uint64_t sizeY = (uint64_t)G.box.size[1], gz = (uint64_t)G.GrownZ();
	uint64_t x, z, y;
	DistanceSplit(i, sizeY, gz, &x, &z, &y);
	const DistanceColumn c = DistanceColumnAt(W, (int64_t)G.box.min[0] - G.R + (int64_t)x, (int64_t)G.box.min[2] - G.R + (int64_t)z, G.solidOutside);
	const uint32_t d = DistanceAlongY(c, W.dimY, (int64_t)G.box.min[1] + (int64_t)y, G.R, toAir);
	const uint32_t dd = d * d;
	return (uint16_t)(dd < G.Cap() ? dd : G.Cap());
}

// Element i of fromZ: the min-plus along Z.
CVX_HD inline uint16_t DistancePassZ(const DistanceGrid &G, const uint16_t *fromY, uint64_t i)
{
	const uint64_t sizeY = (uint64_t)G.box.size[1], sizeZ = (uint64_t)G.box.size[2];
	uint64_t x, z, y;
	DistanceSplit(i, sizeY, sizeZ, &x, &z, &y);
	const uint64_t at = (x * (uint64_t)G.GrownZ() + z + (uint64_t)G.R) * sizeY + y;
	return (uint16_t)DistanceMinPlus(fromY + at, (int64_t)sizeY, G.R, G.Cap());
}

// Element i of the box: the min-plus along X, then the mode.  `previous`: what out[i] holds, read only by the signed mode's second transform.
//   toAir false: D_S(v), CVX_DISTANCE_FAR above R^2 (CVX_DISTANCE_TO_SOLID, and the first transform of CVX_DISTANCE_SIGNED)
//   toAir true:  D_A(v) (CVX_DISTANCE_TO_AIR); signedSecond: -D_A(v) where previous == 0, that is on the solid voxels, else previous
CVX_HD inline int32_t DistancePassX(const DistanceGrid &G, const uint16_t *fromZ, uint64_t i, bool signedSecond, int32_t previous)
{
	if (signedSecond && previous != 0) { return previous; }
	const uint64_t sizeY = (uint64_t)G.box.size[1], sizeZ = (uint64_t)G.box.size[2];
	uint64_t x, z, y;
	DistanceSplit(i, sizeY, sizeZ, &x, &z, &y);
	const uint64_t at = ((x + (uint64_t)G.R) * sizeZ + z) * sizeY + y;
	const uint32_t v = DistanceMinPlus(fromZ + at, (int64_t)(sizeZ * sizeY), G.R, G.Cap());
	const int32_t d = v > (uint32_t)(G.R * G.R) ? CVX_DISTANCE_FAR : (int32_t)v;
	return signedSecond ? -d : d;
}

// The whole call on the host, an element at a time; fromY / fromZ: scratch of G.ElementsY() / G.ElementsZ() entries.
inline void DistanceField(const CopyWorld &W, const DistanceGrid &G, int mode, uint16_t *fromY, uint16_t *fromZ, int32_t *out)
{
	for (int pass = 0; pass < (mode == CVX_DISTANCE_SIGNED ? 2 : 1); pass++) {
		const bool toAir = mode == CVX_DISTANCE_TO_AIR || pass == 1;
		for (uint64_t i = 0; i < G.ElementsY(); i++) { fromY[i] = DistancePassY(W, G, i, toAir); }
		for (uint64_t i = 0; i < G.ElementsZ(); i++) { fromZ[i] = DistancePassZ(G, fromY, i); }
		for (uint64_t i = 0; i < G.Elements(); i++) { out[i] = DistancePassX(G, fromZ, i, pass == 1, pass == 1 ? out[i] : 0); }
	}
}

} // namespace cvxb
