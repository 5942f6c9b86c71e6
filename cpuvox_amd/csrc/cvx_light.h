// cvx_light.h -- the rules of cvx_world_light (cvx_light.hip): sky occlusion and sun shadows baked into the device-resident world.
//
// Written once for the device AND the host (tests/test_world_light_cpu.py compiles it with g++ through tests/light_rules.cpp and compares it with
// the dense model of tests/lightmodel.py).  Everything is decided by occupancy: `occ(x, y, z)` answers "is voxel (x, y, z) solid", false for every
// voxel outside the world.  The kernel answers from a bit brick in LDS (and from the records where the brick ends), the host from the records.
//   LightDirection  the 17 sky directions and their weights
//   SkyOpen / Sky   a direction is open when skyRange voxels along it are air; the sum of the open directions' weights, 0 .. 26
//   SunFacing       the part of |sunDir| whose face neighbours are air
//   SunLit          the shadow walk: the voxels the ray from the voxel's centre along sunDir passes, plane crossing by plane crossing
//   Shade           floor + sky term + sun term, 0 .. 255
//   ApplyShade      the shade baked into a colour word (bytes a, r, g, b: alpha is the LOW byte)
//   ArenaOcc        occupancy from the records of LOD 0
//   LightColumn     a column emitted as BrushColumn emits it (the builder's encoding), every solid voxel's colour passed through a functor
// No surface normals on purpose: the worlds are one or two voxel thick shells, whose occupancy neighbourhood is symmetric.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_pieces.h" // PiecesBox, PiecesClipBox, CopyWorld

namespace cvxb {

constexpr int kLightDirections = 18; // indices 0 .. 17, index 4 is (0, 0, 0): no direction
constexpr int kLightSkyTotal = 26;
constexpr int kLightMaxSkyRange = 32, kLightMaxSunRange = 4096, kLightMaxSunDir = 1024;

struct LightDims {
	int x, y, z;
	CVX_HD bool Holds(int64_t vx, int64_t vy, int64_t vz) const { return vx >= 0 && vx < x && vy >= 0 && vy < y && vz >= 0 && vz < z; }
};

// direction j: dy = j / 9 (0, 1), dx = (j % 9) / 3 - 1, dz = j % 3 - 1; the weight is 1 + dy; j = 4 is no direction (weight 0)
CVX_HD inline int LightDirection(int j, int *dx, int *dy, int *dz)
{
	*dy = j / 9;
	*dx = (j % 9) / 3 - 1;
	*dz = j % 3 - 1;
	return j == 4 ? 0 : 1 + *dy;
}

template <class Occ>
CVX_HD inline bool SkyOpen(const Occ &occ, int x, int y, int z, int dx, int dy, int dz, int skyRange)
{
	for (int s = 1; s <= skyRange; s++) {
		if (occ(x + s * dx, y + s * dy, z + s * dz)) { return false; }
	}
	return true;
}

template <class Occ>
CVX_HD inline int Sky(const Occ &occ, int x, int y, int z, int skyRange)
{
	int sky = 0;
	for (int j = 0; j < kLightDirections; j++) {
		int dx, dy, dz;
		const int weight = LightDirection(j, &dx, &dy, &dz);
		if (weight && SkyOpen(occ, x, y, z, dx, dy, dz, skyRange)) { sky += weight; }
	}
	return sky;
}

CVX_HD inline int LightSign(int v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }
CVX_HD inline int LightAbs(int v) { return v < 0 ? -v : v; }

// the sum of |S_i| over the axes whose face neighbour towards the sun is air; *den: over all axes
template <class Occ>
CVX_HD inline int SunFacing(const Occ &occ, int x, int y, int z, int sx, int sy, int sz, int *den)
{
	int facing = 0;
	if (sx != 0 && !occ(x + LightSign(sx), y, z)) { facing += LightAbs(sx); }
	if (sy != 0 && !occ(x, y + LightSign(sy), z)) { facing += LightAbs(sy); }
	if (sz != 0 && !occ(x, y, z + LightSign(sz))) { facing += LightAbs(sz); }
	*den = LightAbs(sx) + LightAbs(sy) + LightAbs(sz);
	return facing;
}

// The shadow walk of voxel (x, y, z) towards S = (sx, sy, sz) != 0.  Axis i crosses its k-th voxel plane at (2k - 1) / |S_i|; with P the product
// of the non-zero |S_i|, the pending crossing of axis i is t_i = (2k - 1) * P / |S_i|, an integer below 2^34 kept in 64 bits and advanced by
// 2 * P / |S_i|: comparing the t_i is comparing the fractions by cross-multiplication.  All axes that attain the smallest t_i step together.
template <class Occ>
CVX_HD inline bool SunLit(const Occ &occ, const LightDims &dims, int x, int y, int z, int sx, int sy, int sz, int sunRange)
{
	const int64_t ax = LightAbs(sx), ay = LightAbs(sy), az = LightAbs(sz);
	const int64_t never = INT64_MAX;
	const int64_t stepX = sx ? 2 * (ay ? ay : 1) * (az ? az : 1) : 0, stepY = sy ? 2 * (ax ? ax : 1) * (az ? az : 1) : 0, stepZ = sz ? 2 * (ax ? ax : 1) * (ay ? ay : 1) : 0;
	int64_t tx = sx ? stepX / 2 : never, ty = sy ? stepY / 2 : never, tz = sz ? stepZ / 2 : never;
	const int dx = LightSign(sx), dy = LightSign(sy), dz = LightSign(sz);
	for (int n = 0; n < sunRange; n++) {
		const int64_t t = tx < ty ? (tx < tz ? tx : tz) : (ty < tz ? ty : tz);
		if (tx == t) { x += dx; tx += stepX; }
		if (ty == t) { y += dy; ty += stepY; }
		if (tz == t) { z += dz; tz += stepZ; }
		if (!dims.Holds(x, y, z)) { return true; }
		if (occ(x, y, z)) { return false; }
	}
	return true;
}

CVX_HD inline int Shade(const cvx_light_params &P, int sky, int facing, int den, bool lit)
{
	const int skyTerm = P.skyLevel * sky / kLightSkyTotal;
	const int sunTerm = lit && den > 0 ? P.sunLevel * facing / den : 0;
	const int shade = P.floorLevel + skyTerm + sunTerm;
	return shade > 255 ? 255 : shade;
}

// The shade of solid voxel (x, y, z): `near` answers the sky directions and the face neighbours (at most max(skyRange, 1) voxels away), `any` the
// shadow walk.  The walk is skipped where its answer cannot matter.
template <class Near, class Any>
CVX_HD inline int VoxelShade(const Near &near, const Any &any, const LightDims &dims, const cvx_light_params &P, int x, int y, int z)
{
	const int sky = P.skyRange > 0 ? Sky(near, x, y, z, P.skyRange) : kLightSkyTotal;
	int facing = 0, den = 0;
	bool lit = false;
	if (P.sunDir[0] != 0 || P.sunDir[1] != 0 || P.sunDir[2] != 0) {
		facing = SunFacing(any, x, y, z, P.sunDir[0], P.sunDir[1], P.sunDir[2], &den);
		lit = P.sunLevel * facing >= den && SunLit(any, dims, x, y, z, P.sunDir[0], P.sunDir[1], P.sunDir[2], P.sunRange);
	}
	return Shade(P, sky, facing, den, lit);
}

// colour word: bytes a, r, g, b (ColorARGB32's memory order), so alpha is bits 0 .. 7
CVX_HD inline uint32_t ApplyShade(uint32_t colour, int shade, int target)
{
	if (target == CVX_LIGHT_TO_ALPHA) { return (colour & 0xFFFFFF00u) | (uint32_t)shade; }
	uint32_t out = colour & 0xFFu;
	for (int shift = 8; shift < 32; shift += 8) { out |= ((((colour >> shift) & 0xFFu) * (uint32_t)shade + 127u) / 255u) << shift; }
	return out;
}

// occupancy from the records of LOD 0 (air outside the world)
struct ArenaOcc {
	CopyWorld W;
	CVX_HD bool operator()(int64_t x, int64_t y, int64_t z) const
	{
		if (x < 0 || x >= W.dimX || y < 0 || y >= W.dimY || z < 0 || z >= W.dimZ) { return false; }
		const ArenaColumn col = CopyColumnAt(W, x, z);
		if (col.x == 0u || y >= (int64_t)col.WorldMax() || y < (int64_t)col.WorldMin()) { return false; }
		const uint32_t k = RunAtOrBelow(col, y);
		return k < col.Count() && (int64_t)col.Run(k).top > y;
	}
};

// Column (cx, cz) as the arena holds it, emitted as BrushColumn emits it: maximal runs from the top (a foreign column's split runs merge), one
// colour per solid voxel (shared colours unshared), each passed through recolour(y, colour).
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
template <class Recolour>
CVX_HD inline BrushResult LightColumn(const CopyWorld &W, int64_t cx, int64_t cz, uint32_t *outRuns, uint32_t *outColours, const Recolour &recolour)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	const ArenaColumn col = CopyColumnAt(W, cx, cz);
	const uint32_t solidRuns = col.Count();
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0;
	int64_t lowest = -1, highest = -1;
	int64_t y = (int64_t)W.dimY - 1; // the next voxel to emit
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
					const uint32_t c = W.colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - (uint32_t)v)) << (W.colorShift - 2))];
					outColours[res.colours + (uint32_t)(y - v)] = recolour((int)v, c);
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
		span(true, (int64_t)run.top - run.bottom, run);
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

struct LightKeep {
	CVX_HD uint32_t operator()(int, uint32_t c) const { return c; }
};

// the colour of voxel (cx, y, cz) after the call, every test answered from the records: the record-walking route and the host's
struct LightFromRecords {
	ArenaOcc occ;
	PiecesBox B;
	cvx_light_params P;
	int cx, cz;
	CVX_HD uint32_t operator()(int y, uint32_t c) const
	{
		if (cx < B.x0 || cx >= B.x1 || cz < B.z0 || cz >= B.z1 || y < B.y0 || y >= B.y1) { return c; }
		const LightDims dims{ occ.W.dimX, occ.W.dimY, occ.W.dimZ };
		return ApplyShade(c, VoxelShade(occ, occ, dims, P, cx, y, cz), P.target);
	}
};

// cvx_world_light's argument rule (besides the context, the world and levelCount): 0, or which member is wrong
CVX_HD inline const char *LightParamsError(const cvx_light_params &P)
{
	for (int a = 0; a < 3; a++) {
		if (P.boxMin[a] >= P.boxMax[a]) { return "boxMin >= boxMax"; }
		if (P.sunDir[a] < -kLightMaxSunDir || P.sunDir[a] > kLightMaxSunDir) { return "sunDir"; }
	}
	if (P.sunLevel < 0 || P.sunLevel > 255) { return "sunLevel"; }
	if (P.skyLevel < 0 || P.skyLevel > 255) { return "skyLevel"; }
	if (P.floorLevel < 0 || P.floorLevel > 255) { return "floorLevel"; }
	if (P.sunRange < 0 || P.sunRange > kLightMaxSunRange) { return "sunRange"; }
	if (P.skyRange < 0 || P.skyRange > kLightMaxSkyRange) { return "skyRange"; }
	if (P.target != CVX_LIGHT_TO_RGB && P.target != CVX_LIGHT_TO_ALPHA) { return "target"; }
	return nullptr;
}

} // namespace cvxb
