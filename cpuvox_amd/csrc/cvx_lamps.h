// cvx_lamps.h -- the rules of cvx_world_light_lamps (cvx_light.hip): point lights added to the shade cvx_world_light bakes.
//
// Written once for the device AND the host, like cvx_light.h, which it builds on (tests/test_world_lamps_cpu.py compiles it with g++ through
// tests/lamp_rules.cpp and compares it with the dense model of tests/lampmodel.py).  Exact integers from end to end.  For solid voxel v, a lamp at
// voxel L with D = L - v, d2 = |D|^2, r2 = radius^2:
//   LampLit            the shadow walk from the centre of v along D: SunLit's stepping, ended by the arrival at L (L itself is not tested)
//   LampTerm           lit ? level * (r2 - d2) * facing / (r2 * den) : 0, facing and den as SunFacing with S = D
//   LampVoxelTerm      the term of one lamp for one voxel, the walk skipped where the term is 0 anyway
//   VoxelShadeLamps    min(255, floor + sky + sun + the sum over the lamps)
//   LightLampsFromRecords  LightFromRecords with the lamps: every lamp for every voxel, no cull (the record-walking route and the host's)
//   LampParamsError    the call's argument rule for the lamps
#pragma once

#include "cvx_light.h"

namespace cvxb {

constexpr int kLampMaxCount = CVX_LIGHT_MAX_LAMPS, kLampMaxRadius = CVX_LAMP_MAX_RADIUS, kLampMaxPos = 1 << 20;

// The walk of voxel (x, y, z) towards the voxel D = (dx, dy, dz) != 0 away, every |D_i| <= 64.  Axis i crosses its k-th plane at (2k - 1) / |D_i|;
// with P the product of the non-zero |D_i| the pending crossing is t_i = (2k - 1) * P / |D_i| <= 127 * 64 * 64: 32 bits hold it.  The last crossing
// of axis i is its |D_i|-th (at (2 |D_i| - 1) / (2 |D_i|) < 1 of the way), so after |D_x| + |D_y| + |D_z| axis steps the walk stands in L exactly:
// `left` counts them down.  Outside the world is air (occ says so) and the walk goes on.
template <class Occ>
CVX_HD inline bool LampLit(const Occ &occ, int x, int y, int z, int dx, int dy, int dz)
{
	const int ax = LightAbs(dx), ay = LightAbs(dy), az = LightAbs(dz);
	const int never = INT32_MAX;
	const int stepX = dx ? 2 * (ay ? ay : 1) * (az ? az : 1) : 0, stepY = dy ? 2 * (ax ? ax : 1) * (az ? az : 1) : 0, stepZ = dz ? 2 * (ax ? ax : 1) * (ay ? ay : 1) : 0;
	int tx = dx ? stepX / 2 : never, ty = dy ? stepY / 2 : never, tz = dz ? stepZ / 2 : never;
	const int sx = LightSign(dx), sy = LightSign(dy), sz = LightSign(dz);
	int left = ax + ay + az;
	for (;;) {
		const int t = tx < ty ? (tx < tz ? tx : tz) : (ty < tz ? ty : tz);
		if (tx == t) { x += sx; tx += stepX; left--; }
		if (ty == t) { y += sy; ty += stepY; left--; }
		if (tz == t) { z += sz; tz += stepZ; left--; }
		if (left <= 0) { return true; } // arrived at L
		if (occ(x, y, z)) { return false; }
	}
}

// level <= 255, r2 - d2 <= 4096, facing <= den <= 3 * 63: the numerator stays below 2^28, one floored division in 32 bits gives what 64 would
CVX_HD inline int LampTerm(int level, int r2, int d2, int facing, int den, bool lit)
{
	return lit && den > 0 ? (int)((uint32_t)(level * (r2 - d2) * facing) / (uint32_t)(r2 * den)) : 0;
}

// the term of the lamp at (lx, ly, lz) for solid voxel (x, y, z); `any` answers the face neighbours and the walk
template <class Any>
CVX_HD inline int LampVoxelTerm(const Any &any, int x, int y, int z, int lx, int ly, int lz, int radius, int level)
{
	const int dx = lx - x, dy = ly - y, dz = lz - z;
	if (LightAbs(dx) >= radius || LightAbs(dy) >= radius || LightAbs(dz) >= radius) { return 0; } // (and no square can overflow below)
	const int d2 = dx * dx + dy * dy + dz * dz, r2 = radius * radius;
	if (d2 == 0 || d2 >= r2 || level == 0) { return 0; }
	int den = 0;
	const int facing = SunFacing(any, x, y, z, dx, dy, dz, &den);
	if (level * (r2 - d2) * facing < r2 * den) { return 0; } // the term floors to 0 (facing == 0 among them): no walk
	return LampTerm(level, r2, d2, facing, den, LampLit(any, x, y, z, dx, dy, dz));
}

template <class Any>
CVX_HD inline int LampSum(const Any &any, int x, int y, int z, const cvx_lamp *lamps, int lampCount)
{
	int sum = 0;
	for (int l = 0; l < lampCount; l++) { sum += LampVoxelTerm(any, x, y, z, lamps[l].pos[0], lamps[l].pos[1], lamps[l].pos[2], lamps[l].radius, lamps[l].level); }
	return sum;
}

// (min(255, min(255, a) + b) = min(255, a + b) for b >= 0: the sum is added to what VoxelShade gives; at most 4096 * 255 + 255, no overflow)
template <class Near, class Any>
CVX_HD inline int VoxelShadeLamps(const Near &near, const Any &any, const LightDims &dims, const cvx_light_params &P, int x, int y, int z, const cvx_lamp *lamps,
                                  int lampCount)
{
	const int shade = VoxelShade(near, any, dims, P, x, y, z);
	if (shade >= 255) { return 255; }
	const int lit = shade + LampSum(any, x, y, z, lamps, lampCount);
	return lit > 255 ? 255 : lit;
}

// LightFromRecords with the lamps
struct LightLampsFromRecords {
	ArenaOcc occ;
	PiecesBox B;
	cvx_light_params P;
	int cx, cz;
	const cvx_lamp *lamps;
	int lampCount;
	CVX_HD uint32_t operator()(int y, uint32_t c) const
	{
		if (cx < B.x0 || cx >= B.x1 || cz < B.z0 || cz >= B.z1 || y < B.y0 || y >= B.y1) { return c; }
		const LightDims dims{ occ.W.dimX, occ.W.dimY, occ.W.dimZ };
		return ApplyShade(c, VoxelShadeLamps(occ, occ, dims, P, cx, y, cz, lamps, lampCount), P.target);
	}
};

// cvx_world_light_lamps' argument rule for the lamps: 0, or what is wrong
inline const char *LampParamsError(const cvx_lamp *lamps, int lampCount)
{
	if (lampCount < 0 || lampCount > kLampMaxCount) { return "lampCount"; }
	if (lampCount > 0 && !lamps) { return "lamps (NULL)"; }
	for (int l = 0; l < lampCount; l++) {
		if (lamps[l].radius < 1 || lamps[l].radius > kLampMaxRadius) { return "radius"; }
		if (lamps[l].level < 0 || lamps[l].level > 255) { return "level"; }
		for (int a = 0; a < 3; a++) {
			if (lamps[l].pos[a] < -kLampMaxPos || lamps[l].pos[a] > kLampMaxPos) { return "pos"; }
		}
	}
	return nullptr;
}

} // namespace cvxb
