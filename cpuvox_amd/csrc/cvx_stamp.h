// cvx_stamp.h -- stamping triangle meshes into the device-resident world (cvx_world_stamp_mesh, cvx_stamp.hip).
//
// The rules, written once for the device AND the host (tests/test_world_stamp_cpu.py compiles them with g++ through tests/stamp_rules.cpp and
// compares them with the host voxeliser and with numpy models):
//   TriangleSetup / TriangleHit / TriangleColour   the host voxeliser's VoxelizeTriangle (host/cvx_mesh.cpp; VoxelizerHelper.GetVoxelsInternal,
//                VoxelizerHelper.cs:28-132, and the material step of WordBuilder.cs:76-88) operation for operation, split so that a device
//                thread can take one (x, z) column of a triangle's box: the setup once per triangle, the geometric test per voxel, the colour
//                per voxel that passes it.  VoxelizeTriangle strings them together in the host's loop order (x, then z, then y) with its cap.
//   MergeStamped the duplicates of one voxel: ToFinalColumn's average (host/cvx_world.cpp; WordBuilder.cs:192-228).
//   StampColumn  a column after the stamp, emitted as the builder emits it (BrushColumn's encoding, cvx_brush.h).
// Every float operation is the host's, in the host's order (the device unit builds with -ffp-contract=off and correctly rounded divide / sqrt).
// Where the host's result rests on a float -> int conversion of NaN or of a value outside the int range (x86-64: the "integer indefinite"
// 0x80000000), ToInt makes that conversion explicit, so that both sides compute the same thing.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu.h"
#include "cvx_brush.h"
#include "cvx_edit.h" // CVX_HD

namespace cvxs {

constexpr int kVoxelizeBufferMax = 1024 * 256; // VOXELIZE_BUFFER_MAX, WordBuilder.cs:37: hits per triangle

// (int)f as the x86-64 host build computes it (cvttss2si): NaN and values outside [-2^31, 2^31) give INT32_MIN
CVX_HD inline int32_t ToInt(float f) { return (f >= -2147483648.f && f < 2147483648.f) ? (int32_t)f : INT32_MIN; }
CVX_HD inline int ClampI(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// UnityEngine Color -> Color32: (byte)Mathf.Round(Mathf.Clamp01(c) * 255f); NaN passes the clamp and converts like the host (to 0)
CVX_HD inline uint32_t ToByte(float c)
{
	const float v = c < 0.f ? 0.f : (c > 1.f ? 1.f : c);
	return (uint32_t)ToInt(__builtin_nearbyintf(v * 255.f)) & 0xFFu;
}

struct V3 { float x, y, z; };
CVX_HD inline V3 Sub(V3 a, V3 b) { return V3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
CVX_HD inline V3 Add(V3 a, V3 b) { return V3{ a.x + b.x, a.y + b.y, a.z + b.z }; }
CVX_HD inline V3 Mul(V3 a, float s) { return V3{ a.x * s, a.y * s, a.z * s }; }
CVX_HD inline float Dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
CVX_HD inline V3 Cross(V3 a, V3 b) { return V3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
CVX_HD inline V3 Min3(V3 a, V3 b) { return V3{ __builtin_fminf(a.x, b.x), __builtin_fminf(a.y, b.y), __builtin_fminf(a.z, b.z) }; }
CVX_HD inline V3 Max3(V3 a, V3 b) { return V3{ __builtin_fmaxf(a.x, b.x), __builtin_fmaxf(a.y, b.y), __builtin_fmaxf(a.z, b.z) }; }
CVX_HD inline V3 Normalize(V3 a) { const float r = 1.0f / __builtin_sqrtf(Dot(a, a)); return Mul(a, r); }
CVX_HD inline V3 Position(const cvx_mesh_vertex &v) { return V3{ v.position[0], v.position[1], v.position[2] }; }

// What a triangle's voxels are tested against: the corners after the half-voxel extension, the unit normal and the clamped integer box
struct TriSetup {
	V3 a, b, c, n;
	int32_t lo[3], hi[3]; // inclusive
};

// false: the triangle has no area (the host returns before its loop)
CVX_HD inline bool TriangleSetup(const cvx_mesh_vertex &v0, const cvx_mesh_vertex &v1, const cvx_mesh_vertex &v2, int dimX, int dimY, int dimZ, TriSetup *s)
{
	V3 a = Position(v0), b = Position(v1), c = Position(v2);
	const V3 normalCross = Cross(Sub(b, a), Sub(c, a));
	const float normalCrossLengthSqrd = Dot(normalCross, normalCross);
	if (normalCrossLengthSqrd == 0.f) { return false; }
	s->n = Mul(normalCross, 1.0f / __builtin_sqrtf(normalCrossLengthSqrd));
	const V3 sum = Add(Add(a, b), c);
	const V3 middle{ sum.x / 3.f, sum.y / 3.f, sum.z / 3.f };
	a = Add(a, Mul(Normalize(Sub(a, middle)), 0.5f));
	b = Add(b, Mul(Normalize(Sub(b, middle)), 0.5f));
	c = Add(c, Mul(Normalize(Sub(c, middle)), 0.5f));
	s->a = a;
	s->b = b;
	s->c = c;
	const V3 minf = Min3(a, Min3(b, c)), maxf = Max3(a, Max3(b, c));
	const int dims[3] = { dimX, dimY, dimZ };
	const float mins[3] = { minf.x, minf.y, minf.z }, maxs[3] = { maxf.x, maxf.y, maxf.z };
	for (int k = 0; k < 3; k++) {
		s->lo[k] = ClampI(ToInt(__builtin_floorf(mins[k])), 0, dims[k] - 1);
		s->hi[k] = ClampI(ToInt(__builtin_ceilf(maxs[k])), 0, dims[k] - 1);
	}
	return true;
}

// The geometric test of voxel (x, y, z): within half a voxel of the plane and inside the extended triangle (NaN barycentrics pass, as on the
// host).  Out: the barycentric weights.
CVX_HD inline bool TriangleHit(const TriSetup &s, int x, int y, int z, float *bx, float *by, float *bz)
{
	const V3 voxel{ (float)x + 0.5f, (float)y + 0.5f, (float)z + 0.5f };
	const float normalDistToTriangle = Dot(Sub(voxel, s.a), s.n);
	if (__builtin_fabsf(normalDistToTriangle) > 0.5f) { return false; }
	const V3 p = Sub(voxel, Mul(s.n, normalDistToTriangle));
	const V3 p0 = Sub(s.b, s.a), p1 = Sub(s.c, s.a), p2 = Sub(p, s.a);
	const float d00 = Dot(p0, p0), d01 = Dot(p0, p1), d11 = Dot(p1, p1), d20 = Dot(p2, p0), d21 = Dot(p2, p1);
	const float denom = 1.f / (d00 * d11 - d01 * d01);
	const float wy = (d11 * d20 - d01 * d21) * denom;
	const float wz = (d00 * d21 - d01 * d20) * denom;
	const float wx = 1.0f - wy - wz;
	if (wx < 0.f || wy < 0.f || wz < 0.f || wx > 1.f || wy > 1.f || wz > 1.f) { return false; }
	*bx = wx;
	*by = wy;
	*bz = wz;
	return true;
}

// A material's diffuse texture as the kernels see it: RGBA8 rows (row 0 = the bottom one) at `texels` + offset; offset < 0: no texture
struct Texture {
	int32_t width, height;
	int64_t offset;
};

// MeshMaterial::GetDiffusePixel (host/cvx_mesh.cpp; SimpleMesh.cs:130-134): the pixel floor(uv * (size - 1)), clamped into the texture
CVX_HD inline void DiffusePixel(const Texture &t, const uint8_t *texels, float u, float v, float rgba[4])
{
	if (t.offset < 0 || t.width <= 0 || t.height <= 0) {
		rgba[0] = rgba[1] = rgba[2] = rgba[3] = 1.f;
		return;
	}
	const int px = ClampI(ToInt(__builtin_floorf(u * (float)(t.width - 1))), 0, t.width - 1);
	const int py = ClampI(ToInt(__builtin_floorf(v * (float)(t.height - 1))), 0, t.height - 1);
	const uint8_t *p = texels + t.offset + ((int64_t)px + (int64_t)py * t.width) * 4;
	const float inv255 = 1.f / 255.f;
	for (int i = 0; i < 4; i++) { rgba[i] = (float)p[i] * inv255; }
}

// The colour of a voxel that passed TriangleHit (ColorARGB32 byte order: a | r << 8 | g << 16 | b << 24); false: a texel with alpha < 1, no voxel.
// Material (sbyte)v0.material: an index outside 0 .. materialCount - 1 means no texture.
CVX_HD inline bool TriangleColour(const cvx_mesh_vertex &v0, const cvx_mesh_vertex &v1, const cvx_mesh_vertex &v2, float bx, float by, float bz,
                                  const Texture *materials, int materialCount, const uint8_t *texels, uint32_t *argb)
{
	const float inv255 = 1.f / 255.f;
	float rgb[3];
	for (int k = 0; k < 3; k++) {
		const float c0 = (float)v0.rgba[k] * inv255, c1 = (float)v1.rgba[k] * inv255, c2 = (float)v2.rgba[k] * inv255;
		rgb[k] = c0 * bx + c1 * by + c2 * bz;
	}
	bool keep = true;
	const int materialIndex = (int)(int8_t)v0.material;
	if (materialIndex >= 0 && materialIndex < materialCount) {
		const float u = v0.uv[0] * bx + v1.uv[0] * by + v2.uv[0] * bz;
		const float v = v0.uv[1] * bx + v1.uv[1] * by + v2.uv[1] * bz;
		float albedo[4];
		DiffusePixel(materials[materialIndex], texels, u, v, albedo);
		if (albedo[3] < 1.f) { keep = false; }
		for (int k = 0; k < 3; k++) { rgb[k] *= albedo[k]; }
	}
	*argb = 0xFFu | (ToByte(rgb[0]) << 8) | (ToByte(rgb[1]) << 16) | (ToByte(rgb[2]) << 24);
	return keep;
}

// VoxelizeTriangle in the host's loop order: emit(x, y, z, argb) for every voxel it keeps, at most kVoxelizeBufferMax hits (transparent ones
// count).  The host's reference for tests; the device splits the same loop over (x, z) columns.
template <class Emit>
CVX_HD inline void VoxelizeTriangle(const cvx_mesh_vertex &v0, const cvx_mesh_vertex &v1, const cvx_mesh_vertex &v2, int dimX, int dimY, int dimZ,
                                    const Texture *materials, int materialCount, const uint8_t *texels, Emit emit)
{
	TriSetup s;
	if (!TriangleSetup(v0, v1, v2, dimX, dimY, dimZ, &s)) { return; }
	int written = 0;
	for (int x = s.lo[0]; x <= s.hi[0]; x++) {
		for (int z = s.lo[2]; z <= s.hi[2]; z++) {
			for (int y = s.lo[1]; y <= s.hi[1]; y++) {
				float bx, by, bz;
				if (!TriangleHit(s, x, y, z, &bx, &by, &bz)) { continue; }
				uint32_t argb;
				if (TriangleColour(v0, v1, v2, bx, by, bz, materials, materialCount, texels, &argb)) { emit(x, y, z, argb); }
				if (++written == kVoxelizeBufferMax) { return; }
			}
		}
	}
}

// ---- one column after the stamp ---------------------------------------------------------------------------------------------------------------

// The duplicates of one voxel (colours in ColorARGB32 byte order): per channel the sum divided by the count, alpha 255 (ToFinalColumn)
CVX_HD inline uint32_t MergeStamped(const uint32_t *argb, int count)
{
	uint32_t r = 0, g = 0, b = 0;
	for (int i = 0; i < count; i++) {
		r += (argb[i] >> 8) & 0xFFu;
		g += (argb[i] >> 16) & 0xFFu;
		b += argb[i] >> 24;
	}
	const uint32_t n = (uint32_t)count;
	return 0xFFu | ((r / n) << 8) | ((g / n) << 16) | ((b / n) << 24);
}

// Walks the column top-down with the stamped voxels (stampY strictly descending, stampArgb their merged colours; m of them):
// FILL -> solid(stamped colour), CARVE -> air, PAINT -> solid ? solid(stamped colour) : air; every other voxel keeps what the arena holds.
// Outputs as BrushColumn (cvx_brush.h): runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours top-down; either may be null.
CVX_HD inline cvxb::BrushResult StampColumn(const cvxb::ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const uint32_t *stampY,
                                            const uint32_t *stampArgb, int m, int op, int dimY, uint32_t *outRuns, uint32_t *outColours)
{
	cvxb::BrushResult res{ 0u, 0u, 0u, 0u, false };
	const uint32_t solidRuns = col.Count();
	uint32_t k = 0;                      // the arena run at or below y
	int s = 0;                           // the stamped voxel at or below y
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0; // the run being emitted
	int64_t lowest = -1, highest = -1;   // solid voxels
	int64_t y = (int64_t)dimY - 1;
	while (y >= 0) {
		while (k < solidRuns && (int64_t)col.Run(k).bottom > y) { k++; }
		cvxb::SolidRun run{ 0u, 0u, 0u };
		bool origSolid = false;
		int64_t bottom = 0;
		if (k < solidRuns) {
			run = col.Run(k);
			origSolid = (int64_t)run.top > y;
			bottom = origSolid ? (int64_t)run.bottom : (int64_t)run.top;
		}
		while (s < m && (int64_t)stampY[s] > y) { s++; }
		const bool stamped = s < m && (int64_t)stampY[s] == y;
		if (stamped) {
			bottom = y;
		} else if (s < m && (int64_t)stampY[s] + 1 > bottom) {
			bottom = (int64_t)stampY[s] + 1;
		}
		const bool solid = stamped ? (op == CVX_BRUSH_FILL || (op == CVX_BRUSH_PAINT && origSolid)) : origSolid;
		const int64_t length = y + 1 - bottom;
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
				for (int64_t v = y; v >= bottom; v--) {
					outColours[res.colours + (uint32_t)(y - v)] = stamped ? stampArgb[s]
					                                                      : colourSlots[col.ColorsBase() + ((run.colorsIndex + (run.top - 1u - (uint32_t)v)) << (colorShift - 2))];
				}
			}
			res.colours += (uint32_t)length;
			if (highest < 0) { highest = y + 1; }
			lowest = bottom;
		}
		y = bottom - 1;
	}
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

} // namespace cvxs
