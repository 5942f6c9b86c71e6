// cvx_brush.h -- voxel brushes and ray picking on the device-resident world (cvx_world_brush / cvx_world_pick, cvx_brush.hip).
//
// The per-column rules, written once for the device AND the host (tests/test_world_brush_cpu.py compiles them with g++ through
// tests/brush_rules.cpp and compares them with numpy models):
//   ArenaColumn  what a LOD-0 record of the arena says about its column: the solid runs top-down (records with 1 .. 3 runs, run-list blocks),
//                each with its colour index; colours at colorsBase + index << colorShift (blocks of 4 x 8 columns or column after column).
//   StrokeSpan   the y interval a stroke (box, sphere, capsule, ellipsoid) covers in a column: exact integers decide every voxel.
//                StrokeSpanUnclipped is the interval itself (cvx_model_brush.h: bodies have no frame), StrokeSpan its clip to the world's height.
//   StrokeCountValidate, StrokeShapesValidate  the stroke checks of cvx_world_brush and cvxd_models_brush, one copy.
//   BrushColumn  a column after a list of strokes, emitted as the builder emits it (WordBuilder.cs:181-268): maximal runs from the top, the
//                top air run first, ColorsIndex = solid voxels above, worldMin / worldMax as the RLEColumn constructor computes them.
//   PickRay      the first solid voxel along a ray (a 2-D DDA over the columns, one record per step, the solid runs walked in the ray's y order).
// Everything is read from where the record says it is: tail-moved blocks and run-list blocks of edited columns need nothing special.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu.h"
#include "cvx_edit.h" // CVX_HD

namespace cvxb {

// ---- reading a column of the arena (LOD 0: spans in voxels) -----------------------------------------------------------------------------------

struct SolidRun {
	uint32_t bottom, top; // voxels bottom .. top - 1
	uint32_t colorsIndex; // colour of voxel y: colorsIndex + (top - 1 - y)
};

struct ArenaColumn {
	uint32_t x, y, z, w;   // the record (cvx_device.h)
	const uint32_t *runs;  // the level's run list, 2 words per entry

	CVX_HD uint32_t Count() const { return x == 0u ? 0u : ((x >> 30) != 0u ? (x >> 30) : w); }
	CVX_HD uint32_t ColorsBase() const { return x & 0x3FFFFFFFu; }
	CVX_HD uint32_t WorldMin() const { return y & 0xFFFFu; }
	CVX_HD uint32_t WorldMax() const { return y >> 16; }
	// solid run k (0 = the top one) of a column with Count() > k
	CVX_HD SolidRun Run(uint32_t k) const
	{
		const uint32_t code = x >> 30;
		if (code == 0u) {
			const uint32_t w0 = runs[2u * (z + k)], w1 = runs[2u * (z + k) + 1u];
			return SolidRun{ w0 & 0xFFFFu, (w0 >> 16) + 1u, w1 & 0xFFFFu };
		}
		// record runs: run 0 = [w.lo, worldMax], run 1 = [z.lo, w.hi + 1], run 2 = [worldMin, z.hi + 1] (cvx_device.h); indices derived
		const uint32_t b0 = (code == 1u) ? WorldMin() : (w & 0xFFFFu), t0 = WorldMax();
		if (k == 0u) { return SolidRun{ b0, t0, 0u }; }
		const uint32_t b1 = (code == 2u) ? WorldMin() : (z & 0xFFFFu), t1 = (w >> 16) + 1u;
		if (k == 1u) { return SolidRun{ b1, t1, t0 - b0 }; }
		return SolidRun{ WorldMin(), (z >> 16) + 1u, (t0 - b0) + (t1 - b1) };
	}
};

// ---- strokes ----------------------------------------------------------------------------------------------------------------------------------

// Largest h >= 0 with h * h <= v (v >= 0): a float estimate corrected in integers, so that nothing but integers decides what is inside a sphere.
CVX_HD inline int64_t ISqrt(int64_t v)
{
	int64_t h = (int64_t)__builtin_sqrt((double)v);
	while (h > 0 && h * h > v) { h--; }
	while ((h + 1) * (h + 1) <= v) { h++; }
	return h;
}

// The unclipped box [lo, hi) per axis (x, y, z) that holds every voxel of a stroke of any shape: the host's rectangle (cvx_brush.hip, Footprint) and
// the kernels' cull (StrokeMeetsStrip) both come from here, so they cannot disagree.  (A stroke cvx_world_brush accepted: nothing overflows.)
CVX_HD inline void StrokeFootprint(const cvx_brush_stroke &s, int64_t lo[3], int64_t hi[3])
{
	for (int a = 0; a < 3; a++) {
		const int64_t p = s.a[a], q = s.b[a];
		if (s.shape == CVX_SHAPE_BOX) {
			lo[a] = p;
			hi[a] = q;
		} else if (s.shape == CVX_SHAPE_CAPSULE) {
			lo[a] = (p < q ? p : q) - s.pad_;
			hi[a] = (p < q ? q : p) + s.pad_ + 1;
		} else {
			const int64_t r = s.shape == CVX_SHAPE_SPHERE ? s.b[0] : q;
			lo[a] = p - r;
			hi[a] = p + r + 1;
		}
	}
}

// The limits of include/cpuvox_gpu.h: the span rules are exact in int64 inside them.
constexpr int kCapsuleMax = 8191, kEllipsoidMax = 1024;

// The stroke checks of cvx_world_brush and cvxd_models_brush, in the order include/cpuvox_gpu.h lists them: the list (StrokeCountValidate), then
// every stroke's op and shape (StrokeShapesValidate; cvx_world_brush checks its levelCount between the two); false: the message says what.
// (Plain host functions: not CVX_HD.)
inline bool StrokeCountValidate(const cvx_brush_stroke *strokes, int strokeCount, char *message, size_t bytes)
{
	if (!strokes || strokeCount <= 0 || strokeCount > CVX_BRUSH_MAX_STROKES) {
		snprintf(message, bytes, "strokeCount %d outside 1 .. %d", strokeCount, CVX_BRUSH_MAX_STROKES);
		return false;
	}
	return true;
}

inline bool StrokeShapesValidate(const cvx_brush_stroke *strokes, int strokeCount, char *message, size_t bytes)
{
	for (int s = 0; s < strokeCount; s++) {
		const cvx_brush_stroke &k = strokes[s];
		if (k.op < CVX_BRUSH_FILL || k.op > CVX_BRUSH_PAINT) {
			snprintf(message, bytes, "stroke %d: bad op %d", s, k.op);
			return false;
		}
		if (k.shape != CVX_SHAPE_BOX && k.shape != CVX_SHAPE_SPHERE && k.shape != CVX_SHAPE_CAPSULE && k.shape != CVX_SHAPE_ELLIPSOID) {
			snprintf(message, bytes, "stroke %d: bad shape %d", s, k.shape);
			return false;
		}
		if (k.shape == CVX_SHAPE_SPHERE && (k.b[0] < 0 || k.b[0] > (1 << 30))) {
			snprintf(message, bytes, "stroke %d: sphere radius %d outside 0 .. 2^30", s, k.b[0]);
			return false;
		}
		if (k.shape == CVX_SHAPE_CAPSULE) {
			if (k.pad_ < 0 || k.pad_ > kCapsuleMax) {
				snprintf(message, bytes, "stroke %d: capsule radius %d outside 0 .. %d", s, k.pad_, kCapsuleMax);
				return false;
			}
			for (int a = 0; a < 3; a++) {
				const int64_t d = (int64_t)k.b[a] - k.a[a];
				if (d < -kCapsuleMax || d > kCapsuleMax) {
					snprintf(message, bytes, "stroke %d: capsule ends %lld apart on axis %d, more than %d", s, (long long)d, a, kCapsuleMax);
					return false;
				}
				if (k.a[a] < -(1 << 30) || k.a[a] > (1 << 30)) {
					snprintf(message, bytes, "stroke %d: capsule end a[%d] = %d outside -2^30 .. 2^30", s, a, k.a[a]);
					return false;
				}
			}
		}
		if (k.shape == CVX_SHAPE_ELLIPSOID) {
			for (int a = 0; a < 3; a++) {
				if (k.b[a] < 1 || k.b[a] > kEllipsoidMax) {
					snprintf(message, bytes, "stroke %d: ellipsoid radius b[%d] = %d outside 1 .. %d", s, a, k.b[a], kEllipsoidMax);
					return false;
				}
			}
		}
	}
	return true;
}

// floor(n / q) for q > 0, in 32 bits (the capsule's slab bounds: |n| < 2^30)
CVX_HD inline int64_t FloorDiv32(int32_t n, int32_t q)
{
	const int32_t d = n / q;
	return (int64_t)(n % q < 0 ? d - 1 : d);
}

// The part of a capsule's column strictly between its end planes, as offsets t = y - a[1]: the integers with 0 < p0 + t * dy < L (the slab) and
// f(t) = a2 t^2 - 2 b1 t + c0 <= 0 (within r of the axis; a2 = dx^2 + dz^2 > 0, b1 = p0 * dy, c0 = (wx^2 + wz^2 - r^2) * L - p0^2), cut to [tMin, tMax].
// f's roots need a discriminant of up to 85 bits: they are estimated in float64 (off by at most 8 / sqrt(a2) + 1, since p0^2 <= a2 (wx^2 + wz^2)) and
// walked to the exact integers with f itself, which fits in int64 for |t| <= 16382 (a2 t^2 < 2^55, 2 b1 t < 2^57, c0 < 2^58).
CVX_HD inline void CapsuleMiddle(int64_t a2, int64_t b1, int64_t c0, int64_t p0, int64_t dy, int64_t L, int64_t tMin, int64_t tMax, int64_t *outLo, int64_t *outHi)
{
	*outLo = 0;
	*outHi = -1;
	int64_t lo = tMin, hi = tMax;
	if (dy == 0) {
		if (!(p0 > 0 && p0 < L)) { return; }
	} else {
		const int32_t q = (int32_t)(dy > 0 ? dy : -dy);
		const int64_t first = FloorDiv32((int32_t)(dy > 0 ? -p0 : p0 - L), q) + 1, last = FloorDiv32((int32_t)(dy > 0 ? L - p0 : p0) - 1, q);
		lo = first > lo ? first : lo;
		hi = last < hi ? last : hi;
	}
	if (lo > hi) { return; }
	const double fa = (double)a2, fb = (double)b1, vertex = fb / fa, disc = fb * fb - fa * (double)c0;
	const double reach = disc > 0.0 ? __builtin_sqrt(disc) / fa : 0.0;
	const double from = __builtin_floor(vertex - reach) - 1.0, to = __builtin_ceil(vertex + reach) + 1.0; // (the integer nearest the vertex lies strictly between)
	int64_t t1 = from < (double)lo ? lo : (from > (double)hi ? hi : (int64_t)from), t2 = to > (double)hi ? hi : (to < (double)lo ? lo : (int64_t)to);
	while (t1 > lo && (a2 * (t1 - 1) - 2 * b1) * (t1 - 1) + c0 <= 0) { t1--; }
	while (t1 <= t2 && (a2 * t1 - 2 * b1) * t1 + c0 > 0) { t1++; }
	while (t2 < hi && (a2 * (t2 + 1) - 2 * b1) * (t2 + 1) + c0 <= 0) { t2++; }
	while (t2 >= t1 && (a2 * t2 - 2 * b1) * t2 + c0 > 0) { t2--; }
	*outLo = t1;
	*outHi = t2;
}

// The y interval [lo, hi) a stroke covers in column (cx, cz), clipped to nothing; lo >= hi: none.  The rules are those of include/cpuvox_gpu.h; a
// capsule's and an ellipsoid's products are formed only for columns inside the footprint, which keeps them in int64 for strokes far from the
// column.  (A sphere's are formed for every column, as they always were: a caller whose columns can lie 2^31 from the stroke tests
// StrokeFootprint first, as cvx_model_brush.h does.)
CVX_HD inline void StrokeSpanUnclipped(const cvx_brush_stroke &s, int64_t cx, int64_t cz, int64_t *lo, int64_t *hi)
{
	int64_t l = 0, h = 0;
	if (s.shape == CVX_SHAPE_BOX) {
		if (cx >= s.a[0] && cx < s.b[0] && cz >= s.a[2] && cz < s.b[2]) { l = s.a[1]; h = s.b[1]; }
	} else if (s.shape == CVX_SHAPE_SPHERE) {
		const int64_t r = s.b[0], dx = cx - s.a[0], dz = cz - s.a[2];
		const int64_t left = r * r - dx * dx - dz * dz;
		if (left >= 0) {
			const int64_t e = ISqrt(left);
			l = (int64_t)s.a[1] - e;
			h = (int64_t)s.a[1] + e + 1;
		}
	} else if (s.shape == CVX_SHAPE_ELLIPSOID) {
		// dy^2 rx^2 rz^2 <= left = rx^2 ry^2 rz^2 - dx^2 ry^2 rz^2 - dz^2 rx^2 ry^2 (each term at most 2^60 inside the footprint); the half height is
		// ISqrt(left / (rx^2 rz^2)): a float64 estimate corrected with the integer predicate, as ISqrt does
		const int64_t rx = s.b[0], ry = s.b[1], rz = s.b[2], dx = cx - s.a[0], dz = cz - s.a[2];
		if (dx >= -rx && dx <= rx && dz >= -rz && dz <= rz) {
			const int64_t xx = rx * rx, yy = ry * ry, zz = rz * rz, xz = xx * zz;
			const int64_t left = xz * yy - dx * dx * (yy * zz) - dz * dz * (xx * yy);
			if (left >= 0) {
				int64_t e = (int64_t)__builtin_sqrt((double)left / (double)xz);
				while (e > 0 && e * e * xz > left) { e--; }
				while ((e + 1) * (e + 1) * xz <= left) { e++; }
				l = (int64_t)s.a[1] - e;
				h = (int64_t)s.a[1] + e + 1;
			}
		}
	} else {
		// the capsule: the hull of its end spheres' intervals and of the part between the end planes (the set is convex; a voxel of an end sphere
		// on the far side of that end's plane satisfies the rule of the part it lies in, its distance to the segment being no larger)
		const int64_t r = s.pad_, dx = (int64_t)s.b[0] - s.a[0], dy = (int64_t)s.b[1] - s.a[1], dz = (int64_t)s.b[2] - s.a[2];
		const int64_t wx = cx - s.a[0], wz = cz - s.a[2];
		if (wx >= (dx < 0 ? dx : 0) - r && wx <= (dx > 0 ? dx : 0) + r && wz >= (dz < 0 ? dz : 0) - r && wz <= (dz > 0 ? dz : 0) + r) {
			const int64_t rr = r * r, ww = wx * wx + wz * wz, vv = (wx - dx) * (wx - dx) + (wz - dz) * (wz - dz);
			int64_t t1 = 1, t2 = 0; // offsets from a[1], inclusive
			if (ww <= rr) {
				const int64_t e = ISqrt(rr - ww);
				t1 = -e;
				t2 = e;
			}
			if (vv <= rr) {
				const int64_t e = ISqrt(rr - vv);
				if (t1 > t2) { t1 = dy - e; t2 = dy + e; }
				t1 = dy - e < t1 ? dy - e : t1;
				t2 = dy + e > t2 ? dy + e : t2;
			}
			const int64_t a2 = dx * dx + dz * dz;
			if (a2 > 0) { // (a vertical capsule, a point included: the end spheres' hull is all of it)
				const int64_t L = a2 + dy * dy, p0 = wx * dx + wz * dz;
				int64_t m1, m2;
				CapsuleMiddle(a2, p0 * dy, (ww - rr) * L - p0 * p0, p0, dy, L, (dy < 0 ? dy : 0) - r, (dy > 0 ? dy : 0) + r, &m1, &m2);
				if (m1 <= m2) {
					if (t1 > t2) { t1 = m1; t2 = m2; }
					t1 = m1 < t1 ? m1 : t1;
					t2 = m2 > t2 ? m2 : t2;
				}
			}
			if (t1 <= t2) {
				l = (int64_t)s.a[1] + t1;
				h = (int64_t)s.a[1] + t2 + 1;
			}
		}
	}
	*lo = l;
	*hi = h;
}

// StrokeSpanUnclipped clipped to [0, dimY): what a stroke covers of a column of the world.
CVX_HD inline void StrokeSpan(const cvx_brush_stroke &s, int64_t cx, int64_t cz, int64_t dimY, int64_t *lo, int64_t *hi)
{
	int64_t l, h;
	StrokeSpanUnclipped(s, cx, cz, &l, &h);
	*lo = l < 0 ? 0 : l;
	*hi = h > dimY ? dimY : h;
}

// ---- the strokes a strip of columns can meet ----------------------------------------------------------------------------------------------------

// The XZ box [x0, x1] x [z0, z1] (inclusive) of the columns first .. last of a rectangle whose columns are numbered i -> (rectX + i / sizeZ,
// rectZ + i % sizeZ), the blob's column order: a wave's 64 columns in the brush kernels.  A strip that wraps into the next row takes the box of
// both parts, the rectangle's whole width in z.
CVX_HD inline void StripBox(int first, int last, int rectX, int rectZ, int sizeZ, int64_t *x0, int64_t *x1, int64_t *z0, int64_t *z1)
{
	const int rowA = first / sizeZ, rowB = last / sizeZ;
	*x0 = (int64_t)rectX + rowA;
	*x1 = (int64_t)rectX + rowB;
	*z0 = (int64_t)rectZ + (rowA == rowB ? first - rowA * sizeZ : 0);
	*z1 = (int64_t)rectZ + (rowA == rowB ? last - rowB * sizeZ : sizeZ - 1);
}

// Conservative: false only if the stroke's footprint misses every column of the box, where its span (StrokeSpan) is empty
CVX_HD inline bool StrokeMeetsStrip(const cvx_brush_stroke &s, int64_t x0, int64_t x1, int64_t z0, int64_t z1)
{
	int64_t lo[3], hi[3];
	StrokeFootprint(s, lo, hi);
	return lo[0] <= x1 && hi[0] > x0 && lo[2] <= z1 && hi[2] > z0;
}

// The stroke list a column walks: all n strokes of the call, or those a cull kept (ascending indices into the call's list: the fold depends on order)
// Walk(k) is the access of the column walk's loop over the strokes.  REQUIREMENT ON THE CALLER: on the device every active lane of the wave must call
// Walk with the same k at the same time (ListedStrokes reads the entry through readfirstlane, i.e. from ONE lane, so that the stroke's fields come
// through scalar loads).  BrushColumnOver keeps it: its stroke loop restarts at 0 in every iteration of the outer loop and runs to n in every lane,
// with no per-lane exit.  A per-lane index (the last stroke that covered a voxel, say) goes through operator[] instead.
struct AllStrokes {
	const cvx_brush_stroke *strokes;
	CVX_HD const cvx_brush_stroke &operator[](int k) const { return strokes[k]; }
	CVX_HD const cvx_brush_stroke &Walk(int k) const { return strokes[k]; }
};

struct ListedStrokes {
	const cvx_brush_stroke *strokes;
	const uint16_t *list;
	CVX_HD const cvx_brush_stroke &operator[](int k) const { return strokes[list[k]]; }
	CVX_HD const cvx_brush_stroke &Walk(int k) const
	{
#if defined(__HIP_DEVICE_COMPILE__)
		return strokes[__builtin_amdgcn_readfirstlane((int)list[k])]; // (k is wave-uniform: the requirement above)
#else
		return strokes[list[k]];
#endif
	}
};

// ---- one column after the strokes -------------------------------------------------------------------------------------------------------------

struct BrushResult {
	uint32_t runCount;       // runs, air ones included (0: the column is empty)
	uint32_t colours;        // solid voxels
	uint32_t worldMin, worldMax;
	bool overLimit;          // a run count, run length or colour index the format cannot hold
};

// The column in a sub-world blob (the reference's layout): its elements are [guard][runs][guard][colours], none for an empty column ...
CVX_HD inline __attribute__((always_inline)) uint32_t BlobElements(const BrushResult &r) { return r.runCount ? r.runCount + 2u + r.colours : 0u; }
// ... and what a write kernel ends with, the column counted as r: for an empty column the zero header h and nothing else; otherwise, once the
// second walk has written the runs at e + 1 and the colours at e + r.runCount + 2 (behind the runs' second guard, a place known once the runs are
// counted), the two guards and the 12-byte header.  e = the pool + off.
// The test `r.runCount == 0u` stays in the kernels on purpose (`if (r.runCount == 0u) { BlobEmitEmpty(h); return; }`, h computed where it always
// was): with the test inside a helper, or the second walk passed in as a callable, the compiler allocates the write kernels' registers differently
// and their instruction lists change.  Keep the two helpers apart unless the kernels are meant to change.
CVX_HD inline __attribute__((always_inline)) void BlobEmitEmpty(uint32_t *h)
{
	h[0] = 0u;
	h[1] = 0u;
	h[2] = 0u;
}
CVX_HD inline __attribute__((always_inline)) void BlobEmitHeader(uint32_t *h, uint32_t *e, uint32_t off, const BrushResult &r)
{
	e[0] = 0u;
	e[r.runCount + 1u] = 0u;
	h[0] = off;
	h[1] = r.runCount | (r.worldMin << 16);
	h[2] = r.worldMax;
}

// Walks the column (cx, cz) top-down after `n` strokes.  Every voxel ends as the fold of the strokes that cover it over what the arena holds:
// FILL -> solid(argb), CARVE -> air, PAINT -> solid ? solid(argb) : air.  So within a y span where the same strokes cover the column and the
// arena's column does not change between solid and air, every voxel has the same fate: the walk goes span by span, the span ends at the
// next boundary of a stroke interval or an arena run below it.
// Out (may be null): runs[r] = colorsIndex | length << 16 (colorsIndex 0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top
// (colourSlots: the arena's colour array, 4-byte slots, read at the column's colorsBase + index << (colorShift - 2)).
// `strokes` is AllStrokes or ListedStrokes: strokes[k], k < n, in the order they apply.  A stroke a cull left out has an empty span in this
// column, so the walk over the culled list gives what the walk over the whole list gives.
template <class Strokes>
CVX_HD inline BrushResult BrushColumnOver(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const Strokes &strokes, int n,
                                          int64_t cx, int64_t cz, int dimY, uint32_t *outRuns, uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	const uint32_t solidRuns = col.Count();
	uint32_t k = 0;                      // the arena run at or below y
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0; // the run being emitted
	int64_t lowest = -1, highest = -1;   // solid voxels
	int64_t y = (int64_t)dimY - 1;
	while (y >= 0) {
		// the arena: solid run k or the air above it
		while (k < solidRuns && (int64_t)col.Run(k).bottom > y) { k++; }
		SolidRun run{ 0u, 0u, 0u };
		bool origSolid = false;
		int64_t bottom = 0;
		if (k < solidRuns) {
			run = col.Run(k);
			origSolid = (int64_t)run.top > y;
			bottom = origSolid ? (int64_t)run.bottom : (int64_t)run.top;
		}
		// the strokes: the last FILL / CARVE and the last FILL / PAINT that cover y, and where the span ends
		int lastFC = -1, lastFP = -1;
		// (Walk needs s to be the same in every active lane: this loop must keep running 0 .. n - 1 in every lane, whatever the lane's y -- no early
		// exit, no per-lane start; see ListedStrokes)
		for (int s = 0; s < n; s++) {
			int64_t lo, hi;
			const cvx_brush_stroke &stroke = strokes.Walk(s);
			StrokeSpan(stroke, cx, cz, dimY, &lo, &hi);
			if (lo >= hi) { continue; }
			if (lo <= y && y < hi) {
				if (stroke.op != CVX_BRUSH_PAINT) { lastFC = s; }
				if (stroke.op != CVX_BRUSH_CARVE) { lastFP = s; }
				bottom = lo > bottom ? lo : bottom;
			} else if (hi <= y) {
				bottom = hi > bottom ? hi : bottom;
			}
		}
		const bool solid = lastFC < 0 ? origSolid : strokes[lastFC].op == CVX_BRUSH_FILL;
		const bool painted = lastFP >= 0 && lastFP >= lastFC;
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
					outColours[res.colours + (uint32_t)(y - v)] = painted ? strokes[lastFP].argb
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

CVX_HD inline BrushResult BrushColumn(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const cvx_brush_stroke *strokes, int n,
                                      int64_t cx, int64_t cz, int dimY, uint32_t *outRuns, uint32_t *outColours)
{
	return BrushColumnOver(col, colourSlots, colorShift, AllStrokes{ strokes }, n, cx, cz, dimY, outRuns, outColours);
}

// ---- picking ----------------------------------------------------------------------------------------------------------------------------------

struct PickWorld {
	const uint32_t *records;    // LOD 0's records (uint4 each), row-major with 2^rowShift per row; one row + 4 records either side are readable
	const uint32_t *runs;       // run list, 2 words per entry
	const uint8_t *colours;     // colour array (bytes)
	int rowShift, colorShift;
	int dimX, dimY, dimZ;
	int repeat = 0;             // 1: the world repeats in X and Z (cvx_set_world_repeat): PickRayRepeat
};

struct PickResult {
	int32_t voxel[3];
	int32_t face;
	uint32_t argb;
	float t;
};

// The traversal rule, float64 throughout (one rule, so that a float64 model can say which rays it resolves unambiguously):
//   1. clip: per axis with d != 0 the slab [0, dim] gives t0 <= t1 (t = (plane - o) * (1 / d)); tEnter = max(0, t0's), tExit = min(maxT, t1's);
//      the axis whose t0 > 0 set tEnter is the entry face (ties: the lower axis); an axis with d == 0 and o outside [0, dim) misses.
//   2. start inside the box (tEnter == 0 through no face): the voxel floor(o) solid -> that voxel, face 6, t 0.
//   3. columns: the column of o + tEnter * d (clamped into the world); per step the ray's t interval in the column is [tc0, tc1], tc1 = the
//      nearer of the next x / z column planes and tExit.  Its voxels, in ray order: down (d.y < 0) ceil(ya) - 1 .. floor(yb), up floor(ya) ..
//      ceil(yb) - 1, level floor(o.y) (ya / yb: y at tc0 / tc1; clamped into [0, dimY)).  The first solid one of them is the hit: the first
//      voxel of the column -> the face the column was entered through, t = tc0; a later one (or any one in the column a ray starts in) -> its +Y
//      (down) or -Y (up) face, t = the plane's.
//   4. step to the nearer plane (x on a tie: the diagonal step takes two steps, the second one of length 0); stop at tExit.
// A repeating world (PickRayRepeat): step 1 clips to the Y slab only, the columns of steps 3 and 4 are looked up wrapped into the tile (floor-mod) and
// the walk ends at tExit only; maxT must be at most 2^20 (else a miss), and the origin's |x|, |z| below 2^40.  The reported voxel is the wrapped one,
// t the parameter along the ray itself.
CVX_HD inline PickResult PickMiss(float maxT) { return PickResult{ { -1, -1, -1 }, -1, 0u, maxT }; }

struct alignas(16) Record { uint32_t x, y, z, w; };

CVX_HD inline Record PickRecord(const PickWorld &W, int64_t at) { return *reinterpret_cast<const Record *>(W.records + 4 * at); }

CVX_HD inline int64_t ClampY(double v, int64_t lastY) { return v < 0.0 ? 0 : (v > (double)lastY ? lastY : (int64_t)v); }
CVX_HD inline bool Finite(double v) { return v > -1e30 && v < 1e30; }

CVX_HD inline uint32_t PickColour(const PickWorld &W, const ArenaColumn &col, const SolidRun &run, uint32_t v)
{
	const uint32_t index = run.colorsIndex + (run.top - 1u - v);
	const uint64_t byte = (uint64_t)col.ColorsBase() * 4u + ((uint64_t)index << W.colorShift);
	const uint8_t *p = W.colours + byte;
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

CVX_HD inline PickResult PickRay(const PickWorld &W, const float originF[3], const float directionF[3], float maxTF)
{
	const double o[3] = { originF[0], originF[1], originF[2] }, d[3] = { directionF[0], directionF[1], directionF[2] };
	const double dim[3] = { (double)W.dimX, (double)W.dimY, (double)W.dimZ };
	double inv[3];
	double tEnter = 0.0, tExit = (double)maxTF;
	int enterAxis = -1;
	for (int a = 0; a < 3; a++) {
		if (!Finite(o[a]) || !Finite(d[a])) { return PickMiss(maxTF); }
		if (d[a] == 0.0) {
			inv[a] = 0.0;
			if (!(o[a] >= 0.0 && o[a] < dim[a])) { return PickMiss(maxTF); }
			continue;
		}
		inv[a] = 1.0 / d[a];
		double t0 = (0.0 - o[a]) * inv[a], t1 = (dim[a] - o[a]) * inv[a];
		if (t0 > t1) { const double s = t0; t0 = t1; t1 = s; }
		if (t0 > tEnter) { tEnter = t0; enterAxis = a; }
		if (t1 < tExit) { tExit = t1; }
	}
	if (!(tEnter <= tExit)) { return PickMiss(maxTF); }
	const int64_t lastY = W.dimY - 1;
	const int64_t cx0 = ClampY(__builtin_floor(o[0] + tEnter * d[0]), W.dimX - 1), cz0 = ClampY(__builtin_floor(o[2] + tEnter * d[2]), W.dimZ - 1);
	int64_t cx = cx0, cz = cz0;
	const int stepX = d[0] > 0.0 ? 1 : -1, stepZ = d[2] > 0.0 ? 1 : -1;
	const int64_t recordStepX = (int64_t)stepX << W.rowShift, recordStepZ = stepZ;
	int face = enterAxis < 0 ? 6 : 2 * enterAxis + (d[enterAxis] > 0.0 ? 0 : 1);
	int64_t at = (cx << W.rowShift) + cz;
	Record rec = PickRecord(W, at);
	if (enterAxis < 0) { // 2. the origin's own voxel
		const ArenaColumn col{ rec.x, rec.y, rec.z, rec.w, W.runs };
		const uint32_t v = (uint32_t)ClampY(__builtin_floor(o[1]), lastY);
		for (uint32_t k = 0; k < col.Count(); k++) {
			const SolidRun run = col.Run(k);
			if (v >= run.bottom && v < run.top) {
				return PickResult{ { (int32_t)cx, (int32_t)v, (int32_t)cz }, 6, PickColour(W, col, run, v), 0.0f };
			}
		}
	}
	double tc0 = tEnter;
	const bool down = d[1] < 0.0, level = d[1] == 0.0;
	for (int64_t guard = (int64_t)W.dimX + W.dimZ + 2; guard > 0; guard--) {
		const double tx = d[0] != 0.0 ? ((double)(cx + (stepX > 0 ? 1 : 0)) - o[0]) * inv[0] : __builtin_inf();
		const double tz = d[2] != 0.0 ? ((double)(cz + (stepZ > 0 ? 1 : 0)) - o[2]) * inv[2] : __builtin_inf();
		const bool stepAlongX = tx <= tz;
		const double tNext = stepAlongX ? tx : tz;
		const double tc1 = tNext < tExit ? tNext : tExit;
		const int64_t nextAt = at + (stepAlongX ? recordStepX : recordStepZ);
		const Record next = PickRecord(W, nextAt); // one step ahead (the tables have a guard row on both sides)
		const ArenaColumn col{ rec.x, rec.y, rec.z, rec.w, W.runs };
		if (col.x != 0u) {
			const double ya = o[1] + tc0 * d[1], yb = o[1] + tc1 * d[1];
			int64_t vA, vB;
			if (level) {
				vA = vB = ClampY(__builtin_floor(o[1]), lastY);
			} else if (down) {
				vA = ClampY(__builtin_ceil(ya) - 1.0, lastY);
				vB = ClampY(__builtin_floor(yb), lastY);
			} else {
				vA = ClampY(__builtin_floor(ya), lastY);
				vB = ClampY(__builtin_ceil(yb) - 1.0, lastY);
			}
			const int64_t lo = vA < vB ? vA : vB, hi = vA < vB ? vB : vA;
			const bool empty = level ? false : (down ? vA < vB : vA > vB);
			if (!empty && hi >= (int64_t)col.WorldMin() && lo < (int64_t)col.WorldMax()) {
				int64_t best = -1;
				SolidRun bestRun{ 0u, 0u, 0u };
				for (uint32_t k = 0; k < col.Count(); k++) {
					const SolidRun run = col.Run(k);
					if ((int64_t)run.bottom > hi || (int64_t)run.top - 1 < lo) { continue; }
					const int64_t v = down || level ? ((int64_t)run.top - 1 < vA ? (int64_t)run.top - 1 : vA) : ((int64_t)run.bottom > vA ? (int64_t)run.bottom : vA);
					if (best < 0 || (down || level ? v > best : v < best)) { best = v; bestRun = run; }
				}
				if (best >= 0) {
					PickResult hit;
					hit.voxel[0] = (int32_t)cx;
					hit.voxel[1] = (int32_t)best;
					hit.voxel[2] = (int32_t)cz;
					hit.argb = PickColour(W, col, bestRun, (uint32_t)best);
					if (best == vA && face != 6) { // (face 6: the first column of a ray that starts in it; its own voxel is air)
						hit.face = face;
						hit.t = (float)tc0;
					} else {
						hit.face = down ? 3 : 2;
						hit.t = (float)(((double)(down ? best + 1 : best) - o[1]) * inv[1]);
					}
					return hit;
				}
			}
		}
		if (tNext >= tExit) { break; }
		if (stepAlongX) { cx += stepX; face = stepX > 0 ? 0 : 1; } else { cz += stepZ; face = stepZ > 0 ? 4 : 5; }
		if (cx < 0 || cx >= W.dimX || cz < 0 || cz >= W.dimZ) { break; }
		tc0 = tNext;
		at = nextAt;
		rec = next;
	}
	return PickMiss(maxTF);
}


// PickRay in a repeating world (W.repeat): the same rule with the changes listed above the miss helper; kept apart from PickRay so that the
// bounded traversal stays exactly what it was.
CVX_HD inline PickResult PickRayRepeat(const PickWorld &W, const float originF[3], const float directionF[3], float maxTF)
{
	const double o[3] = { originF[0], originF[1], originF[2] }, d[3] = { directionF[0], directionF[1], directionF[2] };
	const double dim[3] = { (double)W.dimX, (double)W.dimY, (double)W.dimZ };
	double inv[3];
	double tEnter = 0.0, tExit = (double)maxTF;
	int enterAxis = -1;
	const bool repeat = W.repeat != 0;
	if (repeat && !(maxTF <= 1048576.0f && __builtin_fabs(o[0]) < 0x1p40 && __builtin_fabs(o[2]) < 0x1p40)) { return PickMiss(maxTF); }
	for (int a = 0; a < 3; a++) {
		if (!Finite(o[a]) || !Finite(d[a])) { return PickMiss(maxTF); }
		if (repeat && a != 1) { // no X / Z slab in a repeating world
			inv[a] = d[a] == 0.0 ? 0.0 : 1.0 / d[a];
			continue;
		}
		if (d[a] == 0.0) {
			inv[a] = 0.0;
			if (!(o[a] >= 0.0 && o[a] < dim[a])) { return PickMiss(maxTF); }
			continue;
		}
		inv[a] = 1.0 / d[a];
		double t0 = (0.0 - o[a]) * inv[a], t1 = (dim[a] - o[a]) * inv[a];
		if (t0 > t1) { const double s = t0; t0 = t1; t1 = s; }
		if (t0 > tEnter) { tEnter = t0; enterAxis = a; }
		if (t1 < tExit) { tExit = t1; }
	}
	if (!(tEnter <= tExit)) { return PickMiss(maxTF); }
	const int64_t lastY = W.dimY - 1;
	const int64_t maskX = W.dimX - 1, maskZ = W.dimZ - 1; // (power-of-two dimensions)
	// (a repeating world: cx / cz are the unwrapped columns along the ray -- the plane distances below use them --, records and voxels their wrapped form)
	const int64_t cx0 = repeat ? (int64_t)__builtin_floor(o[0] + tEnter * d[0]) : ClampY(__builtin_floor(o[0] + tEnter * d[0]), W.dimX - 1);
	const int64_t cz0 = repeat ? (int64_t)__builtin_floor(o[2] + tEnter * d[2]) : ClampY(__builtin_floor(o[2] + tEnter * d[2]), W.dimZ - 1);
	int64_t cx = cx0, cz = cz0;
	const int stepX = d[0] > 0.0 ? 1 : -1, stepZ = d[2] > 0.0 ? 1 : -1;
	const int64_t recordStepX = (int64_t)stepX << W.rowShift, recordStepZ = stepZ;
	int face = enterAxis < 0 ? 6 : 2 * enterAxis + (d[enterAxis] > 0.0 ? 0 : 1);
	int64_t at = ((cx & maskX) << W.rowShift) + (cz & maskZ);
	Record rec = PickRecord(W, at);
	if (enterAxis < 0) { // 2. the origin's own voxel
		const ArenaColumn col{ rec.x, rec.y, rec.z, rec.w, W.runs };
		const uint32_t v = (uint32_t)ClampY(__builtin_floor(o[1]), lastY);
		for (uint32_t k = 0; k < col.Count(); k++) {
			const SolidRun run = col.Run(k);
			if (v >= run.bottom && v < run.top) {
				return PickResult{ { (int32_t)(cx & maskX), (int32_t)v, (int32_t)(cz & maskZ) }, 6, PickColour(W, col, run, v), 0.0f };
			}
		}
	}
	double tc0 = tEnter;
	const bool down = d[1] < 0.0, level = d[1] == 0.0;
	// (a repeating world: the columns up to tExit <= 2^20, at most 2^24 of them)
	const double repeatSteps = (__builtin_fabs(d[0]) + __builtin_fabs(d[2])) * tExit + 4.0;
	for (int64_t guard = repeat ? (int64_t)(repeatSteps < 16777216.0 ? repeatSteps : 16777216.0) : (int64_t)W.dimX + W.dimZ + 2; guard > 0; guard--) {
		const double tx = d[0] != 0.0 ? ((double)(cx + (stepX > 0 ? 1 : 0)) - o[0]) * inv[0] : __builtin_inf();
		const double tz = d[2] != 0.0 ? ((double)(cz + (stepZ > 0 ? 1 : 0)) - o[2]) * inv[2] : __builtin_inf();
		const bool stepAlongX = tx <= tz;
		const double tNext = stepAlongX ? tx : tz;
		const double tc1 = tNext < tExit ? tNext : tExit;
		const int64_t nextAt = repeat ? (stepAlongX ? (((cx + stepX) & maskX) << W.rowShift) + (cz & maskZ) : ((cx & maskX) << W.rowShift) + ((cz + stepZ) & maskZ))
		                              : at + (stepAlongX ? recordStepX : recordStepZ);
		const Record next = PickRecord(W, nextAt); // one step ahead (the tables have a guard row on both sides)
		const ArenaColumn col{ rec.x, rec.y, rec.z, rec.w, W.runs };
		if (col.x != 0u) {
			const double ya = o[1] + tc0 * d[1], yb = o[1] + tc1 * d[1];
			int64_t vA, vB;
			if (level) {
				vA = vB = ClampY(__builtin_floor(o[1]), lastY);
			} else if (down) {
				vA = ClampY(__builtin_ceil(ya) - 1.0, lastY);
				vB = ClampY(__builtin_floor(yb), lastY);
			} else {
				vA = ClampY(__builtin_floor(ya), lastY);
				vB = ClampY(__builtin_ceil(yb) - 1.0, lastY);
			}
			const int64_t lo = vA < vB ? vA : vB, hi = vA < vB ? vB : vA;
			const bool empty = level ? false : (down ? vA < vB : vA > vB);
			if (!empty && hi >= (int64_t)col.WorldMin() && lo < (int64_t)col.WorldMax()) {
				int64_t best = -1;
				SolidRun bestRun{ 0u, 0u, 0u };
				for (uint32_t k = 0; k < col.Count(); k++) {
					const SolidRun run = col.Run(k);
					if ((int64_t)run.bottom > hi || (int64_t)run.top - 1 < lo) { continue; }
					const int64_t v = down || level ? ((int64_t)run.top - 1 < vA ? (int64_t)run.top - 1 : vA) : ((int64_t)run.bottom > vA ? (int64_t)run.bottom : vA);
					if (best < 0 || (down || level ? v > best : v < best)) { best = v; bestRun = run; }
				}
				if (best >= 0) {
					PickResult hit;
					hit.voxel[0] = (int32_t)(cx & maskX);
					hit.voxel[1] = (int32_t)best;
					hit.voxel[2] = (int32_t)(cz & maskZ);
					hit.argb = PickColour(W, col, bestRun, (uint32_t)best);
					if (best == vA && face != 6) { // (face 6: the first column of a ray that starts in it; its own voxel is air)
						hit.face = face;
						hit.t = (float)tc0;
					} else {
						hit.face = down ? 3 : 2;
						hit.t = (float)(((double)(down ? best + 1 : best) - o[1]) * inv[1]);
					}
					return hit;
				}
			}
		}
		if (tNext >= tExit) { break; }
		if (stepAlongX) { cx += stepX; face = stepX > 0 ? 0 : 1; } else { cz += stepZ; face = stepZ > 0 ? 4 : 5; }
		if (!repeat && (cx < 0 || cx >= W.dimX || cz < 0 || cz >= W.dimZ)) { break; }
		tc0 = tNext;
		at = nextAt;
		rec = next;
	}
	return PickMiss(maxTF);
}

} // namespace cvxb
