// cvx_model_draw.h -- the rules of cvxv_models_draw (cvx_model_draw.hip): placed voxel models drawn into a view, a pixel at a time.
//
// Written once for the device AND the host (tests/model_draw_rules.cpp compiles it with g++ and runs it against the numpy model of
// tests/modeldrawmodel.py):
//   ModelDrawRayOf       step 1 of the rule (include/cpuvox_gpu_model_draw.h): the ray of pixel (x, y), float64, every operation rounded once
//   ModelDrawDepthLimit  the depth test's share of step 1
//   ModelDrawBody        one instance against a pixel's ray: cvxq_model_pick's pair rule (cvx_model_pick.h) into the pixel's key.  With `skip` it
//                        leaves out the walk of an instance that cannot beat the key: the box is entered later than the key's t, by more
//                        than the float ulp the start state's rounding could cost (pick_walk_kernel's guard).  Whether the ray crosses the box
//                        -- the job -- is answered either way.
//   ModelDrawOccluded    step 3: cvx_world_pick's rule up to the body's t
//   ModelDrawRect        the cull: the rectangle of pixels whose rays can reach an instance's box.  The kernel and the host form of its tile
//                        walk (tests/model_draw_rules.cpp) list an instance for a tile iff the rectangle meets it; the un-culled rule never
//                        asks.  The two must agree in every byte.
//   the host side        ModelDrawInverse, ModelDrawValidate, ModelDrawViewFromCamera, ModelDrawRays
// All of the ray is float64; the product is built with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_model_draw.h"
#include "cvx_model_pick.h"

namespace cvxb {

constexpr int kModelDrawTile = 8; // a wave's tile: 8 x 8 pixels, lane l = pixel (l & 7, l >> 3)

// Step 1: the ray of pixel (x, y); false is a miss (the ray is then the one cvxv_view_rays writes for it: direction 0, maxT -1).
CVX_HD CVX_PICK_INLINE bool ModelDrawRayOf(const cvxv_view &V, int x, int y, cvx_pick_ray *ray)
{
	const double fx = (double)x, fy = (double)y;
	const double a0 = (V.dir0[0] + fx * V.dirX[0]) + fy * V.dirY[0];
	const double a1 = (V.dir0[1] + fx * V.dirX[1]) + fy * V.dirY[1];
	const double a2 = (V.dir0[2] + fx * V.dirX[2]) + fy * V.dirY[2];
	const double len = __builtin_sqrt((a0 * a0 + a1 * a1) + a2 * a2);
	const bool good = len > 0.0 && len < __builtin_inf();
	ray->origin[0] = V.origin[0];
	ray->origin[1] = V.origin[1];
	ray->origin[2] = V.origin[2];
	ray->direction[0] = good ? (float)(a0 / len) : 0.0f;
	ray->direction[1] = good ? (float)(a1 / len) : 0.0f;
	ray->direction[2] = good ? (float)(a2 / len) : 0.0f;
	ray->maxT = good ? V.maxT : -1.0f;
	ray->pad_ = 0.0f;
	return good;
}

// CVXV_DRAW_DEPTH_TEST: the ray ends at the pixel's depth where that is smaller; false (a NaN or negative depth) is a miss.
CVX_HD CVX_PICK_INLINE bool ModelDrawDepthLimit(float depth, float *maxT)
{
	if (!(depth >= 0.0f)) { return false; }
	if (depth < *maxT) { *maxT = depth; }
	return true;
}

// Instance k (its body B) against the pixel's ray: true when the ray crosses the box (a job).  *key / *argb: the pixel's nearest hit so far.
CVX_HD CVX_PICK_INLINE bool ModelDrawBody(const ModelPickBody &B, int k, const cvx_pick_ray &ray, bool skip, uint64_t *key, uint32_t *argb)
{
	ModelPickRay R;
	ModelPickState S;
	int64_t s[3];
	if (!ModelPickClip(ray.origin, ray.direction, ray.maxT, B.lo, B.hi, &R, &S)) { return false; }
	if (skip && (uint64_t)ModelPickFloatBits(ModelPickReported(R.tEnter)) > (uint64_t)(*key >> 32) + 1u) { return true; } // (no key: never)
	if (ModelPickSequential(R, B, &S, s)) {
		const uint64_t mine = ModelPickKey(ModelPickReported(S.t), k);
		if (mine < *key) {
			*key = mine;
			*argb = PairModelColour(B.M, s);
		}
	}
	return true;
}

CVX_HD inline float ModelDrawKeyT(uint64_t key)
{
	union {
		uint32_t u;
		float f;
	} bits;
	bits.u = (uint32_t)(key >> 32);
	return bits.f;
}

// Step 3: whether the world hides what the ray found at t.
CVX_HD inline bool ModelDrawOccluded(const PickWorld &W, const cvx_pick_ray &ray, float t)
{
	const PickResult r = W.repeat ? PickRayRepeat(W, ray.origin, ray.direction, t) : PickRay(W, ray.origin, ray.direction, t);
	return r.face >= 0;
}

// ---- the cull ----------------------------------------------------------------------------------------------------------------------------------

// Pixels x0 .. x1, y0 .. y1, both ends included; x0 > x1: none.
struct alignas(16) ModelDrawRect {
	int32_t x0, y0, x1, y1;
};

// What the cull reads of the view, made by ModelDrawValidate: inv = [dirX dirY dir0]^-1 (row-major), so that a point P - origin = s * a(x, y)
// with s > 0 has (x, y, 1) * w = inv * (P - origin), w > 0; `grow`: the pixels a rectangle is widened by on every side.
struct ModelDrawCull {
	double inv[9];
	int32_t grow, pad_;
};

// The rectangle of the box [lo, hi): the eight corners through inv, floor / ceil, widened by C.grow pixels and cut to the screen.  A corner at or
// behind the eye plane (w not clearly positive) takes the whole screen.  Conservative: the box is convex and in front of the eye plane, so a ray
// that reaches it goes through a pixel inside the corners' bounds; the widening covers the float rounding of the direction and of this
// arithmetic (ModelDrawValidate sizes it).
CVX_HD inline ModelDrawRect ModelDrawRectOf(const ModelDrawCull &C, const float origin[3], const int32_t lo[3], const int32_t hi[3], int width, int height)
{
	const double inf = __builtin_inf();
	double minX = inf, maxX = -inf, minY = inf, maxY = -inf;
	bool whole = false;
	for (int c = 0; c < 8; c++) {
		const double p0 = (double)((c & 1) ? hi[0] : lo[0]) - (double)origin[0];
		const double p1 = (double)((c & 2) ? hi[1] : lo[1]) - (double)origin[1];
		const double p2 = (double)((c & 4) ? hi[2] : lo[2]) - (double)origin[2];
		const double u = (C.inv[0] * p0 + C.inv[1] * p1) + C.inv[2] * p2;
		const double v = (C.inv[3] * p0 + C.inv[4] * p1) + C.inv[5] * p2;
		const double w = (C.inv[6] * p0 + C.inv[7] * p1) + C.inv[8] * p2;
		const double size = (__builtin_fabs(C.inv[6] * p0) + __builtin_fabs(C.inv[7] * p1)) + __builtin_fabs(C.inv[8] * p2);
		if (!(w > 1e-6 * size)) { whole = true; } // (NaN too)
		const double x = u / w, y = v / w;
		if (!(x == x) || !(y == y)) { whole = true; }
		minX = x < minX ? x : minX;
		maxX = x > maxX ? x : maxX;
		minY = y < minY ? y : minY;
		maxY = y > maxY ? y : maxY;
	}
	if (whole) { return ModelDrawRect{ 0, 0, width - 1, height - 1 }; }
	const double g = (double)C.grow;
	const double fx0 = __builtin_floor(minX) - g, fx1 = __builtin_ceil(maxX) + g, fy0 = __builtin_floor(minY) - g, fy1 = __builtin_ceil(maxY) + g;
	if (fx0 > (double)(width - 1) || fx1 < 0.0 || fy0 > (double)(height - 1) || fy1 < 0.0) { return ModelDrawRect{ 1, 1, 0, 0 }; }
	ModelDrawRect r;
	r.x0 = fx0 < 0.0 ? 0 : (int32_t)fx0;
	r.y0 = fy0 < 0.0 ? 0 : (int32_t)fy0;
	r.x1 = fx1 > (double)(width - 1) ? width - 1 : (int32_t)fx1;
	r.y1 = fy1 > (double)(height - 1) ? height - 1 : (int32_t)fy1;
	return r;
}

// Whether the rectangle meets the tile whose first pixel is (tx, ty).
CVX_HD inline bool ModelDrawRectMeetsTile(const ModelDrawRect &r, int tx, int ty)
{
	return r.x0 <= r.x1 && r.x0 < tx + kModelDrawTile && r.x1 >= tx && r.y0 < ty + kModelDrawTile && r.y1 >= ty;
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)

inline double ModelDrawNorm(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// inv = [dirX dirY dir0]^-1 and the widening; false: the matrix is singular (or not finite).
inline bool ModelDrawInverse(const cvxv_view &V, ModelDrawCull *C)
{
	const double *x = V.dirX, *y = V.dirY, *z = V.dir0;
	const double yz[3] = { y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0] };
	const double zx[3] = { z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0] };
	const double xy[3] = { x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0] };
	const double det = (x[0] * yz[0] + x[1] * yz[1]) + x[2] * yz[2];
	const double scale = ModelDrawNorm(x) * ModelDrawNorm(y) * ModelDrawNorm(z);
	if (!(fabs(det) > 1e-9 * scale) || !(scale < INFINITY)) { return false; }
	for (int c = 0; c < 3; c++) {
		C->inv[c] = yz[c] / det;
		C->inv[3 + c] = zx[c] / det;
		C->inv[6 + c] = xy[c] / det;
	}
	// The float rounding of a direction turns the ray by at most 2^-23 of its length; through inv that moves its pixel by `slack`.  A rectangle
	// is rounded outward and widened by a pixel already, which covers half a pixel of it and the rounding of the cull's own arithmetic.
	double longest = 0.0;
	for (int corner = 0; corner < 4; corner++) {
		const double fx = (corner & 1) ? (double)(V.width - 1) : 0.0, fy = (corner & 2) ? (double)(V.height - 1) : 0.0;
		const double a[3] = { z[0] + fx * x[0] + fy * y[0], z[1] + fx * x[1] + fy * y[1], z[2] + fx * x[2] + fy * y[2] };
		longest = fmax(longest, ModelDrawNorm(a));
	}
	const double r0 = ModelDrawNorm(C->inv), r1 = ModelDrawNorm(C->inv + 3), r2 = ModelDrawNorm(C->inv + 6);
	const double slack = 2.4e-7 * longest * fmax(r0 + (double)V.width * r2, r1 + (double)V.height * r2);
	if (!(slack < 1e9)) { return false; }
	C->grow = slack <= 0.5 ? 1 : 1 + (int32_t)ceil(slack);
	C->pad_ = 0;
	return true;
}

// The argument checks of cvxv_models_draw[_device]: ContactsValidate's of the models and the instances, then the view, the flags and the outputs.
inline bool ModelDrawValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvxv_view *view, uint32_t flags,
                              const void *image, const void *depth, const void *ids, ModelDrawCull *cull, char *message, size_t bytes)
{
	if (!ContactsValidate(models, modelCount, instances, instanceCount, 0, message /* (its `results`: not ours) */, nullptr, 0, message, bytes)) { return false; }
	if (!view) {
		snprintf(message, bytes, "view is NULL");
		return false;
	}
	if (view->width < 1 || view->width > CVXV_MAX_SIZE || view->height < 1 || view->height > CVXV_MAX_SIZE) {
		snprintf(message, bytes, "view %d x %d outside 1 .. %d", view->width, view->height, CVXV_MAX_SIZE);
		return false;
	}
	if (!(view->maxT >= 0.0f)) {
		snprintf(message, bytes, "view maxT %g is negative or NaN", (double)view->maxT);
		return false;
	}
	for (int c = 0; c < 3; c++) {
		if (!Finite((double)view->origin[c]) || !Finite(view->dir0[c]) || !Finite(view->dirX[c]) || !Finite(view->dirY[c])) {
			snprintf(message, bytes, "view origin, dir0, dirX or dirY is not finite on axis %d", c);
			return false;
		}
	}
	if (!ModelDrawInverse(*view, cull)) {
		snprintf(message, bytes, "view: the matrix [dirX dirY dir0] is singular");
		return false;
	}
	if (flags & ~(uint32_t)(CVXV_DRAW_WORLD | CVXV_DRAW_DEPTH_TEST)) {
		snprintf(message, bytes, "flags 0x%x has unknown bits", flags);
		return false;
	}
	if (!image && !depth && !ids) {
		snprintf(message, bytes, "image, depth and ids are all NULL");
		return false;
	}
	if ((flags & CVXV_DRAW_DEPTH_TEST) && !depth) {
		snprintf(message, bytes, "CVXV_DRAW_DEPTH_TEST without depth");
		return false;
	}
	return true;
}

// out = m^-1 of a 4 x 4 row-major matrix (Gauss-Jordan, partial pivoting); false: singular.
inline bool ModelDrawInverse4(const double m[16], double out[16])
{
	double a[4][8];
	for (int r = 0; r < 4; r++) {
		for (int c = 0; c < 4; c++) {
			a[r][c] = m[4 * r + c];
			a[r][4 + c] = r == c ? 1.0 : 0.0;
		}
	}
	for (int col = 0; col < 4; col++) {
		int pivot = col;
		for (int r = col + 1; r < 4; r++) { if (fabs(a[r][col]) > fabs(a[pivot][col])) { pivot = r; } }
		if (!(fabs(a[pivot][col]) > 0.0) || !(fabs(a[pivot][col]) < INFINITY)) { return false; }
		for (int c = 0; c < 8; c++) {
			const double s = a[col][c];
			a[col][c] = a[pivot][c];
			a[pivot][c] = s;
		}
		const double d = a[col][col];
		for (int c = 0; c < 8; c++) { a[col][c] /= d; }
		for (int r = 0; r < 4; r++) {
			if (r == col) { continue; }
			const double f = a[r][col];
			for (int c = 0; c < 8; c++) { a[r][c] -= f * a[col][c]; }
		}
	}
	for (int r = 0; r < 4; r++) { for (int c = 0; c < 4; c++) { out[4 * r + c] = a[r][4 + c]; } }
	return true;
}

// cvxv_view_from_camera: 0, or -1.
inline int ModelDrawViewFromCamera(const cvx_camera_data *camera, int width, int height, float maxT, cvxv_view *out)
{
	if (!camera || !out || width < 1 || width > CVXV_MAX_SIZE || height < 1 || height > CVXV_MAX_SIZE) { return -1; }
	double m[16], inv[16]; // row-major: m[4 r + c] = the column-major storage's [4 c + r]
	for (int r = 0; r < 4; r++) { for (int c = 0; c < 4; c++) { m[4 * r + c] = (double)camera->WorldToScreenMatrix[4 * c + r]; } }
	if (!ModelDrawInverse4(m, inv)) { return -1; }
	const double pos[3] = { (double)camera->PositionXZ[0], (double)camera->PositionY, (double)camera->PositionXZ[1] };
	// a point in front of the camera fixes the depth: row 3 of the matrix is the view depth of a point
	const double ahead[4] = { pos[0] + m[12], pos[1] + m[13], pos[2] + m[14], 1.0 };
	double screen[4];
	for (int r = 0; r < 4; r++) { screen[r] = ((m[4 * r] * ahead[0] + m[4 * r + 1] * ahead[1]) + m[4 * r + 2] * ahead[2]) + m[4 * r + 3] * ahead[3]; }
	const double depth = screen[2] / screen[3];
	double d[3][3];
	const double at[3][2] = { { 0.5, 0.5 }, { 1.5, 0.5 }, { 0.5, 1.5 } };
	for (int k = 0; k < 3; k++) {
		double q[4];
		for (int r = 0; r < 4; r++) { q[r] = ((inv[4 * r] * at[k][0] + inv[4 * r + 1] * at[k][1]) + inv[4 * r + 2] * depth) + inv[4 * r + 3]; }
		for (int c = 0; c < 3; c++) { d[k][c] = q[c] / q[3] - pos[c]; }
	}
	for (int c = 0; c < 3; c++) {
		out->origin[c] = (float)pos[c];
		out->dir0[c] = d[0][c];
		out->dirX[c] = d[1][c] - d[0][c];
		out->dirY[c] = d[2][c] - d[0][c];
		if (!(fabs(d[0][c]) < INFINITY) || !(fabs(d[1][c]) < INFINITY) || !(fabs(d[2][c]) < INFINITY)) { return -1; }
	}
	out->maxT = maxT;
	out->width = width;
	out->height = height;
	return 0;
}

// cvxv_view_rays: 0, or -1.
inline int ModelDrawRays(const cvxv_view *view, int x0, int y0, int w, int h, cvx_pick_ray *rays)
{
	if (!view || !rays || view->width < 1 || view->width > CVXV_MAX_SIZE || view->height < 1 || view->height > CVXV_MAX_SIZE) { return -1; }
	if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || w > view->width - x0 || h > view->height - y0) { return -1; }
	for (int y = 0; y < h; y++) {
		for (int x = 0; x < w; x++) { ModelDrawRayOf(*view, x0 + x, y0 + y, rays + (size_t)y * (size_t)w + (size_t)x); }
	}
	return 0;
}

} // namespace cvxb
