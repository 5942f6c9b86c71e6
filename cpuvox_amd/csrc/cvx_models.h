// cvx_models.h -- the rules of cvx_world_place_models / cvx_world_read_model (cvx_models.hip): voxel models at any orientation and scale into
// and out of the device-resident world.
//
// Written once for the device AND the host (tests/test_world_models_cpu.py compiles it with g++ through tests/models_rules.cpp and compares it
// with the numpy model of tests/modelsmodel.py):
//   ModelMapApply   the image of a voxel under a cvx_model_map: int64 fixed point, the map applied to the voxel's centre, then floored
//   ModelsFinal     what voxel y of a column is after the call: the listed instances in order over what the arena holds
//   ModelsColumn    a column after the call, emitted as DenseColumn / BrushColumn emit it (the builder's encoding).  This scalar walk, a voxel
//                   at a time, is the specification: the wave-wide kernels of cvx_models.hip evaluate ModelsFinal per lane, step by step with
//                   the dense write's step algebra (cvx_dense.h), and must give the same bytes.
//   ModelsLaneVoxel, ModelCullBox  ModelsFinal as a lane of the wave evaluates it; what the cull reads of an instance, and its test
//   ModelReadVoxel  what element s of cvx_world_read_model's output holds
//   the host side   ModelsValidate / ModelReadValidate (the argument checks) and ModelInstanceFromMatrix (cvx_model_instance_from_matrix)
// Every read is from the arena as it is before the call: nothing writes it before cvxi::EditFromDevice takes the new columns.  No float on the
// device: a voxel is decided by int64 alone.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_models.h"
#include "cvx_dense.h"

namespace cvxb {

constexpr int32_t kModelMapMaxM = 1 << 24;
constexpr int64_t kModelMapMaxT = (int64_t)1 << 46;

// The part of q_i (include/cpuvox_gpu_models.h) that a column (v0, v2) fixes: m[i][0] * (2 v0 + 1) + m[i][2] * (2 v2 + 1) + 2 t[i] ...
CVX_HD inline int64_t ModelMapColumnPart(const cvx_model_map &M, int i, int64_t v0, int64_t v2)
{
	return (int64_t)M.m[i][0] * (2 * v0 + 1) + (int64_t)M.m[i][2] * (2 * v2 + 1) + 2 * M.t[i];
}

// ... and the image's coordinate i once v1 is known: int64 addition is exact below 2^63, so the split changes nothing.
CVX_HD inline int64_t ModelMapFinish(int64_t columnPart, int32_t m1, int64_t v1) { return (columnPart + (int64_t)m1 * (2 * v1 + 1)) >> 17; }

CVX_HD inline void ModelMapApply(const cvx_model_map &M, int64_t v0, int64_t v1, int64_t v2, int64_t out[3])
{
	for (int i = 0; i < 3; i++) { out[i] = ModelMapFinish(ModelMapColumnPart(M, i, v0, v2), M.m[i][1], v1); }
}

// An instance's box on axis a clipped to [0, dim): false when nothing is left.
CVX_HD inline bool ModelBoxClip(const cvx_model_instance &I, int a, int64_t dim, int64_t *lo, int64_t *hi)
{
	*lo = I.boxMin[a] < 0 ? 0 : (int64_t)I.boxMin[a];
	*hi = (int64_t)I.boxMax[a] > dim ? dim : (int64_t)I.boxMax[a];
	return *lo < *hi;
}

// The instance applied to a voxel whose model voxel is s (inside [0, size) or not).  `v` is what the earlier instances left; it is looked up in
// the arena only when something needs it (*known: v holds the voxel; else it is still the arena's, not read yet).
CVX_HD inline void ModelApply(const cvx_model &model, int op, const int64_t s[3], const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, int64_t y,
                              Voxel *v, bool *known)
{
	if (s[0] < 0 || s[0] >= model.size[0] || s[1] < 0 || s[1] >= model.size[1] || s[2] < 0 || s[2] >= model.size[2]) { return; }
	const int64_t at = (s[0] * model.size[2] + s[2]) * model.size[1] + s[1];
	const uint32_t c = model.argb ? model.argb[at] : 0u;
	const bool set = model.solid ? model.solid[at] != 0 : c != 0u;
	if (op == CVX_COPY_REPLACE) {
		*v = Voxel{ set, set ? c : 0u };
		*known = true;
		return;
	}
	if (!set) { return; }
	if (op == CVX_BRUSH_FILL) {
		*v = Voxel{ true, c };
		*known = true;
	} else if (op == CVX_BRUSH_CARVE) {
		*v = Voxel{ false, 0u };
		*known = true;
	} else { // PAINT
		if (!*known) {
			*v = ArenaVoxel(col, colourSlots, colorShift, y);
			*known = true;
		}
		if (v->solid) { v->argb = c; }
	}
}

// Voxel y of column (cx, cz) after the call: the instances list[0 .. count) (null: 0 .. count - 1) in order.
CVX_HD inline Voxel ModelsFinal(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const cvx_model *models, const cvx_model_instance *instances,
                                const uint16_t *list, int count, int64_t cx, int64_t cz, int64_t y)
{
	Voxel v{ false, 0u };
	bool known = false;
	for (int k = 0; k < count; k++) {
		const cvx_model_instance &I = instances[list ? (int)list[k] : k];
		if (cx < I.boxMin[0] || cx >= I.boxMax[0] || y < I.boxMin[1] || y >= I.boxMax[1] || cz < I.boxMin[2] || cz >= I.boxMax[2]) { continue; }
		int64_t s[3];
		ModelMapApply(I.toModel, cx, y, cz, s);
		ModelApply(models[I.model], I.op, s, col, colourSlots, colorShift, y, &v, &known);
	}
	return known ? v : ArenaVoxel(col, colourSlots, colorShift, y);
}

// ModelsFinal as a lane of the kernels' wave evaluates it in the step [yTop - 63, yTop] (cvx_dense.h's steps), y = yTop - lane its voxel (air
// below 0).  Everything about an instance is the same in every lane: `U` says so to the compiler (on the device readfirstlane, so that the map,
// the box and the model live in scalar registers; on the host the identity).  q_i splits into the column's part, computed on the scalar side,
// and m[i][1] * (2 y + 1), one 64-bit multiply-add per lane and axis.  An instance whose box misses the step's y range is skipped by the
// whole wave.  `list` holds instances whose boxes cover the column (the cull), so x and z are not tested again.
template <class Uniform>
CVX_HD inline Voxel ModelsLaneVoxel(const Uniform &U, const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const cvx_model *models,
                                    const cvx_model_instance *instances, const uint16_t *list, int count, int32_t cx, int32_t cz, int yTop, int y)
{
	Voxel v{ false, 0u };
	bool known = false;
	const int yLow = yTop - 63;
	for (int k = 0; k < count; k++) {
		const cvx_model_instance &I = instances[U((int32_t)list[k])];
		const int32_t lo = U(I.boxMin[1]), hi = U(I.boxMax[1]);
		if (hi <= yLow || lo > yTop) { continue; }
		int64_t part[3];
		int32_t m1[3];
		for (int i = 0; i < 3; i++) {
			const int64_t t = (int64_t)(((uint64_t)(uint32_t)U((int32_t)((uint64_t)I.toModel.t[i] >> 32)) << 32) | (uint32_t)U((int32_t)(uint32_t)I.toModel.t[i]));
			part[i] = (int64_t)U(I.toModel.m[i][0]) * (2 * (int64_t)cx + 1) + (int64_t)U(I.toModel.m[i][2]) * (2 * (int64_t)cz + 1) + 2 * t;
			m1[i] = U(I.toModel.m[i][1]);
		}
		const cvx_model &G = models[U(I.model)];
		const uintptr_t argb = (uintptr_t)G.argb, solid = (uintptr_t)G.solid;
		cvx_model M;
		for (int a = 0; a < 3; a++) { M.size[a] = U(G.size[a]); }
		M.pad_ = 0;
		M.argb = reinterpret_cast<const uint32_t *>(((uintptr_t)(uint32_t)U((int32_t)(argb >> 32)) << 32) | (uint32_t)U((int32_t)(uint32_t)argb));
		M.solid = reinterpret_cast<const uint8_t *>(((uintptr_t)(uint32_t)U((int32_t)(solid >> 32)) << 32) | (uint32_t)U((int32_t)(uint32_t)solid));
		const int op = U(I.op);
		if (y >= lo && y < hi && y >= 0) {
			const int64_t s[3] = { ModelMapFinish(part[0], m1[0], y), ModelMapFinish(part[1], m1[1], y), ModelMapFinish(part[2], m1[2], y) };
			ModelApply(M, op, s, col, colourSlots, colorShift, y, &v, &known);
		}
	}
	if (y < 0) { return Voxel{ false, 0u }; }
	return known ? v : ArenaVoxel(col, colourSlots, colorShift, y);
}
struct SameInEveryLane { // the host's Uniform
	CVX_HD int32_t operator()(int32_t v) const { return v; }
};

// What the cull reads of an instance: its box clipped to the world, 32 bytes, so that a wave's 64 lanes load 2 KB in one piece instead of 24 bytes
// out of every 96.  The host makes one per instance that touches the world (ModelCullBoxOf: false for the others, which the kernels never see).
struct ModelCullBox {
	int32_t x0, x1, z0, z1, y0, y1, pad_[2];
};
CVX_HD inline bool ModelCullBoxOf(const cvx_model_instance &I, int64_t dimX, int64_t dimY, int64_t dimZ, ModelCullBox *out)
{
	int64_t lo[3], hi[3];
	const bool onX = ModelBoxClip(I, 0, dimX, &lo[0], &hi[0]), onY = ModelBoxClip(I, 1, dimY, &lo[1], &hi[1]), onZ = ModelBoxClip(I, 2, dimZ, &lo[2], &hi[2]);
	const bool touches = onX && onY && onZ;
	*out = ModelCullBox{ (int32_t)lo[0], (int32_t)hi[0], (int32_t)lo[2], (int32_t)hi[2], (int32_t)lo[1], (int32_t)hi[1], { 0, 0 } };
	return touches;
}
// The cull's test for column (cx, cz) of the world.
CVX_HD inline bool ModelCullCovers(const ModelCullBox &b, int32_t cx, int32_t cz) { return cx >= b.x0 && cx < b.x1 && cz >= b.z0 && cz < b.z1; }

// Walks the column (cx, cz) top-down, a voxel at a time, after the call.
// Out (may be null), as BrushColumn: runs[r] = colorsIndex | length << 16 (0xFFFF for air), colours[k] = the k-th solid voxel's colour from the top.
CVX_HD inline BrushResult ModelsColumn(const ArenaColumn &col, const uint32_t *colourSlots, int colorShift, const cvx_model *models, const cvx_model_instance *instances,
                                       const uint16_t *list, int count, int64_t cx, int64_t cz, int dimY, uint32_t *outRuns, uint32_t *outColours)
{
	BrushResult res{ 0u, 0u, 0u, 0u, false };
	bool curSolid = false;
	int64_t curLength = 0, curIndex = 0; // the run being emitted
	int64_t lowest = -1, highest = -1;   // solid voxels
	for (int64_t y = (int64_t)dimY - 1; y >= 0; y--) {
		const Voxel v = ModelsFinal(col, colourSlots, colorShift, models, instances, list, count, cx, cz, y);
		if (v.solid != curSolid || curLength == 0) {
			if (curLength > 0) {
				if (outRuns) { outRuns[res.runCount] = (curSolid ? (uint32_t)curIndex : 0xFFFFu) | ((uint32_t)curLength << 16); }
				if (curLength > 32767) { res.overLimit = true; }
				res.runCount++;
			}
			curSolid = v.solid;
			curLength = 0;
			curIndex = res.colours;
			if (v.solid && curIndex > 32767) { res.overLimit = true; }
		}
		curLength++;
		if (v.solid) {
			if (outColours) { outColours[res.colours] = v.argb; }
			res.colours++;
			if (highest < 0) { highest = y + 1; }
			lowest = y;
		}
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

// Element (x, z, y) of cvx_world_read_model's arrays: the world's voxel at toWorld(s), s = (x, y, z).
CVX_HD inline Voxel ModelReadVoxel(const CopyWorld &W, const cvx_model_map &toWorld, int64_t x, int64_t y, int64_t z)
{
	int64_t d[3];
	ModelMapApply(toWorld, x, y, z, d);
	return DenseVoxel(W, d[0], d[1], d[2]);
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)
// false: `what` (e.g. "instance 3: toModel") has an entry beyond the limits; the message says which.
inline bool ModelMapValidate(const cvx_model_map &M, const char *what, char *message, size_t bytes)
{
	for (int i = 0; i < 3; i++) {
		for (int j = 0; j < 3; j++) {
			if (M.m[i][j] < -kModelMapMaxM || M.m[i][j] > kModelMapMaxM) {
				snprintf(message, bytes, "%s: m[%d][%d] = %d beyond 2^24 (256 in units of 2^-16)", what, i, j, M.m[i][j]);
				return false;
			}
		}
		if (M.t[i] < -kModelMapMaxT || M.t[i] > kModelMapMaxT) {
			snprintf(message, bytes, "%s: t[%d] = %lld beyond 2^46 (2^30 in units of 2^-16)", what, i, (long long)M.t[i]);
			return false;
		}
	}
	return true;
}

inline bool ModelSizeValidate(const int32_t size[3], const char *what, char *message, size_t bytes)
{
	int64_t n = 1;
	for (int a = 0; a < 3; a++) {
		if (size[a] < 1) {
			snprintf(message, bytes, "%s: size %d on axis %d is below 1", what, size[a], a);
			return false;
		}
		n *= size[a]; // (each factor below 2^31, the running product below 2^31 before it: no overflow)
		if (n >= ((int64_t)1 << 31)) {
			snprintf(message, bytes, "%s: 2^31 or more voxels", what);
			return false;
		}
	}
	return true;
}

// The box of instance k (the placed-model calls and the contacts): within +-2^30, no empty axis; BoxCheck's reason behind "instance <k>: "
inline bool InstanceBoxValidate(const cvx_model_instance &I, int k, char *message, size_t bytes)
{
	const int at = snprintf(message, bytes, "instance %d: ", k);
	return BoxCheck(I.boxMin, I.boxMax, kBoxWithin, message + at, bytes - (size_t)at) == 0;
}

// The argument checks of cvx_world_place_models[_device], in the order include/cpuvox_gpu_models.h lists them; false: the message says what.
inline bool ModelsValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int levelCount, char *message, size_t bytes)
{
	char what[48];
	if (!models || modelCount < 1 || modelCount > CVX_MODELS_MAX_MODELS) {
		snprintf(message, bytes, "models NULL or modelCount %d outside 1 .. %d", modelCount, CVX_MODELS_MAX_MODELS);
		return false;
	}
	if (!instances || instanceCount < 1 || instanceCount > CVX_MODELS_MAX_INSTANCES) {
		snprintf(message, bytes, "instances NULL or instanceCount %d outside 1 .. %d", instanceCount, CVX_MODELS_MAX_INSTANCES);
		return false;
	}
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) {
		snprintf(message, bytes, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1);
		return false;
	}
	for (int k = 0; k < modelCount; k++) {
		snprintf(what, sizeof what, "model %d", k);
		if (!ModelSizeValidate(models[k].size, what, message, bytes)) { return false; }
		if (!models[k].argb && !models[k].solid) {
			snprintf(message, bytes, "model %d: argb and solid are both NULL", k);
			return false;
		}
	}
	for (int k = 0; k < instanceCount; k++) {
		const cvx_model_instance &I = instances[k];
		if (I.model < 0 || I.model >= modelCount) {
			snprintf(message, bytes, "instance %d: model %d outside 0 .. %d", k, I.model, modelCount - 1);
			return false;
		}
		if (I.op < CVX_BRUSH_FILL || I.op > CVX_COPY_REPLACE) {
			snprintf(message, bytes, "instance %d: bad op %d", k, I.op);
			return false;
		}
		if (!models[I.model].argb && I.op != CVX_BRUSH_CARVE) {
			snprintf(message, bytes, "instance %d: model %d has no argb (only a CARVE may use it)", k, I.model);
			return false;
		}
		if (!InstanceBoxValidate(I, k, message, bytes)) { return false; }
		snprintf(what, sizeof what, "instance %d: toModel", k);
		if (!ModelMapValidate(I.toModel, what, message, bytes)) { return false; }
	}
	return true;
}

// cvx_model_instance_from_matrix.  Double precision, one fixed order of operations; every product is rounded before it is added (the library is
// built with -ffp-contract=off).
inline bool ModelInstanceFromMatrix(const double forward[12], const int32_t size[3], int model, int op, cvx_model_instance *out)
{
	if (!forward || !size || !out) { return false; }
	for (int k = 0; k < 12; k++) { if (!isfinite(forward[k])) { return false; } }
	for (int a = 0; a < 3; a++) { if (size[a] < 1) { return false; } }
	const double a00 = forward[0], a01 = forward[1], a02 = forward[2], a10 = forward[4], a11 = forward[5], a12 = forward[6], a20 = forward[8], a21 = forward[9],
	             a22 = forward[10];
	const double b[3] = { forward[3], forward[7], forward[11] };
	auto det2 = [](double p, double q, double r, double s) {
		const double pq = p * q, rs = r * s;
		return pq - rs;
	};
	double adj[3][3];
	adj[0][0] = det2(a11, a22, a12, a21);
	adj[0][1] = det2(a02, a21, a01, a22);
	adj[0][2] = det2(a01, a12, a02, a11);
	adj[1][0] = det2(a12, a20, a10, a22);
	adj[1][1] = det2(a00, a22, a02, a20);
	adj[1][2] = det2(a02, a10, a00, a12);
	adj[2][0] = det2(a10, a21, a11, a20);
	adj[2][1] = det2(a01, a20, a00, a21);
	adj[2][2] = det2(a00, a11, a01, a10);
	const double d0 = a00 * adj[0][0], d1 = a01 * adj[1][0], d2 = a02 * adj[2][0];
	const double det = (d0 + d1) + d2;
	if (!isfinite(det) || fabs(det) < 1e-12) { return false; }
	cvx_model_instance I{};
	for (int i = 0; i < 3; i++) {
		double inv[3];
		for (int j = 0; j < 3; j++) {
			inv[j] = adj[i][j] / det;
			const double scaled = inv[j] * 65536.0;
			if (!isfinite(scaled) || fabs(scaled) > (double)kModelMapMaxM) { return false; }
			I.toModel.m[i][j] = (int32_t)llround(scaled);
		}
		const double p0 = inv[0] * b[0], p1 = inv[1] * b[1], p2 = inv[2] * b[2];
		const double translation = -((p0 + p1) + p2), scaled = translation * 65536.0;
		if (!isfinite(scaled) || fabs(scaled) > (double)kModelMapMaxT) { return false; }
		I.toModel.t[i] = (int64_t)llround(scaled);
	}
	for (int i = 0; i < 3; i++) {
		const double row[3] = { forward[4 * i], forward[4 * i + 1], forward[4 * i + 2] };
		double lo = 0.0, hi = 0.0;
		for (int corner = 0; corner < 8; corner++) {
			const double p0 = row[0] * ((corner & 1) ? (double)size[0] : 0.0), p1 = row[1] * ((corner & 2) ? (double)size[1] : 0.0),
			                p2 = row[2] * ((corner & 4) ? (double)size[2] : 0.0);
			const double w = ((p0 + p1) + p2) + b[i];
			if (!isfinite(w)) { return false; }
			lo = corner == 0 || w < lo ? w : lo;
			hi = corner == 0 || w > hi ? w : hi;
		}
		const double limit = (double)(1 << 30);
		double boxLo = floor(lo) - 1.0, boxHi = ceil(hi) + 1.0;
		boxLo = boxLo < -limit ? -limit : boxLo;
		boxHi = boxHi > limit ? limit : boxHi;
		if (boxLo >= boxHi) { return false; } // (wholly beyond 2^30)
		I.boxMin[i] = (int32_t)boxLo;
		I.boxMax[i] = (int32_t)boxHi;
	}
	I.model = model;
	I.op = op;
	*out = I;
	return true;
}

} // namespace cvxb
