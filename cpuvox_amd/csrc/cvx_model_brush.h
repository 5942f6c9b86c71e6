// cvx_model_brush.h -- the rules of cvxd_models_brush (cvx_model_brush.hip): world-space brush strokes that carve and paint placed voxel models
// in the models' own arrays.  No world anywhere.
//
// Written once for the device AND the host (tests/test_model_brush_cpu.py compiles it with g++ through tests/model_brush_rules.cpp and compares it
// with the numpy model of tests/modelbrushmodel.py), on top of cvx_brush.h (the strokes: StrokeFootprint, StrokeSpanUnclipped, the checks),
// cvx_contacts.h (the body, a body's column job, the tall-box cut) and cvx_lift.h (the mass formula), whose rules it calls and does not repeat:
//   StrokeHolds            the voxel predicates of include/cpuvox_gpu.h, a voxel at a time: what StrokeSpanUnclipped is the interval form of
//   ModelBrushSequential   the call a stroke at a time and a voxel at a time, a later stroke seeing what the earlier ones did: the specification
//   the wave's form        the order-free rule as cvx_model_brush.hip evaluates it:
//     ModelBrushCullLane     cull: whether a stroke's footprint meets an instance's box; a bit per (instance, stroke), 64 strokes a word
//     ModelBrushLaneElement  mark: the model element of the lane's voxel if it is in the body
//     ModelBrushLaneKey      mark: the maximum key over the listed strokes whose span holds the lane's y (kModelBrushCarve, or 1 + j for a PAINT)
//     ModelBrushColumn       mark: an (instance, column) job, the lanes the 64 voxels of a step: keys into the key array, the instance's counts
//     ModelBrushApplyLane    apply: a lane's voxels of a (model, chunk) job cleared or recoloured by key, its share of the model's sums
//   the host side          ModelBrushValidate (the argument checks), ModelBrushReach / ModelBrushJobs (the jobs' prefix), ModelBrushFinish
// Nothing is float but StrokeSpanUnclipped's root estimates, which exact integers correct.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_model_brush.h"
#include "cvx_brush.h"
#include "cvx_contacts.h"
#include "cvx_lift.h"

namespace cvxb {

constexpr uint32_t kModelBrushCarve = 0x80000000u; // above every PAINT's key 1 + j: any CARVE wins, else the PAINT with the highest index
constexpr int kModelBrushChunk = 1024;              // the voxels of an apply job: 16 steps of a wave

// ---- the strokes, a voxel at a time ---------------------------------------------------------------------------------------------------------------
// Whether voxel (x, y, z) is inside the stroke: include/cpuvox_gpu.h's predicates.  The products are formed inside the footprint only, which keeps
// them in int64 for a voxel far from the stroke (58 bits for a capsule, 62 for an ellipsoid and a sphere).
CVX_HD inline bool StrokeHolds(const cvx_brush_stroke &s, int64_t x, int64_t y, int64_t z)
{
	int64_t lo[3], hi[3];
	StrokeFootprint(s, lo, hi);
	if (x < lo[0] || x >= hi[0] || y < lo[1] || y >= hi[1] || z < lo[2] || z >= hi[2]) { return false; }
	if (s.shape == CVX_SHAPE_BOX) { return true; }
	const int64_t wx = x - s.a[0], wy = y - s.a[1], wz = z - s.a[2];
	if (s.shape == CVX_SHAPE_SPHERE) { return wx * wx + wy * wy + wz * wz <= (int64_t)s.b[0] * s.b[0]; }
	if (s.shape == CVX_SHAPE_ELLIPSOID) {
		const int64_t xx = (int64_t)s.b[0] * s.b[0], yy = (int64_t)s.b[1] * s.b[1], zz = (int64_t)s.b[2] * s.b[2];
		return wx * wx * (yy * zz) + wy * wy * (xx * zz) + wz * wz * (xx * yy) <= xx * yy * zz;
	}
	const int64_t r = s.pad_, dx = (int64_t)s.b[0] - s.a[0], dy = (int64_t)s.b[1] - s.a[1], dz = (int64_t)s.b[2] - s.a[2];
	const int64_t L = dx * dx + dy * dy + dz * dz, p = wx * dx + wy * dy + wz * dz, ww = wx * wx + wy * wy + wz * wz;
	if (L == 0 || p <= 0) { return ww <= r * r; }
	if (p >= L) {
		const int64_t ux = x - s.b[0], uy = y - s.b[1], uz = z - s.b[2];
		return ux * ux + uy * uy + uz * uz <= r * r;
	}
	return ww * L - p * p <= r * r * L;
}

// ---- a model's voxels -----------------------------------------------------------------------------------------------------------------------------
// Element `at` of a model is SET: cvxb::ModelApply's rule.
CVX_HD inline bool ModelBrushSet(const cvx_model &M, int64_t at) { return M.solid ? M.solid[at] != 0 : M.argb[at] != 0u; }

// The models' arrays are written in place although cvx_model declares them const (the header says so).
CVX_HD inline void ModelBrushCarveElement(const cvx_model &M, int64_t at)
{
	if (M.solid) { const_cast<uint8_t *>(M.solid)[at] = 0; }
	if (M.argb) { const_cast<uint32_t *>(M.argb)[at] = 0u; }
}
CVX_HD inline void ModelBrushPaintElement(const cvx_model &M, int64_t at, uint32_t argb) { const_cast<uint32_t *>(M.argb)[at] = argb; }

CVX_HD inline int64_t ModelBrushVolume(const cvx_model &M) { return (int64_t)M.size[0] * M.size[1] * M.size[2]; }

// The element of model voxel s, -1 outside the model: cvxb::ModelApply's layout (X, Z, Y: y fastest).
CVX_HD inline int64_t ModelBrushElement(const cvx_model &M, const int64_t s[3])
{
	if (s[0] < 0 || s[0] >= M.size[0] || s[1] < 0 || s[1] >= M.size[1] || s[2] < 0 || s[2] >= M.size[2]) { return -1; }
	return (s[0] * M.size[2] + s[2]) * M.size[1] + s[1];
}

// What is counted of a model after the call: additions, minima and maxima of integers, so that the order of the voxels does not show.
struct ModelBrushSums {
	uint64_t voxels = 0u, carved = 0u, painted = 0u, sum[3] = { 0u, 0u, 0u }, moment[6] = { 0u, 0u, 0u, 0u, 0u, 0u };
	int32_t min[3] = { INT32_MAX, INT32_MAX, INT32_MAX }, max[3] = { INT32_MIN, INT32_MIN, INT32_MIN };

	// a set voxel (x, y, z) of the model
	CVX_HD void Add(uint32_t x, uint32_t y, uint32_t z)
	{
		const uint64_t px = x, py = y, pz = z;
		voxels++;
		sum[0] += px;
		sum[1] += py;
		sum[2] += pz;
		moment[0] += px * px;
		moment[1] += py * py;
		moment[2] += pz * pz;
		moment[3] += px * py;
		moment[4] += py * pz;
		moment[5] += pz * px;
		min[0] = (int32_t)x < min[0] ? (int32_t)x : min[0];
		min[1] = (int32_t)y < min[1] ? (int32_t)y : min[1];
		min[2] = (int32_t)z < min[2] ? (int32_t)z : min[2];
		max[0] = (int32_t)x > max[0] ? (int32_t)x : max[0];
		max[1] = (int32_t)y > max[1] ? (int32_t)y : max[1];
		max[2] = (int32_t)z > max[2] ? (int32_t)z : max[2];
	}
};

// A result before anything is counted: sums 0, the box inside out (ModelBrushFinish turns it into [min, max) or zeros).
CVX_HD inline void ModelBrushResultInit(cvxd_model_result *r)
{
	r->voxels = r->carved = r->painted = 0;
	for (int a = 0; a < 3; a++) {
		r->sum[a] = 0u;
		r->min[a] = INT32_MAX;
		r->max[a] = INT32_MIN;
	}
	for (int a = 0; a < 6; a++) { r->moment[a] = 0u; }
	r->pad_[0] = r->pad_[1] = 0;
}

// What a lane, a wave or a loop has counted into the model's result.  (The device does the same with atomics, cvx_model_brush.hip.)
inline void ModelBrushResultAdd(const ModelBrushSums &S, cvxd_model_result *r)
{
	r->voxels += (int64_t)S.voxels;
	r->carved += (int64_t)S.carved;
	r->painted += (int64_t)S.painted;
	for (int a = 0; a < 3; a++) {
		r->sum[a] += S.sum[a];
		r->min[a] = S.min[a] < r->min[a] ? S.min[a] : r->min[a];
		r->max[a] = S.max[a] > r->max[a] ? S.max[a] : r->max[a];
	}
	for (int a = 0; a < 6; a++) { r->moment[a] += S.moment[a]; }
}

// ... and once everything is: min / max so far hold the lowest and the highest set voxel.
inline void ModelBrushFinish(cvxd_model_result *r)
{
	for (int a = 0; a < 3; a++) {
		r->min[a] = r->voxels > 0 ? r->min[a] : 0;
		r->max[a] = r->voxels > 0 ? r->max[a] + 1 : 0;
	}
}

// The call's summary from its finished model results.
inline cvxd_brush_summary ModelBrushSummary(const cvxd_model_result *results, int modelCount, int64_t jobs)
{
	cvxd_brush_summary t{ 0, 0, 0, jobs };
	for (int g = 0; g < modelCount; g++) {
		t.carved += results[g].carved;
		t.painted += results[g].painted;
		t.models += results[g].carved + results[g].painted > 0 ? 1 : 0;
	}
	return t;
}

// The sums of a model as its arrays are: a voxel at a time.
inline void ModelBrushCount(const cvx_model &M, cvxd_model_result *r)
{
	ModelBrushSums S;
	for (int64_t x = 0; x < M.size[0]; x++) {
		for (int64_t z = 0; z < M.size[2]; z++) {
			for (int64_t y = 0; y < M.size[1]; y++) {
				if (ModelBrushSet(M, (x * M.size[2] + z) * M.size[1] + y)) { S.Add((uint32_t)x, (uint32_t)y, (uint32_t)z); }
			}
		}
	}
	ModelBrushResultAdd(S, r);
}

// ---- the rule, a stroke at a time and a voxel at a time -------------------------------------------------------------------------------------------
// The sequential form of the header: the instance results from the bodies as they are before the call, then every stroke in order over the bodies
// as the strokes before it left them.  touched (one byte per element of every model, volumePrefix[g] the first of model g, all 0 on entry)
// remembers the elements a PAINT touched: `painted` counts those still set at the end.  Writes the models' arrays; modelResults finished.
inline void ModelBrushSequential(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_brush_stroke *strokes,
                                 int strokeCount, const uint64_t *volumePrefix, uint8_t *touched, cvxd_model_result *modelResults, cvxd_instance_result *instanceResults)
{
	for (int g = 0; g < modelCount; g++) { ModelBrushResultInit(modelResults + g); }
	for (int k = 0; k < instanceCount; k++) {
		const cvx_model_instance &I = instances[k];
		const cvx_model &M = models[I.model];
		cvxd_instance_result r{ 0, 0 };
		for (int64_t x = I.boxMin[0]; x < I.boxMax[0]; x++) {
			for (int64_t z = I.boxMin[2]; z < I.boxMax[2]; z++) {
				for (int64_t y = I.boxMin[1]; y < I.boxMax[1]; y++) {
					int64_t s[3];
					ModelMapApply(I.toModel, x, y, z, s);
					if (!ContactModelSet(M, s)) { continue; }
					bool carve = false, paint = false;
					for (int j = 0; j < strokeCount; j++) {
						if (!StrokeHolds(strokes[j], x, y, z)) { continue; }
						carve = carve || strokes[j].op == CVX_BRUSH_CARVE;
						paint = paint || (strokes[j].op == CVX_BRUSH_PAINT && M.argb);
					}
					r.carved += carve ? 1 : 0;
					r.painted += !carve && paint ? 1 : 0;
				}
			}
		}
		if (instanceResults) { instanceResults[k] = r; }
	}
	for (int j = 0; j < strokeCount; j++) {
		const cvx_brush_stroke &stroke = strokes[j];
		int64_t lo[3], hi[3];
		StrokeFootprint(stroke, lo, hi);
		for (int k = 0; k < instanceCount; k++) {
			const cvx_model_instance &I = instances[k];
			const cvx_model &M = models[I.model];
			if (stroke.op == CVX_BRUSH_PAINT && !M.argb) { continue; }
			int64_t from[3], to[3]; // (a voxel outside the footprint is outside the stroke)
			for (int a = 0; a < 3; a++) {
				from[a] = lo[a] > I.boxMin[a] ? lo[a] : (int64_t)I.boxMin[a];
				to[a] = hi[a] < I.boxMax[a] ? hi[a] : (int64_t)I.boxMax[a];
			}
			for (int64_t x = from[0]; x < to[0]; x++) {
				for (int64_t z = from[2]; z < to[2]; z++) {
					for (int64_t y = from[1]; y < to[1]; y++) {
						if (!StrokeHolds(stroke, x, y, z)) { continue; }
						int64_t s[3];
						ModelMapApply(I.toModel, x, y, z, s);
						const int64_t at = ModelBrushElement(M, s);
						if (at < 0 || !ModelBrushSet(M, at)) { continue; }
						if (stroke.op == CVX_BRUSH_CARVE) {
							ModelBrushCarveElement(M, at);
							modelResults[I.model].carved++;
						} else {
							ModelBrushPaintElement(M, at, stroke.argb);
							touched[volumePrefix[I.model] + (uint64_t)at] = 1;
						}
					}
				}
			}
		}
	}
	for (int g = 0; g < modelCount; g++) {
		const cvx_model &M = models[g];
		ModelBrushCount(M, modelResults + g);
		const int64_t n = ModelBrushVolume(M);
		for (int64_t at = 0; at < n; at++) { modelResults[g].painted += touched[volumePrefix[g] + (uint64_t)at] != 0 && ModelBrushSet(M, at) ? 1 : 0; }
		ModelBrushFinish(modelResults + g);
	}
}

// ---- the wave's form: cull ------------------------------------------------------------------------------------------------------------------------
// Whether stroke `stroke` can touch instance I: its footprint meets the box on all three axes.  Conservative, as StrokeMeetsStrip: false only
// where no voxel of the box is inside the stroke.  A wave evaluates 64 strokes of one instance, a lane each; the ballot is word `stroke / 64` of
// the instance's list, bit `stroke % 64`: ascending stroke indices, the fold's order.
CVX_HD inline bool ModelBrushCullLane(const cvx_brush_stroke *strokes, int strokeCount, const cvx_model_instance &I, int stroke)
{
	if (stroke >= strokeCount) { return false; }
	int64_t lo[3], hi[3];
	StrokeFootprint(strokes[stroke], lo, hi);
	return lo[0] < I.boxMax[0] && hi[0] > I.boxMin[0] && lo[1] < I.boxMax[1] && hi[1] > I.boxMin[1] && lo[2] < I.boxMax[2] && hi[2] > I.boxMin[2];
}

CVX_HD inline int ModelBrushWords(int strokeCount) { return (strokeCount + 63) / 64; }

// ---- the wave's form: mark ------------------------------------------------------------------------------------------------------------------------
// The model element of voxel y of the job's column if the voxel is in the body, -1 otherwise: cvxb::ContactsLaneVoxel with the element kept.
CVX_HD inline int64_t ModelBrushLaneElement(const ContactsColumnJob &J, int32_t y)
{
	if (y < J.yLo || y >= J.yHi) { return -1; }
	const int64_t s[3] = { ModelMapFinish(J.part[0], J.m1[0], y), ModelMapFinish(J.part[1], J.m1[1], y), ModelMapFinish(J.part[2], J.m1[2], y) };
	const int64_t at = ModelBrushElement(J.M, s);
	return at >= 0 && ModelBrushSet(J.M, at) ? at : -1;
}

// The key of voxel y of column (cx, cz) in the step [yTop - 63, yTop]: the maximum over the strokes of `list` (`words` words, the cull's) whose
// span holds y of kModelBrushCarve for a CARVE and 1 + j for a PAINT (not counted when `paints` is false: a model without argb); 0: no stroke.
// Everything but y is the same in every lane: the list's words go through U, so that the strokes' fields come through scalar loads and every
// branch but the last comparison is the wave's.  A stroke whose footprint misses the column or the step is left out before its span is formed
// (which also keeps a sphere's products in int64, cvx_brush.h).
template <class Uniform>
CVX_HD inline uint32_t ModelBrushLaneKey(const Uniform &U, const cvx_brush_stroke *strokes, const uint64_t *list, int words, bool paints, int32_t cx, int32_t cz, int32_t yTop,
                                         int32_t y)
{
	uint32_t key = 0u;
	for (int w = 0; w < words; w++) {
		uint64_t left = (uint64_t)ContactUniform64(U, list[w]);
		while (left != 0ull) {
			const int j = 64 * w + (int)__builtin_ctzll(left);
			left &= left - 1ull;
			const cvx_brush_stroke &stroke = strokes[j];
			if (stroke.op == CVX_BRUSH_PAINT && !paints) { continue; }
			int64_t lo[3], hi[3];
			StrokeFootprint(stroke, lo, hi);
			if (cx < lo[0] || cx >= hi[0] || cz < lo[2] || cz >= hi[2] || lo[1] > yTop || hi[1] <= (int64_t)yTop - 63) { continue; }
			int64_t from, to;
			StrokeSpanUnclipped(stroke, cx, cz, &from, &to);
			if (y < from || y >= to) { continue; }
			const uint32_t mine = stroke.op == CVX_BRUSH_CARVE ? kModelBrushCarve : 1u + (uint32_t)j;
			key = mine > key ? mine : key;
		}
	}
	return key;
}

// The lanes of a wave at a step of a job.  Body(J, yTop, at): the ballot of "the lane's voxel yTop - l is in the body", its element in the lane's
// at[l]; Mark(..., body, keys, &carved, &painted): every lane of `body` takes its key and, if it has one, raises keys[at[l]] to it; the ballots
// of the lanes with a CARVE's key and with a PAINT's.  On the device a lane evaluates its own voxel and the wave ballots (cvx_model_brush.hip);
// on the host the 64 lanes are run one after the other:
struct ModelBrushLanesInTurn {
	mutable int64_t at[64];
	uint64_t Body(const ContactsColumnJob &J, int32_t yTop) const
	{
		uint64_t mask = 0ull;
		for (int lane = 0; lane < 64; lane++) {
			at[lane] = ModelBrushLaneElement(J, yTop - lane);
			if (at[lane] >= 0) { mask |= 1ull << lane; }
		}
		return mask;
	}
	template <class Uniform>
	void Mark(const Uniform &U, const ContactsColumnJob &J, const cvx_brush_stroke *strokes, const uint64_t *list, int words, int32_t yTop, uint64_t body, uint32_t *keys,
	          uint64_t *carved, uint64_t *painted) const
	{
		*carved = *painted = 0ull;
		for (int lane = 0; lane < 64; lane++) {
			if (((body >> lane) & 1ull) == 0ull) { continue; }
			const uint32_t key = ModelBrushLaneKey(U, strokes, list, words, J.M.argb != nullptr, J.cx, J.cz, yTop, yTop - lane);
			if (key == 0u) { continue; }
			keys[at[lane]] = key > keys[at[lane]] ? key : keys[at[lane]];
			*(key == kModelBrushCarve ? carved : painted) |= 1ull << lane;
		}
	}
};

// An (instance, column) job: column (cx, cz) of instance I's box.  keys: the key array of the instance's MODEL (one word per element).  list: the
// instance's culled strokes.  Adds to *carved / *painted what the column adds to the instance's result.  The models' arrays are only read.
template <class Uniform, class Lanes>
CVX_HD inline void ModelBrushColumn(const Uniform &U, const Lanes &L, const cvx_model *models, const cvx_model_instance &I, const cvx_brush_stroke *strokes, const uint64_t *list,
                                    int words, int32_t cx, int32_t cz, uint32_t *keys, uint32_t *carved, uint32_t *painted)
{
	const ContactsColumnJob J = ContactsColumnJobOf(U, models, I, cx, cz);
	int32_t top, low;
	ContactsStepRange(J, &top, &low);
	for (int32_t yTop = top; yTop >= low; yTop -= 64) {
		const uint64_t body = L.Body(J, yTop);
		if (body == 0ull) { continue; }
		uint64_t c, p;
		L.Mark(U, J, strokes, list, words, yTop, body, keys, &c, &p);
		*carved += (uint32_t)__builtin_popcountll(c);
		*painted += (uint32_t)__builtin_popcountll(p);
	}
}

// ---- the wave's form: apply -----------------------------------------------------------------------------------------------------------------------
// Lane `lane` of the (model, chunk) job: elements chunk * kModelBrushChunk + 64 i + lane, i = 0 .. 15, of model M, whose keys are `keys`.  An
// element with a CARVE's key is cleared, one with a PAINT's key 1 + j takes strokes[j].argb; only marked elements are written, and only set
// elements are marked.  What the lane's voxels add to the model's result goes to *S.
CVX_HD inline void ModelBrushApplyLane(const cvx_model &M, const uint32_t *keys, const cvx_brush_stroke *strokes, uint32_t volume, uint32_t chunk, int lane, ModelBrushSums *S)
{
	const uint32_t sizeY = (uint32_t)M.size[1], sizeZ = (uint32_t)M.size[2];
	for (int i = 0; i < kModelBrushChunk / 64; i++) {
		const uint64_t wide = (uint64_t)chunk * kModelBrushChunk + (uint64_t)(64 * i + lane);
		if (wide >= volume) { break; }
		const uint32_t at = (uint32_t)wide, key = keys[at];
		if (key == kModelBrushCarve) {
			ModelBrushCarveElement(M, at);
			S->carved++;
			continue;
		}
		if (key != 0u) {
			ModelBrushPaintElement(M, at, strokes[key - 1u].argb);
			S->painted++;
		} else if (!ModelBrushSet(M, at)) {
			continue;
		}
		const uint32_t column = at / sizeY;
		S->Add(column / sizeZ, at - column * sizeY, column % sizeZ);
	}
}

CVX_HD inline uint32_t ModelBrushChunks(int64_t volume) { return (uint32_t)((volume + kModelBrushChunk - 1) / kModelBrushChunk); }

// ---- the host side --------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)

// The argument checks of cvxd_models_brush[_device] in the header's order; false: the message says what.
inline bool ModelBrushValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_brush_stroke *strokes, int strokeCount,
                               const void *modelResults, char *message, size_t bytes)
{
	// (no results and no list of that call's: any address but NULL passes its check of results)
	if (!ContactsValidate(models, modelCount, instances, instanceCount, 0, message, nullptr, 0, message, bytes)) { return false; }
	if (!StrokeCountValidate(strokes, strokeCount, message, bytes) || !StrokeShapesValidate(strokes, strokeCount, message, bytes)) { return false; }
	for (int j = 0; j < strokeCount; j++) {
		if (strokes[j].op == CVX_BRUSH_FILL) {
			snprintf(message, bytes, "stroke %d: a FILL (the ops are CARVE and PAINT: growing a body is not part of this)", j);
			return false;
		}
		if (strokes[j].op == CVX_BRUSH_PAINT && strokes[j].argb == 0u) {
			snprintf(message, bytes, "stroke %d: a PAINT with argb 0 (it would unset the voxels of a model without a mask)", j);
			return false;
		}
	}
	if (!modelResults) {
		snprintf(message, bytes, "modelResults is NULL");
		return false;
	}
	// two models whose arrays overlap: every pair of arrays of different models (256 models: 2^17 comparisons at the most)
	for (int g = 0; g < modelCount; g++) {
		const uintptr_t n = (uintptr_t)ModelBrushVolume(models[g]);
		const uintptr_t from[2] = { (uintptr_t)models[g].argb, (uintptr_t)models[g].solid }, to[2] = { from[0] + 4 * n, from[1] + n };
		for (int h = 0; h < g; h++) {
			const uintptr_t m = (uintptr_t)ModelBrushVolume(models[h]);
			const uintptr_t first[2] = { (uintptr_t)models[h].argb, (uintptr_t)models[h].solid }, last[2] = { first[0] + 4 * m, first[1] + m };
			for (int a = 0; a < 4; a++) {
				if (from[a & 1] != 0 && first[a >> 1] != 0 && from[a & 1] < last[a >> 1] && first[a >> 1] < to[a & 1]) {
					snprintf(message, bytes, "models %d and %d: their arrays overlap in memory (a model is written in place: give every model its own arrays)", h, g);
					return false;
				}
			}
		}
	}
	return true;
}

// The box [lo, hi) around all strokes' footprints.
inline void ModelBrushReach(const cvx_brush_stroke *strokes, int strokeCount, int64_t lo[3], int64_t hi[3])
{
	for (int j = 0; j < strokeCount; j++) {
		int64_t l[3], h[3];
		StrokeFootprint(strokes[j], l, h);
		for (int a = 0; a < 3; a++) {
			lo[a] = j == 0 || l[a] < lo[a] ? l[a] : lo[a];
			hi[a] = j == 0 || h[a] > hi[a] ? h[a] : hi[a];
		}
	}
}

// The (instance, column) jobs of a call: an instance whose box meets the strokes' reach has one per column of its box, the others none.
// prefix[k] = the jobs of the instances before k, prefix[instanceCount] (the return value) all of them; -1, with prefix unspecified, when they
// are 2^31 - 1 or more.  Job prefix[k] + (x - boxMin.x) * (boxMax.z - boxMin.z) + (z - boxMin.z) is column (x, z) of instance k; an instance
// without jobs has prefix[k] = prefix[k + 1] and is never landed on by the search for the LAST k with prefix[k] <= job.
inline int64_t ModelBrushJobs(const cvx_model_instance *instances, int instanceCount, const cvx_brush_stroke *strokes, int strokeCount, uint32_t *prefix)
{
	int64_t lo[3], hi[3], total = 0;
	ModelBrushReach(strokes, strokeCount, lo, hi);
	for (int k = 0; k < instanceCount; k++) {
		const cvx_model_instance &I = instances[k];
		prefix[k] = (uint32_t)total;
		const bool meets = lo[0] < I.boxMax[0] && hi[0] > I.boxMin[0] && lo[1] < I.boxMax[1] && hi[1] > I.boxMin[1] && lo[2] < I.boxMax[2] && hi[2] > I.boxMin[2];
		if (meets) { total += ((int64_t)I.boxMax[0] - I.boxMin[0]) * ((int64_t)I.boxMax[2] - I.boxMin[2]); } // (both below 2^31 + 1)
		if (total >= ((int64_t)1 << 31) - 1) { return -1; }
	}
	prefix[instanceCount] = (uint32_t)total;
	return total;
}

// cvxd_model_mass behind its argument check (voxels > 0): cvx_lifted_piece_mass of { voxels, min = 0, sum, moment }.
inline void ModelBrushMass(const cvxd_model_result &r, double centre[3], double inertia[6])
{
	cvx_lifted_piece p{};
	p.piece.voxels = r.voxels;
	for (int a = 0; a < 3; a++) { p.sum[a] = r.sum[a]; }
	for (int a = 0; a < 6; a++) { p.moment[a] = r.moment[a]; }
	LiftMass(p, centre, inertia);
}

} // namespace cvxb
