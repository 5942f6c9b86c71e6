// cvx_model_pick.h -- the rules of cvxq_model_pick (cvx_model_pick.hip): first-hit rays against placed voxel models.
//
// Written once for the device AND the host (tests/test_model_pick_cpu.py compiles it with g++ through tests/model_pick_rules.cpp and compares it
// with the numpy model of tests/modelpickmodel.py):
//   ModelPickClip        steps 1 .. 3 of the pair rule (include/cpuvox_gpu_model_pick.h): the ray against the instance's box, the start state
//   ModelPickAdvance     one step of the rule's loop from a voxel that is not in the body
//   ModelPickSequential  the pair rule, a voxel at a time: the specification
//   ModelPickMajor, ModelPickCrossings, ModelPickLayer, ModelPickStepTime
//                        the same as a wave of cvx_model_pick.hip evaluates it: a wave per (ray, instance) job, the lanes 64 consecutive layers
//                        of the box along the ray's dominant axis M.  The sequential loop is a stable merge of three monotone sequences of
//                        crossing times, each a closed form of the plane's index ((plane - o_a) * inv_a: a rounded subtraction and a rounded
//                        product by a constant keep the order of the planes).  A crossing of axis a comes before one of axis b iff its time is
//                        smaller, or equal with a < b.  So when the ray enters layer j at T_j (the crossing of M into it), a minor axis a has
//                        made exactly the crossings whose time is < T_j (<= T_j for a < M): a count that needs no walk.  From that state the
//                        lane runs the rule's own loop -- ModelPickAdvance, the same comparisons of the same products -- until it hits, ends
//                        or crosses M.  Every crossing of the sequential walk is made by exactly one layer, from the same state.
//   ModelPickKey / ModelPickMiss / ModelPickHitOf   the ray rule's key and the records
// The body test is cvx_contacts.h's (the int64 map, then ContactModelSet).  All of the ray is float64; the product is built with
// -ffp-contract=off, every operation is rounded once.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_model_pick.h"
#include "cvx_brush.h"
#include "cvx_contacts.h"
#include "cvx_pair_contacts.h"

// the walk's functions are inlined whatever the optimisation level: a job handed on by reference would otherwise live in memory
#define CVX_PICK_INLINE inline __attribute__((always_inline))

namespace cvxb {

// A ray as the rule reads it, once clipped to an instance's box.
struct ModelPickRay {
	double o[3], d[3], inv[3]; // inv: 1 / d, 0 where d is 0
	double tEnter, tExit;
};

// Where the walk is: the voxel, the face it was entered through and when.
struct ModelPickState {
	int32_t v[3];
	int32_t face;
	double t;
};

// What a walk reads of its instance: the box, the map and the model's descriptor.
struct ModelPickBody {
	int32_t lo[3], hi[3];
	cvx_model_map map;
	cvx_model M;
};

enum { kModelPickGo = 0, kModelPickHit = 1, kModelPickEnd = 2 };

template <class Uniform> CVX_HD CVX_PICK_INLINE ModelPickBody ModelPickBodyOf(const Uniform &U, const cvx_model *models, const cvx_model_instance &I)
{
	ModelPickBody B;
	B.lo[0] = U(I.boxMin[0]);
	B.lo[1] = U(I.boxMin[1]);
	B.lo[2] = U(I.boxMin[2]);
	B.hi[0] = U(I.boxMax[0]);
	B.hi[1] = U(I.boxMax[1]);
	B.hi[2] = U(I.boxMax[2]);
	B.map.pad_ = 0;
	ContactUniformRow(U, I.toModel, 0, &B.map);
	ContactUniformRow(U, I.toModel, 1, &B.map);
	ContactUniformRow(U, I.toModel, 2, &B.map);
	const cvx_model &G = models[U(I.model)];
	B.M.size[0] = U(G.size[0]);
	B.M.size[1] = U(G.size[1]);
	B.M.size[2] = U(G.size[2]);
	B.M.pad_ = 0;
	B.M.argb = reinterpret_cast<const uint32_t *>((uintptr_t)ContactUniform64(U, (uint64_t)(uintptr_t)G.argb));
	B.M.solid = reinterpret_cast<const uint8_t *>((uintptr_t)ContactUniform64(U, (uint64_t)(uintptr_t)G.solid));
	return B;
}

// s = toModel(v), and whether v (inside the box) is in the body.
CVX_HD CVX_PICK_INLINE bool ModelPickInBody(const ModelPickBody &B, const int32_t v[3], int64_t s[3])
{
	s[0] = ModelMapFinish(ModelMapColumnPart(B.map, 0, v[0], v[2]), B.map.m[0][1], v[1]); // (ModelMapApply, every element addressed by a constant)
	s[1] = ModelMapFinish(ModelMapColumnPart(B.map, 1, v[0], v[2]), B.map.m[1][1], v[1]);
	s[2] = ModelMapFinish(ModelMapColumnPart(B.map, 2, v[0], v[2]), B.map.m[2][1], v[1]);
	return ContactModelSet(B.M, s);
}

// Step 2 on axis a (a constant at every call): false is a miss.  S->face follows the entry axis.
CVX_HD CVX_PICK_INLINE bool ModelPickClipAxis(int a, double o, double d, int32_t lo, int32_t hi, ModelPickRay *R, ModelPickState *S)
{
	const double inv = d == 0.0 ? 0.0 : 1.0 / d;
	if (a == 0) { R->o[0] = o, R->d[0] = d, R->inv[0] = inv; }
	if (a == 1) { R->o[1] = o, R->d[1] = d, R->inv[1] = inv; }
	if (a == 2) { R->o[2] = o, R->d[2] = d, R->inv[2] = inv; }
	if (!Finite(o) || !Finite(d)) { return false; }
	if (d == 0.0) { return o >= (double)lo && o < (double)hi; }
	double t0 = ((double)lo - o) * inv, t1 = ((double)hi - o) * inv;
	if (t0 > t1) {
		const double s = t0;
		t0 = t1;
		t1 = s;
	}
	if (t0 > R->tEnter) {
		R->tEnter = t0;
		S->face = 2 * a + (d > 0.0 ? 0 : 1);
	}
	if (t1 < R->tExit) { R->tExit = t1; }
	return true;
}

// Step 3 on one axis.
CVX_HD CVX_PICK_INLINE int32_t ModelPickStartVoxel(double o, double d, double tEnter, int32_t lo, int32_t hi)
{
	const double p = __builtin_floor(o + tEnter * d);
	return p < (double)lo ? lo : (p > (double)(hi - 1) ? hi - 1 : (int32_t)p);
}

// Steps 1 .. 3: false is a miss.
CVX_HD CVX_PICK_INLINE bool ModelPickClip(const float originF[3], const float directionF[3], float maxTF, const int32_t lo[3], const int32_t hi[3], ModelPickRay *R,
                                 ModelPickState *S)
{
	const double maxT = (double)maxTF;
	if (!(maxT >= 0.0)) { return false; }
	R->tEnter = 0.0;
	R->tExit = maxT;
	S->face = 6;
	// (axis after axis, every array element addressed by a constant: the ray stays in registers)
	if (!ModelPickClipAxis(0, (double)originF[0], (double)directionF[0], lo[0], hi[0], R, S)) { return false; }
	if (!ModelPickClipAxis(1, (double)originF[1], (double)directionF[1], lo[1], hi[1], R, S)) { return false; }
	if (!ModelPickClipAxis(2, (double)originF[2], (double)directionF[2], lo[2], hi[2], R, S)) { return false; }
	if (!(R->tEnter <= R->tExit)) { return false; }
	S->v[0] = ModelPickStartVoxel(R->o[0], R->d[0], R->tEnter, lo[0], hi[0]);
	S->v[1] = ModelPickStartVoxel(R->o[1], R->d[1], R->tEnter, lo[1], hi[1]);
	S->v[2] = ModelPickStartVoxel(R->o[2], R->d[2], R->tEnter, lo[2], hi[2]);
	S->t = R->tEnter;
	return true;
}

// Element a of three values (by value: a select of values, never of addresses, so that the structures they come from stay in registers).
template <class T> CVX_HD CVX_PICK_INLINE T ModelPickOf(int a, T x, T y, T z) { return a == 0 ? x : (a == 1 ? y : z); }

// tNext_a from voxel coordinate v on axis a (d_a != 0): when the ray crosses the plane it leaves the voxel through.
CVX_HD CVX_PICK_INLINE double ModelPickCross(double o, double d, double inv, int64_t v) { return ((double)(v + (d > 0.0 ? 1 : 0)) - o) * inv; }

// One step of the loop from a voxel that is not in the body: the axis stepped along, S moved on; -1: the ray ends (a miss).
CVX_HD CVX_PICK_INLINE int ModelPickAdvance(const ModelPickRay &R, const int32_t lo[3], const int32_t hi[3], ModelPickState *S)
{
	const double inf = __builtin_inf();
	const double t0 = R.d[0] != 0.0 ? ModelPickCross(R.o[0], R.d[0], R.inv[0], S->v[0]) : inf;
	const double t1 = R.d[1] != 0.0 ? ModelPickCross(R.o[1], R.d[1], R.inv[1], S->v[1]) : inf;
	const double t2 = R.d[2] != 0.0 ? ModelPickCross(R.o[2], R.d[2], R.inv[2], S->v[2]) : inf;
	int a = 0;
	double tNext = t0;
	if (t1 < tNext) {
		a = 1;
		tNext = t1;
	}
	if (t2 < tNext) {
		a = 2;
		tNext = t2;
	}
	if (tNext > R.tExit || tNext == inf) { return -1; } // (inf: a zero direction tests the origin's voxel alone)
	const bool up = ModelPickOf(a, R.d[0], R.d[1], R.d[2]) > 0.0;
	const int32_t w = ModelPickOf(a, S->v[0], S->v[1], S->v[2]) + (up ? 1 : -1);
	const int32_t l = ModelPickOf(a, lo[0], lo[1], lo[2]), h = ModelPickOf(a, hi[0], hi[1], hi[2]);
	if (w < l || w >= h) { return -1; }
	S->v[0] = a == 0 ? w : S->v[0]; // (every array element is addressed by a constant: the state stays in registers)
	S->v[1] = a == 1 ? w : S->v[1];
	S->v[2] = a == 2 ? w : S->v[2];
	S->t = tNext;
	S->face = 2 * a + (up ? 0 : 1);
	return a;
}

// The pair rule from its start state on, a voxel at a time: true with S the hit and s its model voxel.
CVX_HD inline bool ModelPickSequential(const ModelPickRay &R, const ModelPickBody &B, ModelPickState *S, int64_t s[3])
{
	for (;;) {
		if (ModelPickInBody(B, S->v, s)) { return true; }
		if (ModelPickAdvance(R, B.lo, B.hi, S) < 0) { return false; }
	}
}

// ---- the same, 64 layers at a time ----------------------------------------------------------------------------------------------------------------

// The dominant axis: the largest |d_a|, the lower axis on a tie (a zero direction: 0, and layer 0 ends the walk).
CVX_HD CVX_PICK_INLINE int ModelPickMajor(const ModelPickRay &R)
{
	const double x = __builtin_fabs(R.d[0]), y = __builtin_fabs(R.d[1]), z = __builtin_fabs(R.d[2]);
	return x >= y && x >= z ? 0 : (y >= z ? 1 : 2);
}

// The crossings minor axis a has made, from start voxel `from`, when the ray crosses the dominant axis at time T: those whose time is < T, or
// <= T with `ties` (a below the dominant axis).  At most `limit` = the crossings inside the box + 1 (the last one leaves it).  The estimate
// comes from the ray's position at T; the two loops make it exact by the rule's own products, whatever the estimate was.
CVX_HD CVX_PICK_INLINE int64_t ModelPickCrossings(double o, double d, double inv, int32_t from, int32_t lo, int32_t hi, double T, bool ties)
{
	if (d == 0.0) { return 0; }
	const int64_t step = d > 0.0 ? 1 : -1;
	const int64_t limit = (d > 0.0 ? (int64_t)hi - 1 - from : (int64_t)from - lo) + 1;
	const double moved = (__builtin_floor(o + T * d) - (double)from) * (double)step;
	int64_t n = moved > 0.0 ? (moved < (double)limit ? (int64_t)moved : limit) : 0; // (a NaN estimate: 0)
	while (n > 0) {
		const double c = ModelPickCross(o, d, inv, (int64_t)from + (n - 1) * step);
		if (ties ? c <= T : c < T) { break; }
		n--;
	}
	while (n < limit) {
		const double c = ModelPickCross(o, d, inv, (int64_t)from + n * step);
		if (!(ties ? c <= T : c < T)) { break; }
		n++;
	}
	return n;
}

// When the ray enters layer j >= 1 of the walk from `start` along dominant axis M.
CVX_HD CVX_PICK_INLINE double ModelPickLayerTime(const ModelPickRay &R, int M, int32_t startM, int64_t j)
{
	const double o = ModelPickOf(M, R.o[0], R.o[1], R.o[2]), d = ModelPickOf(M, R.d[0], R.d[1], R.d[2]), inv = ModelPickOf(M, R.inv[0], R.inv[1], R.inv[2]);
	return ModelPickCross(o, d, inv, (int64_t)startM + (j - 1) * (d > 0.0 ? 1 : -1));
}

// Layer j >= 0 of the walk that starts in state `start` (ModelPickClip's): kModelPickHit with *S the hit and s its model voxel, kModelPickEnd
// when the ray ends in the layer (or the layer lies outside the box), kModelPickGo when it goes on into layer j + 1.  The answer of layer j
// counts only if every layer before it said Go.
CVX_HD CVX_PICK_INLINE int ModelPickLayer(const ModelPickRay &R, const ModelPickBody &B, const ModelPickState &start, int M, int64_t j, ModelPickState *S, int64_t s[3])
{
	*S = start;
	if (j > 0) {
		const int32_t startM = ModelPickOf(M, start.v[0], start.v[1], start.v[2]);
		const double dM = ModelPickOf(M, R.d[0], R.d[1], R.d[2]);
		const int64_t layer = (int64_t)startM + j * (dM > 0.0 ? 1 : -1);
		const int32_t l = ModelPickOf(M, B.lo[0], B.lo[1], B.lo[2]), h = ModelPickOf(M, B.hi[0], B.hi[1], B.hi[2]);
		if (dM == 0.0 || layer < l || layer >= h) { return kModelPickEnd; }
		const double T = ModelPickLayerTime(R, M, startM, j);
		const int64_t n0 = M == 0 ? 0 : ModelPickCrossings(R.o[0], R.d[0], R.inv[0], start.v[0], B.lo[0], B.hi[0], T, true);
		const int64_t n1 = M == 1 ? 0 : ModelPickCrossings(R.o[1], R.d[1], R.inv[1], start.v[1], B.lo[1], B.hi[1], T, 1 < M);
		const int64_t n2 = M == 2 ? 0 : ModelPickCrossings(R.o[2], R.d[2], R.inv[2], start.v[2], B.lo[2], B.hi[2], T, false);
		const int64_t w0 = M == 0 ? layer : (int64_t)start.v[0] + (R.d[0] > 0.0 ? n0 : -n0);
		const int64_t w1 = M == 1 ? layer : (int64_t)start.v[1] + (R.d[1] > 0.0 ? n1 : -n1);
		const int64_t w2 = M == 2 ? layer : (int64_t)start.v[2] + (R.d[2] > 0.0 ? n2 : -n2);
		if (w0 < B.lo[0] || w0 >= B.hi[0] || w1 < B.lo[1] || w1 >= B.hi[1] || w2 < B.lo[2] || w2 >= B.hi[2]) { return kModelPickEnd; } // (it left the box before)
		S->v[0] = (int32_t)w0;
		S->v[1] = (int32_t)w1;
		S->v[2] = (int32_t)w2;
		S->t = T;
		S->face = 2 * M + (dM > 0.0 ? 0 : 1);
	}
	for (;;) {
		if (ModelPickInBody(B, S->v, s)) { return kModelPickHit; }
		const int a = ModelPickAdvance(R, B.lo, B.hi, S);
		if (a < 0) { return kModelPickEnd; }
		if (a == M) { return kModelPickGo; }
	}
}

// ---- the ray rule ------------------------------------------------------------------------------------------------------------------------------------

// Step 5: the reported t.
CVX_HD inline float ModelPickReported(double t) { return (float)t + 0.0f; }

CVX_HD inline uint32_t ModelPickFloatBits(float t)
{
	union {
		float f;
		uint32_t u;
	} bits;
	bits.f = t;
	return bits.u;
}

// A hit's key: the least key of a ray wins (non-negative floats order as their bits; equal floats: the lower instance).  No hit: kModelPickNoKey.
constexpr uint64_t kModelPickNoKey = ~0ull;
CVX_HD inline uint64_t ModelPickKey(float reported, int instance) { return ((uint64_t)ModelPickFloatBits(reported) << 32) | (uint32_t)instance; }

CVX_HD inline cvxq_model_hit ModelPickMiss(float maxT) { return cvxq_model_hit{ { -1, -1, -1 }, -1, 0u, maxT, -1, { -1, -1, -1 }, { 0, 0 } }; }

CVX_HD inline cvxq_model_hit ModelPickHitOf(const ModelPickBody &B, const ModelPickState &S, const int64_t s[3], int instance)
{
	return cvxq_model_hit{ { S.v[0], S.v[1], S.v[2] }, S.face, PairModelColour(B.M, s), ModelPickReported(S.t), instance, { (int32_t)s[0], (int32_t)s[1], (int32_t)s[2] }, { 0, 0 } };
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------------
// (a plain host function: not CVX_HD)

// The argument checks of cvxq_model_pick[_device]: ContactsValidate's of the models and the instances, then the rays and the hits.
inline bool ModelPickValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const void *rays, int rayCount,
                              const void *hits, char *message, size_t bytes)
{
	if (!ContactsValidate(models, modelCount, instances, instanceCount, 0, message /* (its `results`: not ours) */, nullptr, 0, message, bytes)) { return false; }
	if (!rays || !hits) {
		snprintf(message, bytes, "%s is NULL", !rays ? "rays" : "hits");
		return false;
	}
	if (rayCount < 1 || rayCount > CVXQ_PICK_MAX_RAYS) {
		snprintf(message, bytes, "rayCount %d outside 1 .. %d", rayCount, CVXQ_PICK_MAX_RAYS);
		return false;
	}
	return true;
}

} // namespace cvxb
