// cvx_contacts.h -- the rules of cvxc_world_contacts / cvxc_contact_response (cvx_contacts.hip): where placed voxel models touch the
// device-resident world.
//
// Written once for the device AND the host (tests/test_world_contacts_cpu.py compiles it with g++ through tests/contacts_rules.cpp and compares
// it with the numpy model of tests/contactsmodel.py):
//   ContactSolid       Solid(v): cvxb::DistanceColumnAt's column, the outside rule included, and one binary search of its runs
//   ContactModelSet    whether model voxel s is SET: cvxb::ModelApply's rule (a FILL that becomes known)
//   ContactsInstance   one instance, a voxel at a time in the list's order: the specification
//   ContactsColumnJobOf, ContactsStepRange, ContactsLaneVoxel, ContactsLaneSideFaces / EndFaces, ContactsStep, ContactsColumnDone
//                      the same as a wave of cvx_contacts.hip evaluates it: a wave per (instance, column of its box), the lanes the 64 voxels
//                      of a step, top down.  Everything about the instance is the same in every lane (`U`, as cvxb::ModelsLaneVoxel's); the
//                      step's counts come from ballots (masks here), only the sum of y is kept per lane.
//   the host side      ContactsValidate (the argument checks), ContactsPairs (the footprints' prefix) and ContactResponse
// The map is cvxb::ModelMapColumnPart / ModelMapFinish: a voxel is in the body iff a FILL of the instance would write it.  Nothing is float on
// the device.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_contacts.h"
#include "cvx_distance.h"
#include "cvx_models.h"

namespace cvxb {

// Solid(y) of a column of all of space.
CVX_HD inline bool ContactColumnSolid(const DistanceColumn &c, int64_t dimY, int64_t y)
{
	if (c.allSolid) { return true; }
	if (y < 0) { return c.solidBelow; }
	if (y >= dimY) { return c.solidAbove; }
	const uint32_t k = RunAtOrBelow(c.col, y);
	return k < c.col.Count() && (int64_t)c.col.Run(k).top > y;
}

CVX_HD inline bool ContactSolid(const CopyWorld &W, int64_t x, int64_t y, int64_t z, int solidOutside)
{
	return ContactColumnSolid(DistanceColumnAt(W, x, z, solidOutside), W.dimY, y);
}

// The arena's colour word of a solid voxel; 0 outside the world.
CVX_HD inline uint32_t ContactColour(const CopyWorld &W, int64_t x, int64_t y, int64_t z)
{
	if (x < 0 || x >= W.dimX || y < 0 || y >= W.dimY || z < 0 || z >= W.dimZ) { return 0u; }
	return ArenaVoxel(CopyColumnAt(W, x, z), W.colourSlots, W.colorShift, y).argb;
}

// Model voxel s (any integers) is inside the model and SET: what makes a FILL write.
CVX_HD inline bool ContactModelSet(const cvx_model &M, const int64_t s[3])
{
	Voxel v{ false, 0u };
	bool known = false;
	ModelApply(M, CVX_BRUSH_FILL, s, ArenaColumn{ 0u, 0u, 0u, 0u, nullptr }, nullptr, 2, 0, &v, &known);
	return known;
}

// The unit step through face f.
CVX_HD inline void ContactFaceStep(int f, int64_t e[3])
{
	e[0] = e[1] = e[2] = 0;
	e[f >> 1] = (f & 1) ? 1 : -1;
}

// A result before anything is counted: sums 0, the box inside out (ContactResultFinish turns it into [min, max) or zeros).
CVX_HD inline void ContactResultInit(const cvx_model_instance &I, cvxc_contact_result *r)
{
	r->voxels = r->overlap = r->points = r->firstPoint = 0;
	for (int a = 0; a < 3; a++) {
		r->sum[a] = 0u;
		r->normal[a] = 0;
		r->origin[a] = I.boxMin[a];
		r->min[a] = INT32_MAX;
		r->max[a] = INT32_MIN;
	}
	r->pad_ = 0;
}

// ... and once everything is: min / max so far hold the lowest and the highest voxel of O_k.
CVX_HD inline void ContactResultFinish(cvxc_contact_result *r)
{
	for (int a = 0; a < 3; a++) {
		r->min[a] = r->overlap > 0 ? r->min[a] : 0;
		r->max[a] = r->overlap > 0 ? r->max[a] + 1 : 0;
	}
}

// Instance k of a call, a voxel at a time: *r whole but for firstPoint (0), its points to sink(const cvxc_contact_point &) in the list's order.
template <class Sink>
inline void ContactsInstance(const CopyWorld &W, const cvx_model *models, const cvx_model_instance &I, int k, int solidOutside, cvxc_contact_result *r, Sink &&sink)
{
	ContactResultInit(I, r);
	const cvx_model &M = models[I.model];
	for (int64_t x = I.boxMin[0]; x < I.boxMax[0]; x++) {
		for (int64_t z = I.boxMin[2]; z < I.boxMax[2]; z++) {
			for (int64_t y = (int64_t)I.boxMax[1] - 1; y >= I.boxMin[1]; y--) {
				const int64_t d[3] = { x, y, z };
				int64_t s[3];
				ModelMapApply(I.toModel, x, y, z, s);
				if (!ContactModelSet(M, s)) { continue; }
				r->voxels++;
				if (!ContactSolid(W, x, y, z, solidOutside)) { continue; }
				r->overlap++;
				int faces = 0;
				for (int f = 0; f < 6; f++) {
					int64_t e[3];
					ContactFaceStep(f, e);
					if (ContactSolid(W, x + e[0], y + e[1], z + e[2], solidOutside)) { continue; }
					faces |= 1 << f;
					for (int a = 0; a < 3; a++) { r->normal[a] += e[a]; }
				}
				for (int a = 0; a < 3; a++) {
					r->sum[a] += (uint64_t)(d[a] - I.boxMin[a]);
					r->min[a] = d[a] < r->min[a] ? (int32_t)d[a] : r->min[a];
					r->max[a] = d[a] > r->max[a] ? (int32_t)d[a] : r->max[a];
				}
				if (faces == 0) { continue; }
				r->points++;
				sink(cvxc_contact_point{ { (int32_t)x, (int32_t)y, (int32_t)z }, k, faces, ContactColour(W, x, y, z) });
			}
		}
	}
	ContactResultFinish(r);
}

// ---- the same, 64 voxels at a time ----------------------------------------------------------------------------------------------------------------
// A wave has one pair: instance k and column (cx, cz) of its box.  Its steps cover [yTop - 63, yTop], yTop = boxMax.y - 1, then 64 lower each time,
// down to boxMin.y; lane l holds the voxel yTop - l (bit l of the masks).

// What a wave knows of its pair, the same in every lane: the map's column part, the box's y range and the model's descriptor.
struct ContactsColumnJob {
	int64_t part[3];
	int32_t m1[3];
	int32_t yLo, yHi, cx, cz;
	cvx_model M;
};

template <class Uniform> CVX_HD inline int64_t ContactUniform64(const Uniform &U, uint64_t v)
{
	return (int64_t)(((uint64_t)(uint32_t)U((int32_t)(v >> 32)) << 32) | (uint32_t)U((int32_t)(uint32_t)v));
}

// Row i of a map with every entry passed through U.
template <class Uniform> CVX_HD inline void ContactUniformRow(const Uniform &U, const cvx_model_map &M, int i, cvx_model_map *out)
{
	out->m[i][0] = U(M.m[i][0]);
	out->m[i][1] = U(M.m[i][1]);
	out->m[i][2] = U(M.m[i][2]);
	out->t[i] = ContactUniform64(U, (uint64_t)M.t[i]);
}

// (every array element is addressed by a constant: the job stays in registers)
template <class Uniform>
CVX_HD inline ContactsColumnJob ContactsColumnJobOf(const Uniform &U, const cvx_model *models, const cvx_model_instance &I, int32_t cx, int32_t cz)
{
	cvx_model_map map;
	map.pad_ = 0;
	ContactUniformRow(U, I.toModel, 0, &map);
	ContactUniformRow(U, I.toModel, 1, &map);
	ContactUniformRow(U, I.toModel, 2, &map);
	ContactsColumnJob J;
	J.part[0] = ModelMapColumnPart(map, 0, cx, cz); // (every operand on the scalar side)
	J.part[1] = ModelMapColumnPart(map, 1, cx, cz);
	J.part[2] = ModelMapColumnPart(map, 2, cx, cz);
	J.m1[0] = map.m[0][1];
	J.m1[1] = map.m[1][1];
	J.m1[2] = map.m[2][1];
	J.yLo = U(I.boxMin[1]);
	J.yHi = U(I.boxMax[1]);
	J.cx = cx;
	J.cz = cz;
	const cvx_model &G = models[U(I.model)];
	J.M.size[0] = U(G.size[0]);
	J.M.size[1] = U(G.size[1]);
	J.M.size[2] = U(G.size[2]);
	J.M.pad_ = 0;
	J.M.argb = reinterpret_cast<const uint32_t *>((uintptr_t)ContactUniform64(U, (uint64_t)(uintptr_t)G.argb));
	J.M.solid = reinterpret_cast<const uint8_t *>((uintptr_t)ContactUniform64(U, (uint64_t)(uintptr_t)G.solid));
	return J;
}

// Whether the lane's voxel y belongs to the body: inside the box's y range, its image inside the model and SET.  The map and one gather.
CVX_HD inline bool ContactsLaneVoxel(const ContactsColumnJob &J, int32_t y)
{
	if (y < J.yLo || y >= J.yHi) { return false; }
	const int64_t s[3] = { ModelMapFinish(J.part[0], J.m1[0], y), ModelMapFinish(J.part[1], J.m1[1], y), ModelMapFinish(J.part[2], J.m1[2], y) };
	return ContactModelSet(J.M, s);
}

// floor(n / d), d > 0.
CVX_HD inline int64_t ContactFloorDiv(int64_t n, int64_t d)
{
	const int64_t q = n / d;
	return (n % d != 0 && n < 0) ? q - 1 : q;
}

// The steps of a pair that can hold a body voxel: *top is the first step's yTop (0 steps: below *low), the walk goes on, 64 lower a step, while
// yTop >= *low.  Boxes of up to kContactsPlainSteps steps are walked whole.  A taller one is cut to an interval that holds every y whose image
// q_i = part_i + m1_i (2 y + 1) lies in [0, size_i << 17) on all three axes, a voxel wider on both sides: what is left out holds no model
// voxel, so nothing that is counted changes, and a wave's work is bounded by its column of the body, not by the caller's box.  The steps
// stay those of the whole box (yTop = boxMax.y - 1 - 64 n).
constexpr int32_t kContactsPlainSteps = 4;
// One axis of it: [*lo, *hi] (inclusive) cut to the y whose q = part + m1 (2 y + 1) can lie in [0, size << 17).
CVX_HD inline void ContactsAxisRange(int64_t part, int32_t m1, int32_t size, int64_t *lo, int64_t *hi)
{
	const int64_t L = (int64_t)size << 17;
	int64_t a = part, b = m1;
	if (b < 0) { // 0 <= q < L  <=>  0 <= L - 1 - q < L
		a = L - 1 - a;
		b = -b;
	}
	if (b == 0) {
		if (a < 0 || a >= L) { *hi = *lo - 1; }
		return;
	}
	// a + b (2 y + 1) >= 0 and < L: y >= (-a / b - 1) / 2 and y < ((L - a) / b - 1) / 2, widened
	const int64_t from = ContactFloorDiv(-a, 2 * b) - 1, to = ContactFloorDiv(L - a, 2 * b) + 1;
	*lo = from > *lo ? from : *lo;
	*hi = to < *hi ? to : *hi;
}

CVX_HD inline void ContactsStepRange(const ContactsColumnJob &J, int32_t *top, int32_t *low)
{
	*top = J.yHi - 1;
	*low = J.yLo;
	if ((int64_t)J.yHi - J.yLo <= (int64_t)kContactsPlainSteps * 64) { return; }
	int64_t lo = J.yLo, hi = (int64_t)J.yHi - 1; // (every array element is addressed by a constant)
	ContactsAxisRange(J.part[0], J.m1[0], J.M.size[0], &lo, &hi);
	ContactsAxisRange(J.part[1], J.m1[1], J.M.size[1], &lo, &hi);
	ContactsAxisRange(J.part[2], J.m1[2], J.M.size[2], &lo, &hi);
	if (hi < lo) { // no step at all
		*low = *top + 1;
		return;
	}
	*top -= (int32_t)((((int64_t)*top - hi) / 64) * 64); // (hi <= *top: whole steps above hi are left out)
	*low = (int32_t)lo;
}

// The side faces of the lane's voxel y of column (cx, cz): a binary search of each neighbour's runs, one neighbour after the other, so that a
// wave holds one neighbour's record at a time.  Bits 0, 1, 4, 5.
CVX_HD inline int ContactsLaneSideFaces(const CopyWorld &W, int64_t cx, int64_t cz, int solidOutside, int32_t y)
{
	int faces = 0;
	faces |= ContactColumnSolid(DistanceColumnAt(W, cx - 1, cz, solidOutside), W.dimY, y) ? 0 : 0x01;
	faces |= ContactColumnSolid(DistanceColumnAt(W, cx + 1, cz, solidOutside), W.dimY, y) ? 0 : 0x02;
	faces |= ContactColumnSolid(DistanceColumnAt(W, cx, cz - 1, solidOutside), W.dimY, y) ? 0 : 0x10;
	faces |= ContactColumnSolid(DistanceColumnAt(W, cx, cz + 1, solidOutside), W.dimY, y) ? 0 : 0x20;
	return faces;
}

// The -Y / +Y faces of lane `lane` from its neighbours' bits of `solid` (the centre column's voxels of the step, ALL 64 lanes, inside the box or
// not) and the two voxels beyond the step's ends: `above` = Solid(yTop + 1), `below` = Solid(yTop - 64).  Bits 2, 3.
CVX_HD inline int ContactsLaneEndFaces(uint64_t solid, bool above, bool below, int lane)
{
	const bool up = lane == 0 ? above : ((solid >> (lane - 1)) & 1ull) != 0ull;
	const bool down = lane == 63 ? below : ((solid >> (lane + 1)) & 1ull) != 0ull;
	return (down ? 0 : 0x04) | (up ? 0 : 0x08);
}

// What a wave has counted of its pair so far: the same in every lane.
struct ContactsColumnSums {
	uint32_t voxels = 0u, overlap = 0u, points = 0u; // (a column of a box holds at most 2^31 voxels)
	int32_t normal[3] = { 0, 0, 0 };                 // overlap voxels whose face 2 a + 1 is open, less those whose face 2 a is
	int32_t yMin = INT32_MAX, yMax = INT32_MIN;
};

// A step's masks into the pair's counts: `body` the lanes of B_k, `overlap` those of O_k, `points` those with faces, face[f] the lanes of O_k
// whose bit f is set (ballots on the device).
CVX_HD inline void ContactsStep(ContactsColumnSums &S, uint64_t body, uint64_t overlap, uint64_t points, const uint64_t face[6], int32_t yTop)
{
	S.voxels += (uint32_t)__builtin_popcountll(body);
	if (overlap == 0ull) { return; }
	S.overlap += (uint32_t)__builtin_popcountll(overlap);
	S.points += (uint32_t)__builtin_popcountll(points);
	for (int a = 0; a < 3; a++) { S.normal[a] += __builtin_popcountll(face[2 * a + 1]) - __builtin_popcountll(face[2 * a]); }
	const int32_t top = yTop - (int32_t)__builtin_ctzll(overlap), low = yTop - (63 - (int32_t)__builtin_clzll(overlap));
	S.yMax = top > S.yMax ? top : S.yMax;
	S.yMin = low < S.yMin ? low : S.yMin;
}

// What a pair adds to its instance's result; `ySum`: the sum over its overlap voxels of y - boxMin.y (the lanes' sums added up).  Additions, a
// minimum and a maximum of integers: the order of the pairs does not show.  (The device does the same with atomics, cvx_contacts.hip.)
CVX_HD inline void ContactsColumnDone(const ContactsColumnSums &S, uint64_t ySum, const ContactsColumnJob &J, cvxc_contact_result *r)
{
	r->voxels += S.voxels;
	if (S.overlap == 0) { return; }
	r->overlap += S.overlap;
	r->points += S.points;
	r->sum[0] += (uint64_t)S.overlap * (uint64_t)((int64_t)J.cx - r->origin[0]);
	r->sum[1] += ySum;
	r->sum[2] += (uint64_t)S.overlap * (uint64_t)((int64_t)J.cz - r->origin[2]);
	for (int a = 0; a < 3; a++) { r->normal[a] += S.normal[a]; }
	const int32_t lo[3] = { J.cx, S.yMin, J.cz }, hi[3] = { J.cx, S.yMax, J.cz };
	for (int a = 0; a < 3; a++) {
		r->min[a] = lo[a] < r->min[a] ? lo[a] : r->min[a];
		r->max[a] = hi[a] > r->max[a] ? hi[a] : r->max[a];
	}
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)

// The argument checks of cvxc_world_contacts[_device], in the order include/cpuvox_gpu_contacts.h lists them; false: the message says what.
inline bool ContactsValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside, const void *results,
                             const void *points, int64_t pointCapacity, char *message, size_t bytes)
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
		if (!InstanceBoxValidate(I, k, message, bytes)) { return false; }
		snprintf(what, sizeof what, "instance %d: toModel", k);
		if (!ModelMapValidate(I.toModel, what, message, bytes)) { return false; }
	}
	if (solidOutside & ~0x3F) {
		snprintf(message, bytes, "unknown solidOutside bits 0x%x", (unsigned)solidOutside);
		return false;
	}
	if (!results) {
		snprintf(message, bytes, "results is NULL");
		return false;
	}
	if (pointCapacity < 0 || (pointCapacity > 0 && !points)) {
		snprintf(message, bytes, "pointCapacity %lld with %s list", (long long)pointCapacity, points ? "a" : "no");
		return false;
	}
	return true;
}

// The (instance, column) pairs of a call: prefix[k] = the pairs of the instances before k, prefix[instanceCount] (the return value) all of them;
// -1, with prefix unspecified, when they are 2^31 - 1 or more (the scan counts pairs + 1 entries in an int).  Pair prefix[k] + (x - boxMin.x) * (boxMax.z - boxMin.z) + (z - boxMin.z) is column
// (x, z) of instance k.
inline int64_t ContactsPairs(const cvx_model_instance *instances, int instanceCount, uint32_t *prefix)
{
	int64_t total = 0;
	for (int k = 0; k < instanceCount; k++) {
		prefix[k] = (uint32_t)total;
		total += ((int64_t)instances[k].boxMax[0] - instances[k].boxMin[0]) * ((int64_t)instances[k].boxMax[2] - instances[k].boxMin[2]); // (both below 2^31 + 1)
		if (total >= ((int64_t)1 << 31) - 1) { return -1; }
	}
	prefix[instanceCount] = (uint32_t)total;
	return total;
}

// The instance of pair `pair`: the last k with prefix[k] <= pair (a binary search; instances have at least one pair each).
CVX_HD inline int ContactsPairInstance(const uint32_t *prefix, int instanceCount, uint32_t pair)
{
	int lo = 0, hi = instanceCount - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (prefix[mid] <= pair) { lo = mid; } else { hi = mid - 1; }
	}
	return lo;
}

// cvxc_contact_response.  Double precision, one fixed order of operations; every operation is rounded once (the library is built with
// -ffp-contract=off).
inline bool ContactResponse(const cvxc_contact_result *r, double centre[3], double normal[3], double *depth)
{
	if (!r || r->overlap <= 0) { return false; }
	const double n = (double)r->overlap;
	double g[3];
	for (int a = 0; a < 3; a++) {
		const double mean = (double)r->sum[a] / n;
		if (centre) { centre[a] = ((double)r->origin[a] + mean) + 0.5; }
		g[a] = (double)r->normal[a];
	}
	const double xx = g[0] * g[0], yy = g[1] * g[1], zz = g[2] * g[2];
	const double len = sqrt((xx + yy) + zz);
	for (int a = 0; a < 3; a++) {
		if (normal) { normal[a] = len > 0.0 ? g[a] / len : 0.0; }
	}
	if (depth) { *depth = len > 0.0 ? n / len : 0.0; }
	return true;
}

} // namespace cvxb
