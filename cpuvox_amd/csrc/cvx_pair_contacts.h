// cvx_pair_contacts.h -- the rules of cvxp_model_contacts / cvxp_box_pairs / cvxp_pair_response (cvx_pair_contacts.hip): where placed voxel
// models touch each other.  No world anywhere.
//
// Written once for the device AND the host (tests/test_model_contacts_cpu.py compiles it with g++ through tests/pair_contacts_rules.cpp and
// compares it with the numpy model of tests/paircontactsmodel.py), on top of cvx_contacts.h and cvx_models.h, whose rules it calls and does not
// repeat: the body rule is cvxb::ContactModelSet, the map cvxb::ModelMapColumnPart / ModelMapFinish, the tall-box cut cvxb::ContactsStepRange,
// the +-Y faces cvxb::ContactsLaneEndFaces, the response cvxb::ContactResponse.
//   PairBodyHas, PairOf        whether voxel d is in B_k; one pair, a voxel at a time in the list's order: the specification
//   PairSearchProbe / Narrow, PairBodyJobOf, PairStepRange, PairNeighbourVoxel, PairLaneSideFaces, PairStep, PairColumnDone
//                              the same as a wave of cvx_pair_contacts.hip evaluates it: a wave per (pair, column of X_p) job, the lanes the 64
//                              voxels of a step, top down.  BOTH bodies' column jobs are the same in every lane (`U`); each keeps its own box on
//                              all three axes, because a neighbour column or voxel outside a body's own box is not in that body although the walk's
//                              box is X_p.
//   the host side              PairsValidate (the argument checks), PairJobs (the prefix of the footprints of X_p), BoxPairs, PairResponse
// Nothing is float on the device.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "cpuvox_gpu_pair_contacts.h"
#include "cvx_contacts.h"

namespace cvxb {

// d is in B_k: inside the instance's own box, its image inside the model and SET.
CVX_HD inline bool PairBodyHas(const cvx_model *models, const cvx_model_instance &I, int64_t x, int64_t y, int64_t z)
{
	if (x < I.boxMin[0] || x >= I.boxMax[0] || y < I.boxMin[1] || y >= I.boxMax[1] || z < I.boxMin[2] || z >= I.boxMax[2]) { return false; }
	int64_t s[3];
	ModelMapApply(I.toModel, x, y, z, s);
	return ContactModelSet(models[I.model], s);
}

// The model's colour word of model voxel s (inside the model): 0 for a model without argb.
CVX_HD inline uint32_t PairModelColour(const cvx_model &M, const int64_t s[3])
{
	return M.argb ? M.argb[(s[0] * M.size[2] + s[2]) * M.size[1] + s[1]] : 0u;
}

// X_p = [lo, hi) on every axis (empty: lo >= hi on some axis); false when it is empty.
CVX_HD inline bool PairBox(const cvx_model_instance &A, const cvx_model_instance &B, int32_t lo[3], int32_t hi[3])
{
	bool any = true;
	for (int i = 0; i < 3; i++) {
		lo[i] = A.boxMin[i] > B.boxMin[i] ? A.boxMin[i] : B.boxMin[i];
		hi[i] = A.boxMax[i] < B.boxMax[i] ? A.boxMax[i] : B.boxMax[i];
		any = any && lo[i] < hi[i];
	}
	return any;
}

// A result before anything is counted: sums 0, the box inside out (PairResultFinish turns it into [min, max) or zeros).
CVX_HD inline void PairResultInit(const cvx_model_instance &A, const cvx_model_instance &B, int32_t a, int32_t b, cvxp_pair_result *r)
{
	int32_t lo[3], hi[3];
	PairBox(A, B, lo, hi);
	r->overlap = r->points = r->firstPoint = 0;
	for (int i = 0; i < 3; i++) {
		r->sum[i] = 0u;
		r->pushA[i] = r->pushB[i] = 0;
		r->origin[i] = lo[i];
		r->min[i] = INT32_MAX;
		r->max[i] = INT32_MIN;
	}
	r->a = a;
	r->b = b;
	r->pad_ = 0;
}

CVX_HD inline void PairResultFinish(cvxp_pair_result *r)
{
	for (int i = 0; i < 3; i++) {
		r->min[i] = r->overlap > 0 ? r->min[i] : 0;
		r->max[i] = r->overlap > 0 ? r->max[i] + 1 : 0;
	}
}

// Pair p = (a, b) of a call, a voxel at a time: *r whole but for firstPoint (0), its points to sink(const cvxp_pair_point &) in the list's order.
template <class Sink>
inline void PairOf(const cvx_model *models, const cvx_model_instance *instances, int p, int32_t a, int32_t b, cvxp_pair_result *r, Sink &&sink)
{
	const cvx_model_instance &A = instances[a], &B = instances[b];
	PairResultInit(A, B, a, b, r);
	int32_t lo[3], hi[3];
	if (!PairBox(A, B, lo, hi)) {
		PairResultFinish(r);
		return;
	}
	for (int64_t x = lo[0]; x < hi[0]; x++) {
		for (int64_t z = lo[2]; z < hi[2]; z++) {
			for (int64_t y = (int64_t)hi[1] - 1; y >= lo[1]; y--) {
				if (!PairBodyHas(models, A, x, y, z) || !PairBodyHas(models, B, x, y, z)) { continue; }
				r->overlap++;
				const int64_t d[3] = { x, y, z };
				int facesA = 0, facesB = 0;
				for (int f = 0; f < 6; f++) {
					int64_t e[3];
					ContactFaceStep(f, e);
					if (!PairBodyHas(models, A, x + e[0], y + e[1], z + e[2])) {
						facesA |= 1 << f;
						for (int i = 0; i < 3; i++) { r->pushB[i] += e[i]; }
					}
					if (!PairBodyHas(models, B, x + e[0], y + e[1], z + e[2])) {
						facesB |= 1 << f;
						for (int i = 0; i < 3; i++) { r->pushA[i] += e[i]; }
					}
				}
				for (int i = 0; i < 3; i++) {
					r->sum[i] += (uint64_t)(d[i] - lo[i]);
					r->min[i] = d[i] < r->min[i] ? (int32_t)d[i] : r->min[i];
					r->max[i] = d[i] > r->max[i] ? (int32_t)d[i] : r->max[i];
				}
				if ((facesA | facesB) == 0) { continue; }
				r->points++;
				int64_t sa[3], sb[3];
				ModelMapApply(A.toModel, x, y, z, sa);
				ModelMapApply(B.toModel, x, y, z, sb);
				sink(cvxp_pair_point{ { (int32_t)x, (int32_t)y, (int32_t)z }, p, facesA, facesB, PairModelColour(models[A.model], sa), PairModelColour(models[B.model], sb) });
			}
		}
	}
	PairResultFinish(r);
}

// ---- the same, 64 voxels at a time ----------------------------------------------------------------------------------------------------------------
// A wave has one job: pair p and column (cx, cz) of X_p.  Its steps cover [yTop - 63, yTop], yTop = X_p's hi.y - 1, then 64 lower each time, down
// to X_p's lo.y; lane l holds the voxel yTop - l (bit l of the masks).

// What a wave knows of ONE body of its pair, the same in every lane: cvx_contacts.h's job of the centre column (with the body's OWN y range), the
// map's x and z columns, from which a neighbour column's part follows by one addition, and the body's own box on x and z.
struct PairBodyJob {
	ContactsColumnJob J;
	int32_t m0[3], m2[3];
	int32_t x0, x1, z0, z1;
};

// (every array element is addressed by a constant: the job stays in registers)
template <class Uniform>
CVX_HD inline PairBodyJob PairBodyJobOf(const Uniform &U, const cvx_model *models, const cvx_model_instance &I, int32_t cx, int32_t cz)
{
	PairBodyJob B;
	B.J = ContactsColumnJobOf(U, models, I, cx, cz);
	B.m0[0] = U(I.toModel.m[0][0]);
	B.m0[1] = U(I.toModel.m[1][0]);
	B.m0[2] = U(I.toModel.m[2][0]);
	B.m2[0] = U(I.toModel.m[0][2]);
	B.m2[1] = U(I.toModel.m[1][2]);
	B.m2[2] = U(I.toModel.m[2][2]);
	B.x0 = U(I.boxMin[0]);
	B.x1 = U(I.boxMax[0]);
	B.z0 = U(I.boxMin[2]);
	B.z1 = U(I.boxMax[2]);
	return B;
}

// The steps of a job: ContactsStepRange of each body over X_p's y range [yLo, yHi), intersected.  Both ranges keep the steps of X_p
// (yTop = yHi - 1 - 64 n), so the later of the two tops and the higher of the two lows bound the steps that can hold a voxel of BOTH bodies.
CVX_HD inline void PairStepRange(const PairBodyJob &A, const PairBodyJob &B, int32_t yLo, int32_t yHi, int32_t *top, int32_t *low)
{
	ContactsColumnJob a = A.J, b = B.J;
	a.yLo = b.yLo = yLo;
	a.yHi = b.yHi = yHi;
	int32_t topB, lowB;
	ContactsStepRange(a, top, low);
	ContactsStepRange(b, &topB, &lowB);
	*top = topB < *top ? topB : *top;
	*low = lowB > *low ? lowB : *low;
}

// Whether voxel y of the neighbour column (cx + dx, cz + dz) belongs to the body: the column inside the body's own box, then
// ContactsLaneVoxel with the column part moved by the map's x and z columns (ModelMapColumnPart is linear in 2 v + 1: exact in int64).
CVX_HD inline bool PairNeighbourVoxel(const PairBodyJob &B, int dx, int dz, int32_t y)
{
	const int32_t x = B.J.cx + dx, z = B.J.cz + dz;
	if (x < B.x0 || x >= B.x1 || z < B.z0 || z >= B.z1) { return false; }
	ContactsColumnJob N = B.J;
	N.part[0] += 2 * ((int64_t)dx * B.m0[0] + (int64_t)dz * B.m2[0]); // (every operand on the scalar side)
	N.part[1] += 2 * ((int64_t)dx * B.m0[1] + (int64_t)dz * B.m2[1]);
	N.part[2] += 2 * ((int64_t)dx * B.m0[2] + (int64_t)dz * B.m2[2]);
	return ContactsLaneVoxel(N, y);
}

// The side faces of the lane's voxel y against one body, one neighbour column after the other, so that a wave holds one neighbour's parts at a
// time.  Bits 0, 1, 4, 5.
CVX_HD inline int PairLaneSideFaces(const PairBodyJob &B, int32_t y)
{
	int faces = 0;
	faces |= PairNeighbourVoxel(B, -1, 0, y) ? 0 : 0x01;
	faces |= PairNeighbourVoxel(B, +1, 0, y) ? 0 : 0x02;
	faces |= PairNeighbourVoxel(B, 0, -1, y) ? 0 : 0x10;
	faces |= PairNeighbourVoxel(B, 0, +1, y) ? 0 : 0x20;
	return faces;
}

// What a wave has counted of its job so far: the same in every lane.
struct PairColumnSums {
	uint32_t overlap = 0u, points = 0u; // (a column of a box holds at most 2^31 voxels)
	int32_t pushA[3] = { 0, 0, 0 }, pushB[3] = { 0, 0, 0 };
	int32_t yMin = INT32_MAX, yMax = INT32_MIN;
};

// A step's masks into the job's counts: `overlap` the lanes of O_p, `points` those with a face, faceA[f] / faceB[f] the lanes of O_p whose bit f
// of facesA / facesB is set (ballots on the device).
CVX_HD inline void PairStep(PairColumnSums &S, uint64_t overlap, uint64_t points, const uint64_t faceA[6], const uint64_t faceB[6], int32_t yTop)
{
	if (overlap == 0ull) { return; }
	S.overlap += (uint32_t)__builtin_popcountll(overlap);
	S.points += (uint32_t)__builtin_popcountll(points);
	// (every array element is addressed by a constant: the sums stay in registers)
	S.pushA[0] += __builtin_popcountll(faceB[1]) - __builtin_popcountll(faceB[0]);
	S.pushA[1] += __builtin_popcountll(faceB[3]) - __builtin_popcountll(faceB[2]);
	S.pushA[2] += __builtin_popcountll(faceB[5]) - __builtin_popcountll(faceB[4]);
	S.pushB[0] += __builtin_popcountll(faceA[1]) - __builtin_popcountll(faceA[0]);
	S.pushB[1] += __builtin_popcountll(faceA[3]) - __builtin_popcountll(faceA[2]);
	S.pushB[2] += __builtin_popcountll(faceA[5]) - __builtin_popcountll(faceA[4]);
	const int32_t top = yTop - (int32_t)__builtin_ctzll(overlap), low = yTop - (63 - (int32_t)__builtin_clzll(overlap));
	S.yMax = top > S.yMax ? top : S.yMax;
	S.yMin = low < S.yMin ? low : S.yMin;
}

// What a job adds to its pair's result; `ySum`: the sum over its overlap voxels of y - origin.y (the lanes' sums added up).  Additions, a
// minimum and a maximum of integers: the order of the jobs does not show.  (The device does the same with atomics, cvx_pair_contacts.hip.)
CVX_HD inline void PairColumnDone(const PairColumnSums &S, uint64_t ySum, int32_t cx, int32_t cz, cvxp_pair_result *r)
{
	if (S.overlap == 0) { return; }
	r->overlap += S.overlap;
	r->points += S.points;
	r->sum[0] += (uint64_t)S.overlap * (uint64_t)((int64_t)cx - r->origin[0]);
	r->sum[1] += ySum;
	r->sum[2] += (uint64_t)S.overlap * (uint64_t)((int64_t)cz - r->origin[2]);
	for (int i = 0; i < 3; i++) {
		r->pushA[i] += S.pushA[i];
		r->pushB[i] += S.pushB[i];
	}
	const int32_t lo[3] = { cx, S.yMin, cz }, hi[3] = { cx, S.yMax, cz };
	for (int i = 0; i < 3; i++) {
		r->min[i] = lo[i] < r->min[i] ? lo[i] : r->min[i];
		r->max[i] = hi[i] > r->max[i] ? hi[i] : r->max[i];
	}
}

// The pair of job `job`, as a wave finds it: ContactsPairInstance's answer -- the LAST p with prefix[p] <= job -- by a search with 64 probes a
// round, a lane each, instead of one: the range [*lo, *lo + *n) holds the answer and prefix[*lo] <= job; lane l probes entry *lo + l * step,
// step = ceil(n / 64) (PairSearchProbe: -1 beyond the range), `le` is the ballot of prefix[probe] <= job, a run of lanes from lane 0 on because
// the prefix never falls, and the answer lies in the step of the last of them (PairSearchNarrow).  65536 pairs take three rounds of one load
// each where the binary search takes sixteen loads one after the other, and that chain is what a wave of a short column waits for.
CVX_HD inline int32_t PairSearchProbe(int32_t lo, int32_t n, int lane)
{
	const int32_t step = (n + 63) / 64, at = lane * step;
	return at < n ? lo + at : -1;
}
CVX_HD inline void PairSearchNarrow(int32_t *lo, int32_t *n, uint64_t le)
{
	const int32_t step = (*n + 63) / 64, at = (__builtin_popcountll(le) - 1) * step; // (lane 0 is always among them)
	*lo += at;
	*n = *n - at < step ? *n - at : step;
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)

// The argument checks of cvxp_model_contacts[_device], in the order include/cpuvox_gpu_pair_contacts.h lists them; false: the message says what.
// ContactsValidate runs twice: first for models, instances, boxes and maps alone (with results and a list that pass), after the pairs for
// results and the capacity, so that its rules and its messages are written once.
inline bool PairsValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs, int pairCount,
                          const void *results, const void *points, int64_t pointCapacity, char *message, size_t bytes)
{
	if (!ContactsValidate(models, modelCount, instances, instanceCount, 0, message, nullptr, 0, message, bytes)) { return false; } // (`message`: any address but NULL)
	if (!pairs || pairCount < 1 || pairCount > CVXP_MAX_PAIRS) {
		snprintf(message, bytes, "pairs NULL or pairCount %d outside 1 .. %d", pairCount, CVXP_MAX_PAIRS);
		return false;
	}
	for (int p = 0; p < pairCount; p++) {
		const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
		if (a < 0 || a >= instanceCount || b < 0 || b >= instanceCount) {
			snprintf(message, bytes, "pair %d: (%d, %d) has an index outside 0 .. %d", p, a, b, instanceCount - 1);
			return false;
		}
		if (a == b) {
			snprintf(message, bytes, "pair %d: (%d, %d) pairs an instance with itself", p, a, b);
			return false;
		}
	}
	return ContactsValidate(models, modelCount, instances, instanceCount, 0, results, points, pointCapacity, message, bytes);
}

// The (pair, column of X_p) jobs of a call: prefix[p] = the jobs of the pairs before p, prefix[pairCount] (the return value) all of them; -1,
// with prefix unspecified, when they are 2^31 - 1 or more (the scan counts jobs + 1 entries in an int).  A pair whose X_p is empty has no job:
// prefix[p] = prefix[p + 1], and ContactsPairInstance(prefix, pairCount, job) -- the LAST p with prefix[p] <= job -- still finds the pair a job
// belongs to, wherever such pairs lie.  Job prefix[p] + (x - lo.x) * (hi.z - lo.z) + (z - lo.z) is column (x, z) of X_p = [lo, hi).
inline int64_t PairJobs(const cvx_model_instance *instances, const int32_t *pairs, int pairCount, uint32_t *prefix)
{
	int64_t total = 0;
	for (int p = 0; p < pairCount; p++) {
		prefix[p] = (uint32_t)total;
		int32_t lo[3], hi[3];
		if (PairBox(instances[pairs[2 * p]], instances[pairs[2 * p + 1]], lo, hi)) { total += ((int64_t)hi[0] - lo[0]) * ((int64_t)hi[2] - lo[2]); }
		if (total >= ((int64_t)1 << 31) - 1) { return -1; }
	}
	prefix[pairCount] = (uint32_t)total;
	return total;
}

// cvxp_box_pairs: a sweep along x.  The instances in the order of their widened boxMin.x; each is tested against those that follow it while
// their boxMin.x lies below its boxMax.x; what is found is sorted into the lexicographic order.
constexpr int kBoxPairsMaxMargin = 1 << 20;
inline bool BoxPairs(const cvx_model_instance *instances, int instanceCount, int margin, int32_t *pairs, int64_t pairCapacity, int64_t *found)
{
	if ((!instances && instanceCount > 0) || instanceCount < 0 || margin < 0 || margin > kBoxPairsMaxMargin || !found || pairCapacity < 0 || (pairCapacity > 0 && !pairs)) {
		return false;
	}
	std::vector<int32_t> order((size_t)instanceCount);
	for (int k = 0; k < instanceCount; k++) { order[(size_t)k] = k; }
	std::sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return instances[p].boxMin[0] < instances[q].boxMin[0] || (instances[p].boxMin[0] == instances[q].boxMin[0] && p < q); });
	const int64_t widen = 2 * (int64_t)margin; // [min - m, max + m) and [min' - m, max' + m) intersect iff min - max' < 2 m and min' - max < 2 m
	std::vector<std::pair<int32_t, int32_t>> all;
	for (int i = 0; i < instanceCount; i++) {
		const cvx_model_instance &P = instances[order[(size_t)i]];
		for (int j = i + 1; j < instanceCount; j++) {
			const cvx_model_instance &Q = instances[order[(size_t)j]];
			if ((int64_t)Q.boxMin[0] - P.boxMax[0] >= widen) { break; } // (and so for every later one)
			bool meet = true;
			for (int a = 0; a < 3; a++) { meet = meet && (int64_t)Q.boxMin[a] - P.boxMax[a] < widen && (int64_t)P.boxMin[a] - Q.boxMax[a] < widen; }
			if (meet) { all.emplace_back(std::min(order[(size_t)i], order[(size_t)j]), std::max(order[(size_t)i], order[(size_t)j])); }
		}
	}
	std::sort(all.begin(), all.end());
	*found = (int64_t)all.size();
	for (int64_t k = 0; k < *found && k < pairCapacity; k++) {
		pairs[2 * k] = all[(size_t)k].first;
		pairs[2 * k + 1] = all[(size_t)k].second;
	}
	return true;
}

// cvxp_pair_response: ContactResponse on the pair's overlap, sums and origin with pushA (which = 0) or pushB (1) as the normal.
inline bool PairResponse(const cvxp_pair_result *r, int which, double centre[3], double normal[3], double *depth)
{
	if (!r || (which != 0 && which != 1)) { return false; }
	cvxc_contact_result c{};
	c.overlap = r->overlap;
	for (int i = 0; i < 3; i++) {
		c.sum[i] = r->sum[i];
		c.origin[i] = r->origin[i];
		c.normal[i] = which == 0 ? r->pushA[i] : r->pushB[i];
	}
	return ContactResponse(&c, centre, normal, depth);
}

} // namespace cvxb
