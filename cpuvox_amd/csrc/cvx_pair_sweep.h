// cvx_pair_sweep.h -- the rules of cvxm_pair_sweep (cvx_pair_sweep.hip): how far a placed voxel model can move along an integer motion before it
// touches another placed model.  No world anywhere.
//
// Written once for the device AND the host (tests/test_model_sweep_cpu.py compiles it with g++ through tests/pair_sweep_rules.cpp and compares it
// with the numpy model of tests/pairsweepmodel.py), on top of cvx_sweep.h (the path, its closed forms, the moved instance, the sweep result) and
// cvx_pair_contacts.h (the body, a body's column job, the search of the pairs), whose rules it calls and does not repeat:
//   PairSweepPair        one pair, a pose at a time: SweepPathNext / SweepInstanceMoved and PairOf's overlap of every pose: the specification
//   PairSweepRange       R_c of the header: the coordinates of a's box that can come inside b's on axis c during the motion
//   PairSweepAxisWindow  the poses of a path whose offset on one axis lies in an interval, from SweepStepIndex: the closed form
//   PairSweepTakenAt     the steps taken on every axis at a window's first pose, from SweepStepsBefore
//   PairSweepColumn      a (pair, column of R_x x R_z) job as a wave of cvx_pair_sweep.hip evaluates it.  Body a stays where it is and body b
//                        goes the path backwards: B_(I_a + o) meets B_b iff B_a meets B_(I_b - o).  The lanes are the 64 voxels of a step of
//                        a's column, top down; everything about b and the path is the same in every lane (`U`)
//   the host side        PairSweepValidate (the argument checks), PairSweepJobs (the prefix of the jobs), PairSweepResultOf
// Nothing is float.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_pair_sweep.h"
#include "cvx_pair_contacts.h"
#include "cvx_sweep.h"

namespace cvxb {

// ---- the rule, a pose at a time -------------------------------------------------------------------------------------------------------------------
// hit of pair (A, B) under `motion`: the least j for which A + o_j overlaps B by cvxb::PairOf's own count, -1 when none does (-2: a pose leaves
// the limits, which PairSweepValidate rules out).
inline int32_t PairSweepPair(const cvx_model *models, const cvx_model_instance &A, const cvx_model_instance &B, const int32_t motion[3])
{
	int32_t taken[3] = { 0, 0, 0 };
	for (int64_t j = 0;; j++) {
		const int32_t o[3] = { SweepSign(motion[0]) * taken[0], SweepSign(motion[1]) * taken[1], SweepSign(motion[2]) * taken[2] };
		cvx_model_instance two[2] = { A, B };
		cvxp_pair_result r;
		if (!SweepInstanceMoved(A, o, &two[0])) { return -2; }
		PairOf(models, two, 0, 0, 1, &r, [](const cvxp_pair_point &) {});
		if (r.overlap > 0) { return (int32_t)j; }
		if (SweepPathNext(motion, taken) < 0) { return -1; }
	}
}

// ---- the jobs -------------------------------------------------------------------------------------------------------------------------------------
// R_c = [*lo, *hi) (empty: *lo >= *hi): the u in [aMin, aMax) for which [min(u, u + v), max(u, u + v)] meets [bMin, bMax).
CVX_HD inline void PairSweepRange(int32_t aMin, int32_t aMax, int32_t bMin, int32_t bMax, int32_t v, int64_t *lo, int64_t *hi)
{
	const int64_t from = (int64_t)bMin - (v > 0 ? v : 0), to = (int64_t)bMax - (v < 0 ? v : 0); // u + max(v, 0) >= bMin, u + min(v, 0) < bMax
	*lo = from > aMin ? from : (int64_t)aMin;
	*hi = to < aMax ? to : (int64_t)aMax;
}

// The jobs of a pair: |R_x| * |R_z| if R_y is not empty (0 otherwise); *x0, *z0, *sizeZ: where its columns begin and how they are laid out --
// job x * sizeZ + z is column (*x0 + x, *z0 + z) of a's box.
CVX_HD inline int64_t PairSweepPairJobs(const int32_t aMin[3], const int32_t aMax[3], const int32_t bMin[3], const int32_t bMax[3], const int32_t motion[3], int32_t *x0,
                                        int32_t *z0, uint32_t *sizeZ)
{
	int64_t xLo, xHi, yLo, yHi, zLo, zHi;
	PairSweepRange(aMin[0], aMax[0], bMin[0], bMax[0], motion[0], &xLo, &xHi);
	PairSweepRange(aMin[1], aMax[1], bMin[1], bMax[1], motion[1], &yLo, &yHi);
	PairSweepRange(aMin[2], aMax[2], bMin[2], bMax[2], motion[2], &zLo, &zHi);
	*x0 = (int32_t)xLo;
	*z0 = (int32_t)zLo;
	*sizeZ = zLo < zHi ? (uint32_t)(zHi - zLo) : 0u;
	return xLo < xHi && yLo < yHi && zLo < zHi ? (xHi - xLo) * (zHi - zLo) : 0;
}

// ---- windows of a path ----------------------------------------------------------------------------------------------------------------------------
// The poses j0 .. j1 of a path (none: j0 > j1).  j0 is the pose behind the k-th step of axis c; k = 0: pose 0.
struct PairSweepWindow {
	int64_t j0, j1, k;
	int c;
};

// W cut to the poses j whose offset on axis c lies in [lo, hi].  The offset's magnitude is the steps taken of the axis, which never fall along
// the path: "at least k steps of axis c are taken" is j >= SweepStepIndex(motion, c, k).  (c is a constant at every call: no array is addressed
// by a variable.)
CVX_HD inline void PairSweepAxisWindow(const int32_t motion[3], int c, int64_t lo, int64_t hi, PairSweepWindow *W)
{
	const int64_t n = SweepAbs(motion[c]);
	int64_t kLo = motion[c] >= 0 ? lo : -hi, kHi = motion[c] >= 0 ? hi : -lo; // the same interval in steps taken
	kLo = kLo > 0 ? kLo : 0;
	kHi = kHi < n ? kHi : n;
	if (kLo > kHi) {
		W->j1 = W->j0 - 1;
		return;
	}
	const int64_t from = kLo == 0 ? 0 : SweepStepIndex(motion, c, kLo), to = kHi == n ? SweepSteps(motion) : SweepStepIndex(motion, c, kHi + 1) - 1;
	if (from > W->j0) {
		W->j0 = from;
		W->k = kLo;
		W->c = c;
	}
	W->j1 = to < W->j1 ? to : W->j1;
}

// taken[] at pose W.j0: the k steps of axis c, and of every other axis those that come before the k-th of c.
CVX_HD inline void PairSweepTakenAt(const int32_t motion[3], const PairSweepWindow &W, int32_t taken[3])
{
	taken[0] = taken[1] = taken[2] = 0;
	if (W.k == 0) { return; }
	const int64_t n0 = SweepAbs(motion[0]), n1 = SweepAbs(motion[1]), n2 = SweepAbs(motion[2]);
	if (W.c == 0) {
		taken[0] = (int32_t)W.k;
		taken[1] = (int32_t)SweepStepsBefore(n0, W.k, n1, false);
		taken[2] = (int32_t)SweepStepsBefore(n0, W.k, n2, false);
	} else if (W.c == 1) {
		taken[0] = (int32_t)SweepStepsBefore(n1, W.k, n0, true);
		taken[1] = (int32_t)W.k;
		taken[2] = (int32_t)SweepStepsBefore(n1, W.k, n2, false);
	} else {
		taken[0] = (int32_t)SweepStepsBefore(n2, W.k, n0, true);
		taken[1] = (int32_t)SweepStepsBefore(n2, W.k, n1, true);
		taken[2] = (int32_t)W.k;
	}
}

// ---- the wave's form ------------------------------------------------------------------------------------------------------------------------------
// Body b's column job after body b has gone by (-dx, -dy, -dz): what SweepInstanceMoved does to an instance, done to the job.  The column part
// is linear in the voxel (exact in int64) and the y range shifts with the box.  Every operand is on the scalar side.
CVX_HD inline void PairSweepBodyBack(PairBodyJob &B, int64_t dx, int64_t dy, int64_t dz)
{
	B.J.part[0] += 2 * (dx * B.m0[0] + dy * B.J.m1[0] + dz * B.m2[0]);
	B.J.part[1] += 2 * (dx * B.m0[1] + dy * B.J.m1[1] + dz * B.m2[1]);
	B.J.part[2] += 2 * (dx * B.m0[2] + dy * B.J.m1[2] + dz * B.m2[2]);
	B.J.yLo -= (int32_t)dy;
	B.J.yHi -= (int32_t)dy;
}

// The lanes of a wave.  Body(J, yTop, among): the ballot, over the lanes l of `among`, of ContactsLaneVoxel(J, yTop - l).  On the device a
// lane evaluates its own voxel and the wave ballots (cvx_pair_sweep.hip); on the host the 64 lanes are run one after the other:
struct PairSweepLanesInTurn {
	uint64_t Body(const ContactsColumnJob &J, int32_t yTop, uint64_t among) const
	{
		uint64_t mask = 0ull;
		for (int lane = 0; lane < 64; lane++) {
			if (((among >> lane) & 1ull) != 0ull && ContactsLaneVoxel(J, yTop - lane)) { mask |= 1ull << lane; }
		}
		return mask;
	}
};

// The job's candidate for first[p]: column (cx, cz) of a's box.  kSweepNone when no pose of the column touches.
//   - across: the poses at which the column lies inside b's box on x and z, once for the job
//   - per step of 64 voxels of a's column: the ballot of a's body, the poses at which the step's highest and lowest body voxel can lie inside
//     b's y range, cut below the best pose so far; b's job at the window's first pose by the closed form; then a counted walk of the window, b
//     going the path backwards a step a pose, one ballot a pose, ending at the first pose with a set bit
template <class Uniform, class Lanes>
CVX_HD inline uint32_t PairSweepColumn(const Uniform &U, const Lanes &L, const cvx_model *models, const cvx_model_instance &Ia, const cvx_model_instance &Ib,
                                       const int32_t motion[3], int32_t cx, int32_t cz)
{
	const ContactsColumnJob Ja = ContactsColumnJobOf(U, models, Ia, cx, cz);
	const PairBodyJob Jb = PairBodyJobOf(U, models, Ib, cx, cz);
	const int32_t sign0 = SweepSign(motion[0]), sign1 = SweepSign(motion[1]), sign2 = SweepSign(motion[2]);
	PairSweepWindow across{ 0, SweepSteps(motion), 0, 0 };
	PairSweepAxisWindow(motion, 0, (int64_t)Jb.x0 - cx, (int64_t)Jb.x1 - 1 - cx, &across);
	PairSweepAxisWindow(motion, 2, (int64_t)Jb.z0 - cz, (int64_t)Jb.z1 - 1 - cz, &across);
	uint32_t best = kSweepNone;
	if (across.j0 > across.j1) { return best; }
	int32_t top, low;
	ContactsStepRange(Ja, &top, &low);
	for (int32_t yTop = top; yTop >= low; yTop -= 64) {
		const uint64_t body = L.Body(Ja, yTop, ~0ull);
		if (body == 0ull) { continue; }
		const int64_t highest = (int64_t)yTop - __builtin_ctzll(body), lowest = (int64_t)yTop - (63 - __builtin_clzll(body));
		PairSweepWindow W = across;
		if (best != kSweepNone && (int64_t)best - 1 < W.j1) { W.j1 = (int64_t)best - 1; }
		PairSweepAxisWindow(motion, 1, (int64_t)Jb.J.yLo - highest, (int64_t)Jb.J.yHi - 1 - lowest, &W);
		if (W.j0 > W.j1) { continue; }
		int32_t taken[3];
		PairSweepTakenAt(motion, W, taken);
		PairBodyJob at = Jb;
		PairSweepBodyBack(at, (int64_t)sign0 * taken[0], (int64_t)sign1 * taken[1], (int64_t)sign2 * taken[2]);
		for (int64_t j = W.j0;; j++) {
			if (L.Body(at.J, yTop, body) != 0ull) {
				best = (uint32_t)j;
				break;
			}
			if (j >= W.j1) { break; }
			const int axis = SweepPathNext(motion, taken); // (never -1: j1 <= n)
			if (axis == 0) {
				PairSweepBodyBack(at, sign0, 0, 0);
			} else if (axis == 1) {
				PairSweepBodyBack(at, 0, sign1, 0);
			} else {
				PairSweepBodyBack(at, 0, 0, sign2);
			}
		}
	}
	return best;
}

// A job of a call: its pair's instances and motion and its column, then PairSweepColumn.  (The device finds p with PairSearchProbe / Narrow.)
template <class Uniform, class Lanes>
CVX_HD inline uint32_t PairSweepJob(const Uniform &U, const Lanes &L, const cvx_model *models, const cvx_model_instance *instances, const int32_t *pairs,
                                    const int32_t *motions, int32_t p, uint32_t column)
{
	const cvx_model_instance &Ia = instances[U(pairs[2 * p])], &Ib = instances[U(pairs[2 * p + 1])];
	const int32_t motion[3] = { U(motions[3 * p]), U(motions[3 * p + 1]), U(motions[3 * p + 2]) };
	const int32_t aMin[3] = { U(Ia.boxMin[0]), U(Ia.boxMin[1]), U(Ia.boxMin[2]) }, aMax[3] = { U(Ia.boxMax[0]), U(Ia.boxMax[1]), U(Ia.boxMax[2]) };
	const int32_t bMin[3] = { U(Ib.boxMin[0]), U(Ib.boxMin[1]), U(Ib.boxMin[2]) }, bMax[3] = { U(Ib.boxMax[0]), U(Ib.boxMax[1]), U(Ib.boxMax[2]) };
	int32_t x0, z0;
	uint32_t sizeZ;
	PairSweepPairJobs(aMin, aMax, bMin, bMax, motion, &x0, &z0, &sizeZ); // (not 0: the pair has this job)
	return PairSweepColumn(U, L, models, Ia, Ib, motion, x0 + (int32_t)(column / sizeZ), z0 + (int32_t)(column % sizeZ));
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)

// The argument checks of cvxm_pair_sweep[_device] in the header's order; false: the message says what.
inline bool PairSweepValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs, const int32_t *motions,
                              int pairCount, const void *sweeps, char *message, size_t bytes)
{
	// (no results and no list of that call's: any address but NULL passes its check of results)
	if (!PairsValidate(models, modelCount, instances, instanceCount, pairs, pairCount, message, nullptr, 0, message, bytes)) { return false; }
	if (!motions || !sweeps) {
		snprintf(message, bytes, "%s is NULL", !motions ? "motions" : "sweeps");
		return false;
	}
	for (int p = 0; p < pairCount; p++) {
		const int32_t *v = motions + 3 * (size_t)p;
		for (int a = 0; a < 3; a++) {
			if (v[a] < -CVXS_MAX_MOTION || v[a] > CVXS_MAX_MOTION) {
				snprintf(message, bytes, "pair %d: motion %d on axis %d beyond %d", p, v[a], a, CVXS_MAX_MOTION);
				return false;
			}
		}
		cvx_model_instance moved;
		if (!SweepInstanceMoved(instances[pairs[2 * p]], v, &moved)) {
			snprintf(message, bytes, "pair %d: instance %d moved by (%d, %d, %d) leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)", p, pairs[2 * p], v[0], v[1],
			         v[2]);
			return false;
		}
	}
	return true;
}

// The (pair, column) jobs of a call: prefix[p] = the jobs of the pairs before p, prefix[pairCount] (the return value) all of them; -1, with
// prefix unspecified, when they are 2^31 - 1 or more.  A pair without jobs has prefix[p] = prefix[p + 1] and is never landed on by the search
// for the LAST p with prefix[p] <= job.
inline int64_t PairSweepJobs(const cvx_model_instance *instances, const int32_t *pairs, const int32_t *motions, int pairCount, uint32_t *prefix)
{
	int64_t total = 0;
	for (int p = 0; p < pairCount; p++) {
		prefix[p] = (uint32_t)total;
		const cvx_model_instance &A = instances[pairs[2 * p]], &B = instances[pairs[2 * p + 1]];
		int32_t x0, z0;
		uint32_t sizeZ;
		total += PairSweepPairJobs(A.boxMin, A.boxMax, B.boxMin, B.boxMax, motions + 3 * (size_t)p, &x0, &z0, &sizeZ); // (a footprint is below 2^62)
		if (total >= ((int64_t)1 << 31) - 1) { return -1; }
	}
	prefix[pairCount] = (uint32_t)total;
	return total;
}

// The result of pair (a, b) from first[p].
inline cvxm_pair_sweep_result PairSweepResultOf(const int32_t motion[3], uint32_t first, int32_t a, int32_t b)
{
	return cvxm_pair_sweep_result{ SweepResultOf(motion, first), a, b };
}

} // namespace cvxb
