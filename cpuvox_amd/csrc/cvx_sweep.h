// cvx_sweep.h -- the rules of cvxs_world_sweep / cvxs_sweep_offset / cvxs_instance_moved (cvx_sweep.hip): how far a placed voxel model can move
// along an integer motion before it touches the device-resident world.
//
// Written once for the device AND the host (tests/test_world_sweep_cpu.py compiles it with g++ through tests/sweep_rules.cpp and compares it
// with the numpy model of tests/sweepmodel.py), on top of cvx_contacts.h (the body, the job of a wave) and cvx_distance.h (the world's column):
//   SweepPathNext      the path as the plain merge loop of the three axes' steps: the specification
//   SweepStepsBefore   the closed form beside it: the steps of another axis taken before the k-th step of an axis
//   SweepInstanceMoved I + o, and whether it stays inside cvx_world_place_models' limits
//   SweepInstance      one instance, a pose at a time through cvxb::ContactsInstance's own overlap: the specification of `hit`
//   SweepStations      the stretches of a path between two horizontal steps (the closed form), 16 bytes each
//   SweepFirstSolid    the least m in 0 .. count for which a column is solid at y0 + sign * m: one binary search of the column's runs
//   SweepLane          what a lane of cvx_sweep.hip's wave gives for its voxel of a (instance, column, station) job
//   the host side      SweepValidate (the argument checks), SweepJobs (the prefix of the jobs) and SweepResultOf
// Nothing is float.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_sweep.h"
#include "cvx_contacts.h"
#include "cvx_distance.h"

namespace cvxb {

constexpr uint32_t kSweepNone = 0xFFFFFFFFu; // first[k] while no pose of instance k is known to touch

CVX_HD inline int64_t SweepAbs(int64_t v) { return v < 0 ? -v : v; }
CVX_HD inline int32_t SweepSign(int64_t v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }

// ---- the path -------------------------------------------------------------------------------------------------------------------------------------
// taken[a]: the steps of axis a taken so far.  The next step is the one with the least parameter (2 taken[a] + 1) / (2 |v_a|) among the axes
// that have steps left, the lower axis on a tie; fractions compared by cross-multiplying.  Returns its axis (and counts it), -1 at the end.
CVX_HD inline int SweepPathNext(const int32_t motion[3], int32_t taken[3])
{
	int best = -1;
	for (int a = 0; a < 3; a++) {
		const int64_t n = SweepAbs(motion[a]);
		if (taken[a] >= n) { continue; }
		if (best < 0) {
			best = a;
			continue;
		}
		// (2 taken[a] + 1) / (2 n) < (2 taken[best] + 1) / (2 nBest); a > best, so a tie stays with `best`
		const int64_t nBest = SweepAbs(motion[best]);
		if ((2 * (int64_t)taken[a] + 1) * nBest < (2 * (int64_t)taken[best] + 1) * n) { best = a; }
	}
	if (best >= 0) { taken[best]++; }
	return best;
}

CVX_HD inline int64_t SweepSteps(const int32_t motion[3]) { return SweepAbs(motion[0]) + SweepAbs(motion[1]) + SweepAbs(motion[2]); }

// o_j and the axis of step j by the merge loop; false for j outside 0 .. n.
CVX_HD inline bool SweepOffset(const int32_t motion[3], int64_t j, int32_t offset[3], int *axis)
{
	if (j < 0 || j > SweepSteps(motion)) { return false; }
	int32_t taken[3] = { 0, 0, 0 };
	int last = -1;
	for (int64_t i = 0; i < j; i++) { last = SweepPathNext(motion, taken); }
	for (int a = 0; a < 3; a++) { offset[a] = SweepSign(motion[a]) * taken[a]; }
	*axis = last;
	return true;
}

// The closed form: how many steps of axis b (nb = |v_b| of them) come before the k-th step (k = 1 .. na) of axis a != b.  Step kb of b comes
// first iff (2 kb - 1) na < (2 k - 1) nb, or <= when b is the lower axis.
CVX_HD inline int64_t SweepStepsBefore(int64_t na, int64_t k, int64_t nb, bool bWinsTies)
{
	if (nb == 0) { return 0; }
	const int64_t p = (2 * k - 1) * nb - (bWinsTies ? 0 : 1); // (2 kb - 1) na <= p, p >= 0
	const int64_t count = (p / na + 1) / 2;
	return count < nb ? count : nb;
}

// The index j (1 .. n) of the k-th step of axis a.
CVX_HD inline int64_t SweepStepIndex(const int32_t motion[3], int a, int64_t k)
{
	int64_t j = k;
	for (int b = 0; b < 3; b++) {
		if (b != a) { j += SweepStepsBefore(SweepAbs(motion[a]), k, SweepAbs(motion[b]), b < a); }
	}
	return j;
}

// o_j and the axis of step j by the closed form: step j is the k-th of axis a for the one (a, k) whose index is j -- k by a binary search, the
// index being monotone in k.
CVX_HD inline bool SweepOffsetClosed(const int32_t motion[3], int64_t j, int32_t offset[3], int *axis)
{
	if (j < 0 || j > SweepSteps(motion)) { return false; }
	*axis = -1;
	for (int a = 0; a < 3; a++) {
		// the steps of axis a among the first j: the greatest k with SweepStepIndex(a, k) <= j
		int64_t lo = 0, hi = SweepAbs(motion[a]);
		while (lo < hi) {
			const int64_t mid = (lo + hi + 1) >> 1;
			if (SweepStepIndex(motion, a, mid) <= j) { lo = mid; } else { hi = mid - 1; }
		}
		offset[a] = SweepSign(motion[a]) * (int32_t)lo;
		if (lo > 0 && SweepStepIndex(motion, a, lo) == j) { *axis = a; }
	}
	return true;
}

// ---- the moved instance ---------------------------------------------------------------------------------------------------------------------------
// I + o: the box shifted, t[i] - m[i] . o.  false (out unspecified) when the result leaves cvx_world_place_models' limits.
CVX_HD inline bool SweepInstanceMoved(const cvx_model_instance &I, const int32_t o[3], cvx_model_instance *out)
{
	*out = I;
	for (int a = 0; a < 3; a++) {
		const int64_t lo = (int64_t)I.boxMin[a] + o[a], hi = (int64_t)I.boxMax[a] + o[a];
		if (lo < -(1 << 30) || lo > (1 << 30) || hi < -(1 << 30) || hi > (1 << 30)) { return false; }
		out->boxMin[a] = (int32_t)lo;
		out->boxMax[a] = (int32_t)hi;
		const cvx_model_map &M = I.toModel; // (|m| <= 2^24, |o| < 2^31, |t| <= 2^46: below 2^57)
		const int64_t t = M.t[a] - ((int64_t)M.m[a][0] * o[0] + (int64_t)M.m[a][1] * o[1] + (int64_t)M.m[a][2] * o[2]);
		if (t < -kModelMapMaxT || t > kModelMapMaxT) { return false; }
		out->toModel.t[a] = t;
	}
	return true;
}

// ---- the rule, a pose at a time -------------------------------------------------------------------------------------------------------------------
// hit of instance I under `motion`: the least j whose pose I + o_j overlaps the world by cvxb::ContactsInstance's own count, -1 when none does.
inline int32_t SweepInstance(const CopyWorld &W, const cvx_model *models, const cvx_model_instance &I, const int32_t motion[3], int solidOutside)
{
	int32_t taken[3] = { 0, 0, 0 };
	for (int64_t j = 0;; j++) {
		const int32_t o[3] = { SweepSign(motion[0]) * taken[0], SweepSign(motion[1]) * taken[1], SweepSign(motion[2]) * taken[2] };
		cvx_model_instance moved;
		cvxc_contact_result r;
		if (!SweepInstanceMoved(I, o, &moved)) { return -2; }
		ContactsInstance(W, models, moved, 0, solidOutside, &r, [](const cvxc_contact_point &) {});
		if (r.overlap > 0) { return (int32_t)j; }
		if (SweepPathNext(motion, taken) < 0) { return -1; }
	}
}

// ---- stations -------------------------------------------------------------------------------------------------------------------------------------
// Station q (0 .. H, H = |vx| + |vz|): the poses from the q-th horizontal step up to the next one.  All of them share (ox, oz); they are
// o_j0, o_(j0 + 1), .. o_(j0 + dyCount), the y offset going from dy0 by the sign of vy a step.
struct SweepStation { // 16 bytes
	int16_t ox, oz;
	int32_t j0, dy0, dyCount;
};

CVX_HD inline int64_t SweepStationCount(const int32_t motion[3]) { return SweepAbs(motion[0]) + SweepAbs(motion[2]) + 1; }

// The stations of a motion by the closed form: the k-th step of x is horizontal step k + (the z steps before it) and has (the y steps before
// it) behind it; z likewise.  out: SweepStationCount(motion) records.
inline void SweepStations(const int32_t motion[3], SweepStation *out)
{
	const int64_t n[3] = { SweepAbs(motion[0]), SweepAbs(motion[1]), SweepAbs(motion[2]) }, H = n[0] + n[2];
	const int32_t sy = SweepSign(motion[1]);
	out[0] = SweepStation{ 0, 0, 0, 0, 0 };
	for (int a = 0; a < 3; a += 2) {
		const int b = 2 - a;
		for (int64_t k = 1; k <= n[a]; k++) {
			const int64_t other = SweepStepsBefore(n[a], k, n[b], b < a), below = SweepStepsBefore(n[a], k, n[1], 1 < a), q = k + other;
			const int64_t along = SweepSign(motion[a]) * k, across = SweepSign(motion[b]) * other;
			out[q] = SweepStation{ (int16_t)(a == 0 ? along : across), (int16_t)(a == 0 ? across : along), (int32_t)(q + below), sy * (int32_t)below, 0 };
		}
	}
	for (int64_t q = 0; q <= H; q++) {
		const int64_t next = q < H ? SweepAbs(out[q + 1].dy0) : n[1];
		out[q].dyCount = (int32_t)(next - SweepAbs(out[q].dy0));
	}
}

// ---- a lane ---------------------------------------------------------------------------------------------------------------------------------------
// The least m in 0 .. count with ContactColumnSolid(c, dimY, y0 + sign * m), -1 when there is none.  The arena's runs are searched once
// (SolidAtOrBelow / SolidAtOrAbove); the half lines below 0 and above dimY are the column's flags.
CVX_HD inline int64_t SweepFirstSolid(const DistanceColumn &c, int64_t dimY, int64_t y0, int32_t sign, int64_t count)
{
	if (c.allSolid) { return 0; }
	if (sign == 0 || count == 0) { return ContactColumnSolid(c, dimY, y0) ? 0 : -1; }
	int64_t m = -1;
	if (sign < 0) {
		if (y0 >= dimY && c.solidAbove) { return 0; }
		if (y0 < 0) { return c.solidBelow ? 0 : -1; }
		const int64_t at = SolidAtOrBelow(c.col, y0 < dimY ? y0 : dimY - 1); // (what lies between dimY - 1 and y0 is air)
		m = at >= 0 ? y0 - at : (c.solidBelow ? y0 + 1 : -1);
	} else {
		if (y0 < 0 && c.solidBelow) { return 0; }
		if (y0 >= dimY) { return c.solidAbove ? 0 : -1; }
		const int64_t at = SolidAtOrAbove(c.col, y0 > 0 ? y0 : 0, dimY);
		m = at < dimY ? at - y0 : (c.solidAbove ? dimY - y0 : -1);
	}
	return m >= 0 && m <= count ? m : -1;
}

// The lane's candidate for first[k]: voxel y of the job's column of the body, the column `c` of the world at (cx + ox, cz + oz).
CVX_HD inline uint32_t SweepLane(const ContactsColumnJob &J, const DistanceColumn &c, int64_t dimY, const SweepStation &S, int32_t signY, int32_t y)
{
	if (!ContactsLaneVoxel(J, y)) { return kSweepNone; }
	const int64_t m = SweepFirstSolid(c, dimY, (int64_t)y + S.dy0, signY, S.dyCount);
	return m < 0 ? kSweepNone : (uint32_t)(S.j0 + (int32_t)m);
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------------------
// (plain host functions: not CVX_HD)

// What the kernel reads of an instance besides the instance itself: where its stations begin, how many they are and the sign of its vy.
struct SweepInstanceJob { // 16 bytes
	uint32_t stationBase;
	int32_t stations, signY, pad_;
};

// The argument checks of cvxs_world_sweep[_device] in the header's order; false: the message says what.
inline bool SweepValidate(const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *motions, int solidOutside,
                          const void *sweeps, const void *contacts, const void *points, int64_t pointCapacity, char *message, size_t bytes)
{
	// (contacts stands where that call has results and may be NULL: any other pointer passes its check)
	if (!ContactsValidate(models, modelCount, instances, instanceCount, solidOutside, contacts ? contacts : message, points, pointCapacity, message, bytes)) { return false; }
	if (!motions || !sweeps) {
		snprintf(message, bytes, "%s is NULL", !motions ? "motions" : "sweeps");
		return false;
	}
	if (!contacts && pointCapacity > 0) {
		snprintf(message, bytes, "pointCapacity %lld without contacts", (long long)pointCapacity);
		return false;
	}
	for (int k = 0; k < instanceCount; k++) {
		const int32_t *v = motions + 3 * (size_t)k;
		for (int a = 0; a < 3; a++) {
			if (v[a] < -CVXS_MAX_MOTION || v[a] > CVXS_MAX_MOTION) {
				snprintf(message, bytes, "instance %d: motion %d on axis %d beyond %d", k, v[a], a, CVXS_MAX_MOTION);
				return false;
			}
		}
		cvx_model_instance moved;
		if (!SweepInstanceMoved(instances[k], v, &moved)) {
			snprintf(message, bytes, "instance %d: moved by (%d, %d, %d) it leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)", k, v[0], v[1], v[2]);
			return false;
		}
	}
	return true;
}

// The (instance, column, station) jobs of a call: prefix[k] = the jobs of the instances before k, prefix[instanceCount] (the return value) all of
// them; -1 when they are 2^31 - 1 or more.  Job prefix[k] + station * footprint + column: station-major, so that neighbouring waves read
// neighbouring columns of the world under one offset.  info[k]: the instance's stations and where they begin among all stations (the second return value).
inline int64_t SweepJobs(const cvx_model_instance *instances, const int32_t *motions, int instanceCount, uint32_t *prefix, SweepInstanceJob *info, int64_t *stations)
{
	int64_t total = 0, base = 0;
	for (int k = 0; k < instanceCount; k++) {
		const int64_t footprint = ((int64_t)instances[k].boxMax[0] - instances[k].boxMin[0]) * ((int64_t)instances[k].boxMax[2] - instances[k].boxMin[2]);
		const int64_t count = SweepStationCount(motions + 3 * (size_t)k);
		prefix[k] = (uint32_t)total;
		info[k] = SweepInstanceJob{ (uint32_t)base, (int32_t)count, SweepSign(motions[3 * (size_t)k + 1]), 0 };
		if (footprint >= ((int64_t)1 << 31) - 1) { return -1; } // (before the product: it could pass 2^63)
		total += footprint * count;
		base += count;
		if (total >= ((int64_t)1 << 31) - 1) { return -1; }
	}
	prefix[instanceCount] = (uint32_t)total;
	*stations = base;
	return total;
}

// The sweep result of an instance from first[k].
inline cvxs_sweep_result SweepResultOf(const int32_t motion[3], uint32_t first)
{
	cvxs_sweep_result r{};
	r.steps = (int32_t)SweepSteps(motion);
	r.hit = first == kSweepNone ? -1 : (int32_t)first;
	r.axis = -1;
	for (int a = 0; a < 3; a++) { r.free[a] = r.at[a] = r.hit < 0 ? motion[a] : 0; }
	if (r.hit > 0) {
		int axis, unused;
		SweepOffsetClosed(motion, r.hit, r.at, &axis);
		SweepOffsetClosed(motion, r.hit - 1, r.free, &unused);
		r.axis = axis;
		r.sign = SweepSign(motion[axis]);
	}
	return r;
}

} // namespace cvxb
