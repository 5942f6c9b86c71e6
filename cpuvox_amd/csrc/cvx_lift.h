// cvx_lift.h -- the rules of cvx_world_lift_pieces (cvx_lift.hip): the floating pieces of the device-resident world as models with mass moments.
//
// Written once for the device AND the host (tests/test_world_lift_cpu.py compiles it with g++ through tests/lift_rules.cpp and compares it with
// brute-force sums, Python integers modulo 2^64 and numpy's ravel order):
//   LiftVolume    the elements of a piece's bounding box
//   LiftPlan      which listed pieces are stored and where: the longest prefix whose volumes fit the capacity
//   LiftElement   the index of a voxel in a piece's box, cvx_world_read_voxels' layout: (X, Z, Y), y fastest
//   LiftNodeSums  the nine sums of one node (x, z, [lo, hi)) in closed form: no loop over its voxels
//   LiftMass      cvx_lifted_piece_mass: centre and inertia from the sums, in the order include/cpuvox_gpu_lift.h writes out
// Everything is 64-bit integers; the sums are unsigned and wrap modulo 2^64, as the contract says.
#pragma once

#include <stdint.h>

#include "cpuvox_gpu_lift.h"
#include "cvx_edit.h" // CVX_HD

namespace cvxb {

CVX_HD inline int64_t LiftVolume(const int32_t mn[3], const int32_t mx[3])
{
	return ((int64_t)mx[0] - mn[0]) * ((int64_t)mx[1] - mn[1]) * ((int64_t)mx[2] - mn[2]);
}

struct LiftStored {
	int64_t pieces, voxels;
};

// offsets[i] for the `listed` pieces of `list` (stride in bytes: cvx_piece or cvx_lifted_piece arrays): the sum of the volumes before a stored
// piece, -1 from the first piece that no longer fits on.  (capacity >= 0; no sum overflows: a piece is stored only if it fits what is left.)
CVX_HD inline LiftStored LiftPlan(const void *list, size_t stride, int64_t listed, int64_t capacity, int64_t *offsets)
{
	LiftStored s{ 0, 0 };
	bool open = true;
	for (int64_t i = 0; i < listed; i++) {
		const cvx_piece &p = *reinterpret_cast<const cvx_piece *>(static_cast<const char *>(list) + (size_t)i * stride);
		const int64_t volume = LiftVolume(p.min, p.max);
		open = open && volume <= capacity - s.voxels;
		offsets[i] = open ? s.voxels : -1;
		if (open) {
			s.pieces++;
			s.voxels += volume;
		}
	}
	return s;
}

// voxel p (relative to the box's min) of a box with sizeY x sizeZ voxels per X slab
CVX_HD inline int64_t LiftElement(int64_t px, int64_t py, int64_t pz, int64_t sizeY, int64_t sizeZ) { return (px * sizeZ + pz) * sizeY + py; }

// sum of y over [lo, hi): n (lo + hi - 1) / 2; exactly one of the two factors is even (lo + hi - 1 = n + 2 lo - 1) and is halved first
CVX_HD inline uint64_t LiftSumY(uint64_t lo, uint64_t hi)
{
	const uint64_t n = hi - lo, m = lo + hi - 1u;
	return (n & 1u) ? n * (m >> 1) : (n >> 1) * m;
}
// sum of y^2 over [0, k): the square-pyramidal number (k - 1) k (2 k - 1) / 6, for k < 2^21 (nothing wraps before the division)
CVX_HD inline uint64_t LiftSquaresBelow(uint64_t k) { return k == 0u ? 0u : (k - 1u) * k * (2u * k - 1u) / 6u; }

// out[0 .. 2] = sum, out[3 .. 8] = moment of the voxels (px, y, pz), lo <= y < hi, all relative to the piece's min
CVX_HD inline void LiftNodeSums(uint64_t px, uint64_t pz, uint64_t lo, uint64_t hi, uint64_t out[9])
{
	const uint64_t n = hi - lo, sy = LiftSumY(lo, hi), syy = LiftSquaresBelow(hi) - LiftSquaresBelow(lo);
	out[0] = n * px;
	out[1] = sy;
	out[2] = n * pz;
	out[3] = n * px * px;
	out[4] = syy;
	out[5] = n * pz * pz;
	out[6] = px * sy;
	out[7] = sy * pz;
	out[8] = n * pz * px;
}

// cvx_lifted_piece_mass behind its argument check (voxels > 0); the order is the header's
inline void LiftMass(const cvx_lifted_piece &p, double centre[3], double inertia[6])
{
	const double n = (double)p.piece.voxels;
	double s[3], c[3], q[3];
	for (int a = 0; a < 3; a++) {
		s[a] = (double)p.sum[a];
		c[a] = s[a] / n;
		const double sc = s[a] * c[a];
		q[a] = (double)p.moment[a] - sc;
		if (centre) { centre[a] = ((double)p.piece.min[a] + c[a]) + 0.5; }
	}
	if (!inertia) { return; }
	const double own = n / 3.0;
	inertia[0] = (q[1] + q[2]) + own;
	inertia[1] = (q[2] + q[0]) + own;
	inertia[2] = (q[0] + q[1]) + own;
	for (int k = 0; k < 3; k++) { // (x, y), (y, z), (z, x)
		const double sc = s[k] * c[(k + 1) % 3];
		inertia[3 + k] = -((double)p.moment[3 + k] - sc);
	}
}

} // namespace cvxb
