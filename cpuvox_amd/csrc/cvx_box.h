// cvx_box.h -- what the world calls ask of a caller's box [boxMin, boxMax), written once (host only, no HIP: tests/box_calls_rules.cpp pins every
// text and the order of the checks through the calls that use it).
//
// BoxCheck writes the reason without a prefix; the caller puts its own in front ("<call>: ", "instance 3: ", none) and fails in its own way.  Every box
// must be given and have no empty axis.  What else it must keep is the caller's choice: the calls that clip the box to the world (PiecesClipBox,
// cvx_pieces.h) take any coordinates; the calls that hand out one value per voxel or column of the box as given bound its coordinates and its size.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu.h"

namespace cvxb {

constexpr unsigned kBoxWithin = 1;    // every coordinate lies within +-2^30 (sizes and sums of two coordinates then fit 32 bits)
constexpr unsigned kBoxVoxels = 2;    // fewer than 2^31 voxels
constexpr unsigned kBoxFootprint = 4; // fewer than 2^31 columns
constexpr size_t kBoxMessage = 96;    // bytes that hold every message

// 0, or CVX_ERR_INVALID_ARGUMENT with the reason in `message`.  Per axis, in order: the coordinates' bound, then the empty axis; the sizes last.
inline int BoxCheck(const int32_t boxMin[3], const int32_t boxMax[3], unsigned rules, char *message, size_t size)
{
	if (!boxMin || !boxMax) {
		snprintf(message, size, "a NULL box");
		return CVX_ERR_INVALID_ARGUMENT;
	}
	for (int a = 0; a < 3; a++) {
		if ((rules & kBoxWithin) && (boxMin[a] < -(1 << 30) || boxMin[a] > (1 << 30) || boxMax[a] < -(1 << 30) || boxMax[a] > (1 << 30))) {
			snprintf(message, size, "the box [%d, %d) on axis %d has a coordinate beyond 2^30", boxMin[a], boxMax[a], a);
			return CVX_ERR_INVALID_ARGUMENT;
		}
		if (boxMin[a] >= boxMax[a]) {
			snprintf(message, size, "the box [%d, %d) on axis %d is empty", boxMin[a], boxMax[a], a);
			return CVX_ERR_INVALID_ARGUMENT;
		}
	}
	int64_t n = 1;
	for (int a = 0; a < 3 && (rules & kBoxVoxels); a++) {
		n *= (int64_t)boxMax[a] - boxMin[a]; // (each factor below 2^32, the running product below 2^31 before it: no overflow)
		if (n >= ((int64_t)1 << 31)) {
			snprintf(message, size, "a box of 2^31 or more voxels");
			return CVX_ERR_INVALID_ARGUMENT;
		}
	}
	const int64_t sizeX = (int64_t)boxMax[0] - boxMin[0], sizeZ = (int64_t)boxMax[2] - boxMin[2], limit = (int64_t)1 << 31;
	if ((rules & kBoxFootprint) && (sizeX >= limit || sizeX * sizeZ >= limit)) { // (sizeZ below 2^32, sizeX below 2^31 before it: no overflow)
		snprintf(message, size, "a footprint of 2^31 or more columns");
		return CVX_ERR_INVALID_ARGUMENT;
	}
	return 0;
}

} // namespace cvxb
