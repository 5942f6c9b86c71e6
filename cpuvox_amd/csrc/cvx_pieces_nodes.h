// cvx_pieces_nodes.h -- what cvx_world_pieces (cvx_pieces.hip) and cvx_world_settle (cvx_settle.hip) share: cvxpieces::Analyse checks the arguments
// of the two calls and runs the component engine (cvx_components.h) with the pieces' rule and select kernels; the node tables stay on the device
// for REMOVE and the settle, and are released with the Analysis.
#pragma once

#include "cvx_components.h"

namespace cvxpieces {

struct Totals {
	cvxcomp::TotalsHead head;          // listed: the floating pieces; x0 .. z1: their XZ bounding box
	unsigned long long mostVoxels = 0; // the largest piece
	unsigned int largest = 0xFFFFFFFFu; // ... its root
	unsigned int pad = 0;
	cvx_pieces_summary summary{};
};
static_assert(sizeof(Totals) % 16 == 0, "the list follows the totals");

struct Analysis : cvxcomp::Analysis {
	using cvxcomp::Analysis::Analysis;
	Totals host; // the totals, on the host
};

// `call`: the entry point's name for messages; ctx is not null.  `extraError` (may be null): the message of the call's own argument check (op / maxDrop), reported
// as CVX_ERR_INVALID_ARGUMENT in its place among the shared checks.
int Analyse(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, const char *extraError, int levelCount,
            const cvx_piece *pieces, int pieceCapacity, Analysis *R);

} // namespace cvxpieces
