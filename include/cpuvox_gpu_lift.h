/* cpuvox_gpu_lift.h -- the floating pieces of the uploaded world handed out as voxel models with their mass moments: three entry points of
 * libcpuvox_gpu.so (the product library exports them like those of include/cpuvox_gpu.h; they are declared here, in a header of their own that
 * includes it, so that the list of include/cpuvox_gpu.h stays what its hosts were built against).  Error codes, cvx_context, cvx_piece,
 * cvx_pieces_summary, the CVX_ANCHOR_* bits and cvx_last_error are include/cpuvox_gpu.h's. */
#ifndef CPUVOX_GPU_LIFT_H
#define CPUVOX_GPU_LIFT_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvx_world_lift_pieces / _device: what a carve has cut loose, each piece as a dense array of its own voxels and the integer sums a host needs
 * for its mass, centre of mass and inertia tensor.  The loop it closes: carve, lift (REMOVE), integrate the rigid bodies on the host (every step cvxc_world_contacts
 * says where a body touches the world and cvxp_model_contacts where two bodies touch each other), per frame
 * cvx_world_snapshot + cvx_world_place_models_device of the lifted arrays + restore, and a last FILL when a body comes to rest.
 *
 * Which pieces.  The floating pieces F_1 .. F_m are exactly the list cvx_world_pieces(..., CVX_PIECES_REPORT, ...) gives for the same box and
 *   anchors: clipping, connectivity, anchor rules, seeds and order are that call's.  pieces[i].piece holds the bytes REPORT gives for F_(i+1).
 *   `pieces` (may be NULL iff pieceCapacity = 0) receives the first min(pieceCapacity, m) of them, the LISTED pieces; a smaller capacity is no
 *   error.  summary (may be NULL): `pieces` as cvx_world_pieces' summary, and the three totals below.
 * Storage.  The volume of F_i is the product of the three extents max - min of its bounding box, in int64.  The STORED pieces are the longest
 *   prefix F_1 .. F_k of the listed ones whose volumes sum to at most voxelCapacity; storedPieces = k, storedVoxels = that sum.  A stored
 *   piece's `offset` is the sum of the volumes of the pieces before it, and its box occupies the elements [offset, offset + volume) of `argb`
 *   and of `solid` (either may be NULL; both only with voxelCapacity = 0; each has room for voxelCapacity elements) in cvx_world_read_voxels'
 *   layout relative to piece.min: voxel v is element
 *       offset + ((v_x - min_x) * (max_z - min_z) + (v_z - min_z)) * (max_y - min_y) + (v_y - min_y)          (X, Z, Y: y fastest)
 *   all in 64 bits.  A voxel of F_i gets its colour word verbatim in `argb` and 1 in `solid`; every other element of the box is 0, solid voxels
 *   of other pieces or of anchored structure inside the box among them.  Elements at and beyond storedVoxels are not written.  A listed piece
 *   that is not stored has offset -1.  A stored piece is a ready cvx_model (include/cpuvox_gpu_models.h): { size = max - min, argb + offset,
 *   solid + offset }; the identity map translated to piece.min puts it back where it was.
 *   neededVoxels = the sum of the volumes of ALL m floating pieces, whatever the capacities: a call with capacities 0 is a REPORT that also
 *   tells how large the pools have to be.
 * Mass properties.  For every listed piece, stored or not, with p = v - piece.min over its voxels v:
 *       sum    = { sum p_x, sum p_y, sum p_z }
 *       moment = { sum p_x^2, sum p_y^2, sum p_z^2, sum p_x p_y, sum p_y p_z, sum p_z p_x }
 *   in unsigned 64-bit arithmetic modulo 2^64: exact whenever voxels * extent^2 < 2^64.  Integer sums have no order: the same world gives the
 *   same bytes, list, summary and pools.
 * Ops.  CVX_LIFT_COPY never changes the world.  CVX_LIFT_REMOVE turns the voxels of the STORED pieces, and only those, into air -- a piece
 *   leaves the world only if the caller now holds it -- through cvx_world_edit's machinery as CVX_PIECES_REMOVE does: the rectangle is the XZ
 *   bounding box of the stored pieces rounded outward to multiples of 2^levelCount and clipped to the world, LOD 1 .. levelCount (0 .. 5) are
 *   rebuilt over it, and columns of it that lose nothing are re-encoded with the builder's rule.  Nothing stored: CVX_OK, nothing changes.
 * Ordering, atomicity and several GPUs as cvx_world_pieces: the call is ordered on the context's stream behind everything enqueued before it
 *   and returns when the list is on the host, so the pools -- device pools too -- are complete at return; every rank makes the same call on its
 *   own context; coordinates address the stored tile.  Every error leaves the world as it was; the list and the summary are written only once
 *   the call can no longer fail; on an error the contents of the pools are unspecified.  outDeviceMs (may be NULL): device time of the
 *   analysis, the lift and, for a REMOVE that removes something, the edit.
 * cvx_world_lift_pieces_device: argbDevice / solidDevice are device pointers (a torch tensor's data_ptr()) on the context's device; list and
 *   summary still come to the host.
 * Errors: cvx_world_pieces' (a NULL box, an empty or outside box, unknown anchors bits, levelCount outside 0 .. 5, a negative pieceCapacity,
 *   pieces NULL with a capacity above 0; CVX_ERR_NOT_READY; CVX_ERR_CAPACITY) and CVX_ERR_INVALID_ARGUMENT for an op that is neither, for
 *   voxelCapacity < 0 and for voxelCapacity > 0 with both pools NULL.
 * Device memory while it runs: cvx_world_pieces' plus an 8-byte offset and 72 bytes of sums per listed piece and, for a REMOVE, 4 bytes per
 *   solid run; cvx_world_lift_pieces stages the pools it was given on the device (5 bytes per stored element). */
enum { CVX_LIFT_COPY = 0, CVX_LIFT_REMOVE = 1 };

typedef struct cvx_lifted_piece { /* 128 bytes */
	cvx_piece piece;     /* the bytes cvx_world_pieces(REPORT) gives for this piece */
	int64_t   offset;    /* first element of its box in the pools; -1: listed but not stored */
	uint64_t  sum[3];    /* sum of p_x, p_y, p_z over its voxels, p = v - piece.min */
	uint64_t  moment[6]; /* sums of p_x^2, p_y^2, p_z^2, p_x p_y, p_y p_z, p_z p_x */
} cvx_lifted_piece;

typedef struct cvx_lift_summary { /* 64 bytes */
	cvx_pieces_summary pieces;          /* 32 bytes, as cvx_world_pieces */
	int64_t storedPieces, storedVoxels; /* pool elements used = sum of the stored boxes' volumes */
	int64_t neededVoxels;               /* sum of the box volumes of ALL floating pieces */
	int64_t pad_;
} cvx_lift_summary;

int cvx_world_lift_pieces(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount,
                          cvx_lifted_piece *pieces, int pieceCapacity, uint32_t *argb, uint8_t *solid, int64_t voxelCapacity,
                          cvx_lift_summary *summary, float *outDeviceMs);
int cvx_world_lift_pieces_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount,
                                 cvx_lifted_piece *pieces, int pieceCapacity, uint32_t *argbDevice, uint8_t *solidDevice, int64_t voxelCapacity,
                                 cvx_lift_summary *summary, float *outDeviceMs);

/* cvx_lifted_piece_mass: mass properties of a listed piece made of unit cubes of unit mass (mass = piece.voxels).  Pure host code: no context,
 * no device.  centre (may be NULL): the centre of mass in world coordinates, a voxel v being the cube [v, v + 1).  inertia (may be NULL):
 * { Ixx, Iyy, Izz, Ixy, Iyz, Izx } about that centre; each diagonal term includes each cube's own 1/6 + 1/6 = 1/3 (n / 3 for the piece: a single
 * voxel gives 1/3, 1/3, 1/3, 0, 0, 0), and the products of inertia are the NEGATIVE sums (the tensor is [[Ixx, Ixy, Izx], [Ixy, Iyy, Iyz],
 * [Izx, Iyz, Izz]]).
 * Computed in double in this order, every operation rounded once (no contraction):
 *     n = (double)voxels;  s_a = (double)sum[a];  m_k = (double)moment[k];  c_a = s_a / n                       a = x, y, z
 *     centre[a] = ((double)min[a] + c_a) + 0.5
 *     q_a = m_a - s_a * c_a                                   (central second moments)
 *     Ixx = (q_y + q_z) + n / 3;  Iyy = (q_z + q_x) + n / 3;  Izz = (q_x + q_y) + n / 3
 *     Ixy = -(m_3 - s_x * c_y);   Iyz = -(m_4 - s_y * c_z);   Izx = -(m_5 - s_z * c_x)
 * CVX_ERR_INVALID_ARGUMENT: p NULL, or voxels <= 0. */
int cvx_lifted_piece_mass(const cvx_lifted_piece *p, double centre[3], double inertia[6]);

#ifdef __cplusplus
}
#endif
#endif
