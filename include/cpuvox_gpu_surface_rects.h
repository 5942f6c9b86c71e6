/* cpuvox_gpu_surface_rects.h -- the exposed faces of the uploaded world merged into rectangles: three entry points of libcpuvox_gpu.so (the
 * product library exports them like those of include/cpuvox_gpu.h; they are declared here, in a header of their own that includes it, so that
 * the list of include/cpuvox_gpu.h stays what its hosts were built against).  Error codes, cvx_context, cvx_mesh_vertex and cvx_last_error
 * are include/cpuvox_gpu.h's. */
#ifndef CPUVOX_GPU_SURFACE_RECTS_H
#define CPUVOX_GPU_SURFACE_RECTS_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*  * cvx_world_surface_rects: cvx_world_surface's quads merged across columns -- a floor is one rectangle, not one quad per voxel, a wall one
 * rectangle, not one strip per column: a list a physics engine's mesh collider or a flat-shaded preview can take.  The rule is defined on top of
 * cvx_world_surface, exact integers in LOD-0 voxels of the stored tile; the call only reads the arena.
 *   Strips.  The items to start from are exactly the quads cvx_world_surface returns for the same box, solidOutside and flags: a quad is an
 *     item with the same voxel and size = {1, length, 1}.  summary.strips is that call's quads, summary.unitFaces its unitFaces.
 *   A merge pass along axis a.  Item q FOLLOWS item p when they have the same face, the same size and the same voxel on the two axes other than
 *     a, q.voxel[a] == p.voxel[a] + p.size[a], and the same argb unless CVX_SURFACE_IGNORE_COLOUR is set.  Items are disjoint, so an item has at
 *     most one follower and follows at most one item: the relation forms chains.  Every maximal chain becomes one item: voxel and argb are those
 *     of the chain's first item, size[a] is the sum over the chain.
 *   Passes.  Faces 0 and 1 (-X, +X): one pass along z.  Faces 4 and 5 (-Z, +Z): one pass along x.  Faces 2 and 3 (-Y, +Y): a pass along x, which
 *     gives rows, then a pass along z over the rows: rows with the same start and the same length stack into rectangles.  There is no length
 *     limit: a wall as long as the world is one rectangle.
 *   What follows.  The unit faces of the rectangles are exactly the unit faces of the strips, each once.  No two rectangles of one face that lie
 *     in one plane and carry one colour (any colour, with CVX_SURFACE_IGNORE_COLOUR) share a whole edge.  Rectangles end at the faces of the
 *     clipped box: as with cvx_world_surface the faces of adjacent boxes tile, none missing and none twice, and no rectangle crosses the seam.
 *     This is not a minimum cover (an L-shaped floor gives two rectangles, and which of them takes the shared rows is the rule's choice), and
 *     colours are merged only by CVX_SURFACE_IGNORE_COLOUR, with which a rectangle carries the colour of its first strip's top voxel.
 *   Order.  Ascending voxel[0], then voxel[2], then face, then DESCENDING voxel[1] + size[1]: the order of the chains' first strips in
 *     cvx_world_surface's list.  The list is a function of the world and the arguments: the same call twice gives the same bytes.
 * `summary` (may be NULL): the rectangles, the strips and unit faces they were made of, and the rectangles per face, whatever the capacity.
 * `rects` receives the first min(rectCapacity, summary.rects) rectangles; a smaller capacity is not an error, and capacity 0 with rects NULL is
 * the way to ask for the count.  outDeviceMs (may be NULL): device time of the call.
 * Ordering as cvx_world_surface: both calls are ordered on the context's stream behind everything enqueued before them, place unplaced levels
 * first and return when the results are on the host.  cvx_world_surface_rects_device leaves the rectangles in rectsDevice (device memory of
 * rectCapacity entries; entries at and beyond min(rectCapacity, summary.rects) are not written); the summary still comes to the host and the
 * call still waits for it.
 * cvx_surface_rect_triangles is a pure host function (no context, no device): four vertices and six indices per rectangle, rectangle k's
 * vertices 4k .. 4k+3 indexed 0,1,2, 0,2,3.  The corners are those of the rectangle on its face plane -- the low side of the voxels for faces
 * 0, 2, 4, the high side for 1, 3, 5 -- in cvx_surface_triangles' order, (v1 - v0) x (v2 - v0) along the face's outward axis: a rectangle that
 * is a single strip gives exactly the vertices cvx_surface_triangles gives for that quad.  rgba, uv and material as there.  A merged mesh has
 * T-junctions (a long rectangle's edge runs past the corners of its shorter neighbours): fine for collision and for flat-shaded drawing, visible
 * as pin holes only where a rasteriser interpolates along such an edge.  CVX_ERR_INVALID_ARGUMENT: a negative count, a NULL pointer with a count
 * above 0, 2^29 or more rectangles, a face outside 0 .. 5, a size below 1, a size other than 1 on the face's normal axis.
 * Errors of the two world calls, all checked on the host before anything is enqueued, cvx_world_surface's.  CVX_ERR_INVALID_ARGUMENT: a NULL
 * box, boxMin >= boxMax on an axis, a box wholly outside the world, solidOutside bits above 0x3F, unknown flag bits, a negative capacity, rects
 * NULL with a capacity above 0; CVX_ERR_NOT_READY: LOD 0 has not been uploaded; CVX_ERR_CAPACITY: the scratch does not fit in device memory,
 * or the box holds 2^31 or more (column, face) pairs or strips.
 * Device memory while it runs: 48 bytes per column of the clipped box (a strip count and a rectangle count per face), 16 bytes per 4096
 * (column, face) pairs for the two scans and 20 bytes per strip (its bottom, length, colour and the two extents the passes give it);
 * cvx_world_surface_rects adds 32 bytes per rectangle it returns.  The strips themselves are never listed for the caller. */
typedef struct cvx_surface_rect {   /* 32 bytes */
	int32_t voxel[3];   /* the rectangle's lowest voxel (min x, min y, min z) */
	int32_t size[3];    /* extent in voxels per axis; 1 along the face's normal axis */
	int32_t face;       /* 0..5 = -X,+X,-Y,+Y,-Z,+Z, as cvx_world_surface */
	uint32_t argb;      /* the colour word of the chain's first strip */
} cvx_surface_rect;
typedef struct cvx_surface_rects_summary {  /* 72 bytes */
	int64_t rects;            /* total rectangles */
	int64_t strips;           /* cvx_world_surface's quads for the same call: what was merged */
	int64_t unitFaces;        /* the exposed voxel faces: the sum of the rectangles' areas */
	int64_t rectsPerFace[6];
} cvx_surface_rects_summary;
int cvx_world_surface_rects(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags,
                            cvx_surface_rect *rects, int64_t rectCapacity, cvx_surface_rects_summary *summary, float *outDeviceMs);
int cvx_world_surface_rects_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags,
                                   cvx_surface_rect *rectsDevice, int64_t rectCapacity, cvx_surface_rects_summary *summary, float *outDeviceMs);
int cvx_surface_rect_triangles(const cvx_surface_rect *rects, int64_t rectCount, cvx_mesh_vertex *vertices, int32_t *indices);

#ifdef __cplusplus
}
#endif
#endif
