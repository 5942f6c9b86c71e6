/*
 * cpuvox_gpu.h -- the drop-in boundary: C ABI of libcpuvox_gpu.so.
 *
 * The reference (pipliz/cpuvox) has no FFI for this path: the boundary is the
 * C# static method RenderManager.DrawSegments (Assets/Code/RenderManager.cs:
 * 258-372) which fills SegmentContext[4]/DrawContext, schedules the four
 * Burst jobs of Assets/Code/Rendering/DrawSegmentRayJob.cs and blocks on
 * render.Complete().  Every entry point below cites the reference interface
 * it replaces; INTEGRATION.md shows the P/Invoke binding a maintainer adds.
 *
 * Plain pointers and sizes only; all structs are blittable (C# sequential
 * layout, Pack = 4).  All functions return CVX_OK (0) or a negative error
 * code; cvx_last_error() gives the text.  The reference has no error returns
 * (Burst cannot throw; managed exceptions propagate to UnityManager.cs:184):
 * the P/Invoke wrapper turns a non-zero code into an exception.
 *
 * Threading: one caller thread per context (as the reference: Unity main
 * thread).  cvx_draw_segments is blocking like DrawSegments unless
 * CVX_DRAW_ASYNC is passed.
 *
 * Two kernels stand behind the draw calls and give the same raybuffers bit for
 * bit: the latency kernel for the reference's own call pattern, one blocking
 * frame at a time (one wavefront per ray), and the batch kernel for many
 * frames per launch (one lane per ray); see cvx_set_latency_kernel.
 */
#ifndef CPUVOX_GPU_H
#define CPUVOX_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVX_LOD_LEVELS 6 /* UnityManager.LOD_LEVELS, UnityManager.cs:42 */

enum {
	CVX_OK = 0,
	CVX_ERR_INVALID_ARGUMENT = -1,
	CVX_ERR_HIP = -2,          /* a HIP runtime call failed (no device, OOM, ...) */
	CVX_ERR_NOT_READY = -3,    /* world / resolution not set */
	CVX_ERR_CAPACITY = -4,     /* ray count exceeds the raybuffer capacity */
	CVX_ERR_TIMEOUT = -5,      /* a peer did not arrive in time (cvx_comm_create) */
};

enum {
	CVX_RAYBUFFER_TOPDOWN = 0,   /* RenderManager.rayBufferTopDown,   RenderManager.cs:16,36 */
	CVX_RAYBUFFER_LEFTRIGHT = 1, /* RenderManager.rayBufferLeftRight, RenderManager.cs:17,35 */
};

enum {
	CVX_DRAW_SYNC = 0,  /* return after the kernels completed (render.Complete(), :363) */
	CVX_DRAW_ASYNC = 1, /* enqueue only; cvx_synchronize() or a read-back completes it */
};

/* RenderManager.SegmentData, RenderManager.cs:503-510 (36 bytes). */
typedef struct cvx_segment_data {
	float MinScreen[2];
	float MaxScreen[2];
	float CamLocalPlaneRayMin[2];
	float CamLocalPlaneRayMax[2];
	int32_t RayCount;
} cvx_segment_data;

/* CameraData, CameraData.cs:11-16 (108 bytes).  WorldToScreenMatrix is
 * column major (c0,c1,c2,c3), the memory order of Unity.Mathematics.float4x4.
 * InverseElementIterationDirection is the C# bool (1 byte) + padding. */
typedef struct cvx_camera_data {
	float WorldToScreenMatrix[16];
	float PositionXZ[2];
	float PositionY;
	uint8_t InverseElementIterationDirection;
	uint8_t pad_[3];
	float FarClip;
	float LODDistances[CVX_LOD_LEVELS];
} cvx_camera_data;

/* Work counters of the last draw (optional instrumentation):
 * algorithmic bytes B = 12*S + 4*E + 4*C + 4*P + 80*R. */
typedef struct cvx_counters {
	int64_t S, E, C, P, R;
	int64_t lodVisits[CVX_LOD_LEVELS];
} cvx_counters;

typedef struct cvx_context cvx_context;

/* Lifetime of what RenderManager owns (ctor RenderManager.cs:25-41, Destroy :43-51).
 * device = HIP device ordinal. */
int cvx_create(int device, cvx_context **out);
void cvx_destroy(cvx_context *ctx);
const char *cvx_last_error(const cvx_context *ctx); /* ctx may be NULL: creation errors */

/* Use an externally owned HIP stream (hipStream_t as void*) for all work of
 * this context; NULL = the context's own stream. */
int cvx_set_stream(cvx_context *ctx, void *hipStream);

/*
 * Replaces `new World(dimensions, lod, data)` (World.cs:36-43) + the
 * `fixed (World* worldPtr = worldLODs)` hand-over (RenderManager.cs:155).
 * storage = WorldAllocator.GetStartPointer() (World.cs:273): columnCount
 * 12-byte RLEColumn headers {int32 offset; uint16 runCount, worldMin,
 * worldMax} followed by the 4-byte RLEElement/ColorARGB32 pool
 * (World.cs:161-169,245-259,304-313); byteLength = GetByteLength()
 * (World.cs:278-283), or the exact used length.  columnCount =
 * World.ColumnCount (World.cs:17) = where the element pool starts.
 * The data is copied to the device (and re-laid-out); the caller keeps
 * ownership of storage.  Dimensions must be powers of two (WordBuilder.cs:30),
 * X and Z at most 32768, Y at most 65536 (8192 x 8192 columns already fill the
 * 4 GiB of device tables the 32-bit offsets of the kernel address).
 * Per level: fewer than 2^30 pool entries (CVX_ERR_CAPACITY beyond); on the device the colours are kept in blocks
 * of 4 x 8 columns, each as deep as its tallest column -- ~2.5 x the colours of a terrain, at most 2^29 slots, and a level
 * whose blocks would take more than 4 x its colours keeps them column after column; all levels together within the 4 GiB arena.
 */
int cvx_world_upload(cvx_context *ctx, int lod, const void *storage, int64_t byteLength,
                     int dimX, int dimY, int dimZ, int columnCount);

/* RenderManager.SetResolution, RenderManager.cs:94-109: (re)allocates the
 * raybuffers: top-down = width H, capacity W+2H rays; left-right = width W,
 * capacity 2W+H rays (RenderManager.cs:35-36), times bufferCount. */
int cvx_set_resolution(cvx_context *ctx, int resolutionX, int resolutionY);

/* RenderManager.BUFFER_COUNT (RenderManager.cs:14) is 2; a GPU pipeline that
 * keeps many frames in flight may ask for more.  Call before cvx_set_resolution. */
int cvx_set_buffer_count(cvx_context *ctx, int bufferCount);

/*
 * RenderManager.DrawSegments, RenderManager.cs:258-372: same argument set
 * (segments[4], camera, screen size, vanishing point); worldLODs are the
 * uploaded ones; bufferIndex selects the raybuffer pair (RenderManager.
 * bufferIndex, :19,53-56).  Runs RaySetupJob, DDASetupJob,
 * TraceToFirstColumnJob and RenderJob (DrawSegmentRayJob.cs:12,49,87,156)
 * as HIP kernels.
 */
int cvx_draw_segments(cvx_context *ctx, const cvx_segment_data segments[4], const cvx_camera_data *camera,
                      int screenWidth, int screenHeight, const float vanishingPointScreenSpace[2],
                      int bufferIndex, int flags);

/* Many independent frames in one launch (frame i -> buffer (firstBufferIndex+i) % bufferCount).
 * segments: frameCount*4 entries; cameras, vanishingPoints (x,y pairs): frameCount entries. */
int cvx_draw_segments_batch(cvx_context *ctx, int frameCount, const cvx_segment_data *segments,
                            const cvx_camera_data *cameras, int screenWidth, int screenHeight,
                            const float *vanishingPoints, int firstBufferIndex, int flags);

/*
 * Same as cvx_draw_segments_batch, but the caller chooses where every 64-ray tile is written: tileOut[i] is the device
 * address of pixel row 0 / lane 0 of the i-th tile of the batch (canonical order: frame by frame, segment 0..3, tile
 * 0.. of the segment = ceil(RayCount / 64) tiles each); pixel y of lane l goes to ((uint32_t*)tileOut[i])[y*64 + l] and
 * only rows [origMin, origMax] of the tile's segment are ever written, so a slot needs (origMax - origMin + 1) * 256
 * bytes starting at tileOut[i] + origMin * 256.  tileOut[i] == 0: this context does not render the tile (another GPU
 * does).  Used by the multi-GPU path to render straight into send / display buffers (cpuvox_amd/dist.py); read-back
 * and blit do not apply to placed draws.  tileCount must equal the batch's tile count.
 */
int cvx_draw_segments_placed(cvx_context *ctx, int frameCount, const cvx_segment_data *segments,
                             const cvx_camera_data *cameras, int screenWidth, int screenHeight,
                             const float *vanishingPoints, int64_t tileCount, const uint64_t *tileOut, int flags);

/* Multi-GPU sharding: this context renders only the 64-ray
 * tiles t with t % shardCount == shardIndex.  Default (0, 1) = everything. */
int cvx_set_shard(cvx_context *ctx, int shardIndex, int shardCount);

/* Which kernel a draw goes to.  The reference's caller issues ONE blocking DrawSegments per frame (UnityManager.cs:182, RenderManager.cs:358-363): a
 * few thousand rays, far too few for the batch kernel (one lane per ray).  Such launches go to the latency kernel (one wavefront per RAY, its lanes the
 * ray's next 64 columns: csrc/cvx_lone.h); large batches go to the batch kernel.  Same raybuffers bit for bit either way.
 *   CVX_LATENCY_AUTO (default): the latency kernel for launches of at most ~12 000 rays (~8000 at 4K) whose pixel windows fit its mask (4096 pixels),
 *   CVX_LATENCY_NEVER / CVX_LATENCY_ALWAYS: pin the choice (ALWAYS still falls back to the batch kernel for windows of more than 4096 pixels and while the
 *   work counters are enabled: the counting variant exists for the batch kernel only). */
enum { CVX_LATENCY_AUTO = 0, CVX_LATENCY_NEVER = 1, CVX_LATENCY_ALWAYS = 2 };
int cvx_set_latency_kernel(cvx_context *ctx, int mode);

/* Repeating worlds (the reference's World.REPEAT_WORLD, World.cs:10).  0 (default): bounded -- a ray that starts outside the world is stepped to its box
 * (DrawSegmentRayJob.cs:114-139) and a ray that leaves the box ends with the sky (World.cs:130-142, DrawSegmentRayJob.cs:245-250).  1: the world tiles X and
 * Z endlessly (Y never repeats): the column at (x, z) is the uploaded one at (x & (dimX - 1), z & (dimZ - 1)) (World.cs:132-133) -- two's-complement
 * `&`, a floor-mod, so negative coordinates wrap too --, there is no entry step, and a ray ends only at the far clip or when its pixel window closes.
 * (The reference raises the far clip from 2 x to 10 x the largest dimension in this mode, UnityManager.cs:421-423: cvxh_setup_lods_ex.)
 * Applies per context to every draw (cvx_draw_segments, _batch, _placed) and pick (cvx_world_pick, _device) enqueued after the call; edits, brushes,
 * stamps, read-back and compaction address the stored tile and are unchanged.  In mode 1 a draw or pick returns CVX_ERR_INVALID_ARGUMENT if the world's
 * X or Z dimension is below 32 (2^(LOD levels - 1): wrapping keeps the position bits NextLOD reads, SegmentDDAData.cs:37), a draw if a camera's FarClip is
 * above 2^20, cvx_world_pick if a ray's maxT is above 2^20 (cvx_world_pick_device reports such a ray as a miss).  A pick in mode 1 clips the ray to the
 * Y slab only, reports the hit voxel wrapped into [0, dim) (ready for cvx_world_brush / cvx_world_edit) and t along the ray itself.
 * Any mode other than 0 / 1: CVX_ERR_INVALID_ARGUMENT. */
int cvx_set_world_repeat(cvx_context *ctx, int repeat);

int cvx_synchronize(cvx_context *ctx);

/*
 * Multi-GPU frames behind the C ABI.  The reference's only synchronisation is `render.Complete()` (RenderManager.cs:358-363);
 * sharded over N GPUs (one process and one context per GPU) the equivalent is, per batch of frames:
 *     plan = cvx_shard_plan_create(frames, rank, N)             -- host arithmetic, identical on every rank
 *     cvx_shard_plan_tile_out(plan, sendBase, dispBase, out)    -- where this rank's tiles are rendered
 *     cvx_draw_segments_placed(ctx, ..., out, CVX_DRAW_ASYNC)   -- RaySetupJob .. RenderJob for this rank's tiles
 *     cvx_exchange(ctx, plan, comm, stream, sendBase, dispBase) -- grouped ncclSend / ncclRecv, one pair per peer
 * Tile t of frame b (canonical order: segment 0..3, tiles of a segment in ray order) is rendered by rank t % N; frame b is
 * displayed on rank b % N.  Two areas of 256-byte pixel rows (64 pixels of one tile row) per rank:
 *     send area     my tiles of frames displayed elsewhere, one section per destination rank, (frame, tile) order
 *     display area  all tiles of the frames I display, one section per rendering rank, (frame, tile) order -- my own section
 *                   is written by my kernel, the others arrive from the peers and are exactly their send sections for me
 * Only rows [origMin, origMax] of a tile exist in either area.  sendStart / dispStart: N + 1 section boundaries in rows.
 */
typedef struct cvx_shard_plan cvx_shard_plan;
int cvx_shard_plan_create(int frameCount, const cvx_segment_data *segments, const float *vanishingPoints, int screenWidth, int screenHeight,
                          int rank, int worldSize, cvx_shard_plan **out);
void cvx_shard_plan_destroy(cvx_shard_plan *plan);
int64_t cvx_shard_plan_tile_count(const cvx_shard_plan *plan);
int cvx_shard_plan_sections(const cvx_shard_plan *plan, int64_t *sendStart, int64_t *dispStart);
/* What travels between this rank and `peer` (what cvx_exchange sends and receives; a host with its own transport can use it directly):
 * rows [sendRow, sendRow + sendRows) of the send area go to peer, rows [recvRow, recvRow + recvRows) of the display area come from it. */
int cvx_shard_plan_transfer(const cvx_shard_plan *plan, int peer, int64_t *sendRow, int64_t *sendRows, int64_t *recvRow, int64_t *recvRows);
/* tileOut[i] for cvx_draw_segments_placed (0 = another rank renders tile i); sendBase / dispBase: device addresses of the two areas */
int cvx_shard_plan_tile_out(const cvx_shard_plan *plan, void *sendBase, void *dispBase, uint64_t *tileOut);
/* RCCL communicator owned by the library (librccl is loaded on first use): rank 0 makes the 128-byte id, the host passes it to
 * the other ranks over its own channel, every rank calls cvx_comm_create.  A communicator made elsewhere (ncclComm_t) works too. */
int cvx_comm_unique_id(void *id128);
int cvx_comm_create(cvx_context *ctx, const void *id128, int rank, int worldSize, void **comm);
/* ... with an explicit limit on how long to wait for the peers (cvx_comm_create waits 180 s): CVX_ERR_TIMEOUT when a rank of
 * the clique never arrives -- the sharded `render.Complete()` (RenderManager.cs:363) must not hang for ever on a dead peer.
 * After CVX_ERR_TIMEOUT the helper thread that called ncclCommInitRank is still parked inside RCCL (it cannot be cancelled) and
 * owns a half-made communicator: the process must report the failure and EXIT, not go on using the library. */
int cvx_comm_create_timeout(cvx_context *ctx, const void *id128, int rank, int worldSize, double timeoutSeconds, void **comm);
int cvx_comm_destroy(void *comm);
/* The exchange of one batch on hipStream (NULL = the context's stream): returns after enqueueing; order the consumer with the stream. */
int cvx_exchange(cvx_context *ctx, const cvx_shard_plan *plan, void *comm, void *hipStream, void *sendBase, void *dispBase);

/*
 * The other way of putting a sharded frame together: the IMAGE gather.  Every rank runs Phase 2
 * (RenderManager.BlitSegments, RenderManager.cs:199-256 + RayBufferBlit.shader:48-64) for the pixels whose ray lies in a tile it
 * rendered itself, and the display rank of a frame receives W * H pixels in total instead of the other ranks' raybuffer rows (a
 * raybuffer is ~2x the pixels of the screen it produces).  Per batch of frames:
 *     plan = cvx_image_plan_create(ctx, frames, rank, N)        -- counts pixels per rank on the device (one pass over the images)
 *     cvx_image_plan_tile_out(plan, localStore, out)            -- my tiles go into a compact local store (64 * max(W, H) pixels per tile)
 *     cvx_draw_segments_placed(ctx, ..., out, CVX_DRAW_ASYNC)
 *     cvx_image_pack(ctx, plan, stream, localStore, send, images)    -- my pixels: into the images I display, or my send stream
 *     cvx_image_exchange(ctx, plan, comm, stream, send, recv)        -- one ncclSend + one ncclRecv per peer
 *     cvx_image_unpack(ctx, plan, stream, recv, images)              -- the peers' pixels of the frames I display
 * Frame b is displayed by rank b % N as image b / N of `images` (W * H ARGB32 each, cvx_blit_segments' pixel rule); tile t of a frame
 * is rendered by rank t % N (as in the raybuffer gather).  The stream (src -> dst) holds the frames dst displays in frame order,
 * each with src's pixels in row-major order.  At most 8 ranks.
 */
typedef struct cvx_image_plan cvx_image_plan;
int cvx_image_plan_create(cvx_context *ctx, int frameCount, const cvx_segment_data *segments, const float *vanishingPoints, int screenWidth, int screenHeight,
                          int rank, int worldSize, cvx_image_plan **out);
void cvx_image_plan_destroy(cvx_image_plan *plan);
int64_t cvx_image_plan_tile_count(const cvx_image_plan *plan);
/* bytes of the local tile store, pixels (4 bytes each) of the send and receive streams, number of images this rank displays */
int cvx_image_plan_sizes(const cvx_image_plan *plan, int64_t *localStoreBytes, int64_t *sendPixels, int64_t *recvPixels, int32_t *imagesDisplayed);
int cvx_image_plan_transfer(const cvx_image_plan *plan, int peer, int64_t *sendPixel, int64_t *sendPixels, int64_t *recvPixel, int64_t *recvPixels);
int cvx_image_plan_tile_out(const cvx_image_plan *plan, void *localStore, uint64_t *tileOut);
/* (`images`: imagesDisplayed x H x W pixels; may be NULL on a rank that displays no frame of the batch, imagesDisplayed == 0) */
int cvx_image_pack(cvx_context *ctx, const cvx_image_plan *plan, void *hipStream, const void *localStore, void *sendStream, void *images);
int cvx_image_exchange(cvx_context *ctx, const cvx_image_plan *plan, void *comm, void *hipStream, void *sendStream, void *recvStream);
int cvx_image_unpack(cvx_context *ctx, const cvx_image_plan *plan, void *hipStream, const void *recvStream, void *images);

/* RenderManager.ClearRayBuffer, RenderManager.cs:58-92 (fills with one ARGB32
 * value, bytes A,R,G,B in memory order packed little-endian in `argb`). */
int cvx_clear_raybuffer(cvx_context *ctx, int bufferIndex, int which, uint32_t argb);

/*
 * Read back rows of a raybuffer in the reference's logical layout
 * (RayBuffer.Native.GetRayColumn, RayBuffer.cs:121-128): ray r of the buffer
 * = `width` contiguous ARGB32 pixels, rows [firstRay, firstRay+rayCount).
 * dst is host memory of rayCount*width*4 bytes.  Only rows rendered by the
 * last draw into that buffer are defined (others keep the cleared value).
 */
int cvx_read_raybuffer(cvx_context *ctx, int bufferIndex, int which, int firstRay, int rayCount, void *dst);

/*
 * RenderManager.BlitSegments (RenderManager.cs:199-256) + RayBufferBlit.shader
 * frag (Assets/Shaders/RayBufferBlit.shader:48-64): Phase 2, raybuffer ->
 * W x H ARGB32 screen image (row 0 = bottom row, Unity screen space).  Uses
 * the segments / vanishing point of the last draw into bufferIndex.
 * dstHost may be NULL (image stays on the device, see cvx_screen_device_ptr).
 */
int cvx_blit_segments(cvx_context *ctx, int bufferIndex, void *dstHost);

/*
 * Phase 2 for the frames of a batch in ONE launch: BlitSegments (RenderManager.cs:199-256) of the last draws into buffers
 * firstBufferIndex .. firstBufferIndex + frameCount - 1 (what cvx_draw_segments_batch rendered), image f into
 * dstDevice + f * W * H * 4 bytes (device memory; NULL = an array the context owns, grown on demand).  Asynchronous on
 * the context's stream; *imagesDevice (may be NULL) receives the address of image 0.  Same pixels as frameCount calls of
 * cvx_blit_segments.
 */
int cvx_blit_segments_batch(cvx_context *ctx, int firstBufferIndex, int frameCount, void *dstDevice, void **imagesDevice);

/* Use caller-owned device memory for the raybuffers (e.g. torch tensors that a RCCL collective
 * operates on).  Sizes: bufferCount * tileCapacity * tileBytes per kind (cvx_get_raybuffer_layout),
 * 256-byte aligned.  Buffer b of a kind starts at b * tileCapacity * tileBytes.  The context never
 * frees bound memory; call after cvx_set_resolution (which allocates internal ones). */
int cvx_bind_raybuffers(cvx_context *ctx, void *topDown, int64_t topDownBytes, void *leftRight, int64_t leftRightBytes);

/* Multi-GPU tile exchange helper: copies pixel rows (one row = 64 pixels of a tile = 256 bytes) between the
 * raybuffer pools of this context and a contiguous device staging buffer.  poolRow counts 256-byte rows from the start
 * of the pool (all buffers back to back): ((buffer * tileCapacity + tile) * width + pixelRow).  The span array lives in
 * device memory; hipStream NULL = the context's stream.  toPacked != 0: pool -> staging, else staging -> pool. */
typedef struct cvx_row_span {
	int64_t poolRow;
	int64_t packedRow;
	int32_t rows;
	int32_t kind; /* CVX_RAYBUFFER_TOPDOWN / CVX_RAYBUFFER_LEFTRIGHT */
} cvx_row_span;
int cvx_copy_rows(cvx_context *ctx, void *hipStream, int toPacked, int64_t spanCount, const cvx_row_span *spansDevice, void *packedDevice);

/* Device pointers for zero-copy consumers (RCCL gather, torch tensors). */
int cvx_raybuffer_device_ptr(cvx_context *ctx, int bufferIndex, int which, void **ptr, int64_t *bytes);
int cvx_screen_device_ptr(cvx_context *ctx, void **ptr, int64_t *bytes);

/* Timing of the last draw call, measured with HIP events on the context's
 * stream (milliseconds; kernels only, no host setup). */
int cvx_last_draw_ms(cvx_context *ctx, float *ms);
/* Sum and count of the kernel times of all draws since the last reset (each draw is bracketed by its own
 * HIP event pair on the context's stream; waits for pending draws). */
int cvx_draw_time_stats(cvx_context *ctx, double *totalMs, int *draws, int reset);

/* Enable in-kernel work counters (slower); read them after a SYNC draw. */
int cvx_enable_counters(cvx_context *ctx, int enable);
int cvx_get_counters(cvx_context *ctx, cvx_counters *out);

/* Device layout description of the tile-major raybuffer (for gathers/tests). */
typedef struct cvx_raybuffer_layout {
	int32_t width;         /* pixels per ray: H (top-down) or W (left-right) */
	int32_t rayCapacity;   /* W+2H or 2W+H */
	int32_t tileRays;      /* 64 */
	int32_t tileCapacity;  /* tiles allocated */
	int64_t tileBytes;     /* width * 64 * 4 */
} cvx_raybuffer_layout;
int cvx_get_raybuffer_layout(cvx_context *ctx, int which, cvx_raybuffer_layout *out);

/* World.DownSample(extraLods) (Assets/Code/World.cs:45-127: DownSampleColumn :71-96, DownSamplePartial :101-127, with
 * RLEColumnBuilder.ToFinalColumn WordBuilder.cs:181-268 and the RLEColumn constructor World.cs:190-234) as a device
 * kernel: builds LOD extraLods from the LOD 0 blob (same layout as cvx_world_upload takes; `lod` must be 0 -- the reference only
 * downsamples LOD 0, UnityManager.cs:328-331, other values are refused with CVX_ERR_INVALID_ARGUMENT) and returns the new
 * blob in the reference's storage layout, byte-identical to the host build (columns stored in index order), in memory
 * owned by the library: release it with cvx_free.  outColumnCount = World.ColumnCount of the new level (World.cs:17),
 * outVoxelCount (may be NULL) = voxels after deduplication, outDeviceMs (may be NULL) = device time of the two passes
 * and the offset scan. */
int cvx_world_downsample(cvx_context *ctx, const void *storage, int64_t byteLength, int dimX, int dimY, int dimZ, int lod, int columnCount, int extraLods,
                         void **outStorage, int64_t *outByteLength, int32_t *outColumnCount, int64_t *outVoxelCount, float *outDeviceMs);
/* UnityManager.cs:328-331 (`worldLODs[i] = worldLODs[0].DownSample(i)`): LOD 1..levelCount from the LOD 0 blob with one
 * validation and one upload of it.  outStorage / outByteLength / outColumnCount are arrays of levelCount entries ([i] = LOD i+1);
 * each blob is released with cvx_free.  outDeviceMs (may be NULL) = device time of the whole chain.  LOD 0 is read ONCE: level 1
 * is built from its colours, every further level (up to 7) from the level before it through exact per-voxel sums, which gives the
 * bytes of `DownSample(i)` applied to LOD 0 (integer averages of the LOD-0 voxels, the first inserted voxel's alpha); levels above 7
 * are built from LOD 0 directly like cvx_world_downsample does.  Device memory while it runs: per level 4 bytes x (the elements of the LOD 0
 * columns, counted column by column, + its columns) and two tables of per-voxel sums of 24 bytes x the same -- ~17 x the LOD 0 blob for five
 * levels, ~19 x for seven; when that does not fit (or passes 2^31 elements) the levels are built one by one from LOD 0, which needs ~2 x. */
int cvx_world_build_lods(cvx_context *ctx, const void *storage, int64_t byteLength, int dimX, int dimY, int dimZ, int columnCount, int levelCount,
                         void **outStorage, int64_t *outByteLength, int32_t *outColumnCount, float *outDeviceMs);
void cvx_free(void *p);

/* ---- editing the uploaded world in place (World.SetVoxelColumn, World.cs:151-159) -----------------------------------------------------
 * `storage` is a sub-world blob in the reference's layout: `columnCount` 12-byte RLEColumn headers, then the element pool; column (x, z) of
 * the rectangle is header (x - x0) * sizeZ + (z - z0) (World.GetIndexKnownInBounds order; cvxh_world_extract_region makes such a blob from a
 * host world).  Coordinates are in the level's own columns.  Every column is validated on the host like cvx_world_upload's before anything on
 * the device changes: any failure returns CVX_ERR_INVALID_ARGUMENT (or CVX_ERR_CAPACITY: the 4 GiB arena, 2^30 colour slots per level) and
 * leaves the world as it was.  The edit is enqueued on the context's stream behind what is already there and the call returns once it is done:
 * a draw enqueued before it (CVX_DRAW_ASYNC included) renders the old world, every draw after it the new one.  Levels uploaded but not drawn
 * yet are placed in the arena first (what the next draw would do).  Colours and run-list blocks go to the column's old place when they fit,
 * else to a tail behind the level's colours / run list (a 4 x 8 colour block that gets too shallow moves there as a whole); the first edit of
 * a level lays the arena out again with headroom, and the arena grows when the headroom runs out.  Space edits leave behind is not compacted
 * by the edit: cvx_world_edit_stats reports it, and cvx_world_compact reclaims it on the device (so does uploading the level again).  With several
 * GPUs (one context per rank), every rank applies the same edit to its own context. */
/* World.SetVoxelColumn for a sizeX x sizeZ rectangle of one level (the caller supplies that level's columns). */
int cvx_world_set_columns(cvx_context *ctx, int lod, int x0, int z0, int sizeX, int sizeZ, const void *storage, int64_t byteLength, int columnCount);
/* Replaces a rectangle of LOD 0 and rebuilds LOD 1 .. levelCount (0 .. 5) over it on the device (World.DownSample of the sub-world, as
 * cvx_world_build_lods): x0, z0, sizeX, sizeZ must be multiples of 2^levelCount, so that every coarse column is rebuilt from its complete
 * footprint.  outDeviceMs (may be NULL): device time of the edit, from the sub-blob's upload to the last level's patch. */
int cvx_world_edit(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, const void *storage, int64_t byteLength, int columnCount, int levelCount,
                   float *outDeviceMs);
/* Arena occupancy (any pointer may be NULL): bytes in use (abandoned ones included), bytes that edits left behind, bytes of headroom left in
 * the edit tails.  A context that never edited reports its whole arena as used. */
int cvx_world_edit_stats(cvx_context *ctx, int64_t *usedBytes, int64_t *abandonedBytes, int64_t *spareBytes);

/* ---- voxel brushes and ray picking on the uploaded world ---------------------------------------------------------------------------------
 * Everything in LOD-0 voxel coordinates: voxel (x, y, z) is the unit cube [x, x+1) x [y, y+1) x [z, z+1), y = 0 at the bottom.
 * cvx_world_brush: voxel-level edits, computed on the device and handed to cvx_world_edit's machinery (records, tails, LOD refresh).  A stroke
 * acts on the voxels inside its shape, all integer: a box holds a <= (x, y, z) < b per axis; a sphere holds (x-a0)^2 + (y-a1)^2 + (z-a2)^2 <= r^2
 * (r = b[0] >= 0, 64-bit arithmetic).
 *   A capsule (CVX_SHAPE_CAPSULE) holds the voxels whose centre lies within r = pad_ of the segment from voxel a to voxel b.  With d = b - a,
 *   w = v - a, L = d.d and p = w.d: L == 0 or p <= 0: w.w <= r^2; p >= L: |v - b|^2 <= r^2; otherwise (w.w) L - p^2 <= r^2 L.  Limits:
 *   0 <= r <= 8191, |b[i] - a[i]| <= 8191 per axis, |a[i]| <= 2^30.  Footprint per axis: [min(a, b) - r, max(a, b) + r + 1).  A capsule with
 *   a == b is the sphere of that radius.
 *   An ellipsoid (CVX_SHAPE_ELLIPSOID) has the centre a and the radii (rx, ry, rz) = b, each 1 .. 1024 (pad_ ignored); with (dx, dy, dz) = v - a it
 *   holds dx^2 ry^2 rz^2 + dy^2 rx^2 rz^2 + dz^2 rx^2 ry^2 <= rx^2 ry^2 rz^2.  Footprint per axis: [a - r_axis, a + r_axis + 1).  With equal
 *   radii it is the sphere.
 *   Both rules are exact in int64 at these limits (products of at most 58 and 62 bits); nothing but integers decides a voxel.
 * FILL makes them solid with colour argb (solid ones included), CARVE makes them air, PAINT gives colour argb
 * to the solid ones and leaves air alone.  Strokes apply in array order (a later one sees what the earlier ones did) and are clipped to the world;
 * a stroke entirely outside it does nothing.  The call changes LOD 0 and rebuilds LOD 1 .. levelCount (0 .. 5) over the union of the strokes'
 * XZ footprints, rounded outward to multiples of 2^levelCount and clipped to the world: cvx_world_edit's rectangle.  Columns of that rectangle no
 * stroke touches are re-encoded with the builder's rule (WordBuilder.cs:181-268), which gives back the same column for every world the builder
 * made.  Ordering, atomicity and outDeviceMs are cvx_world_edit's.  CVX_ERR_INVALID_ARGUMENT: a bad op / shape, a negative radius, strokeCount
 * outside 1 .. CVX_BRUSH_MAX_STROKES, a sphere radius above 2^30, a capsule or an ellipsoid outside its limits (the message names the stroke)
 * or levelCount outside 0 .. 5; CVX_ERR_CAPACITY: a column would need more than 65535 runs, a run longer than
 * 32767 voxels or a colour index above 32767 (World.cs:161-259 keeps them in ushort / short), or the arena limits of cvx_world_edit.  Either
 * leaves the world as it was.  With several GPUs every rank applies the same strokes to its own context. */
enum { CVX_BRUSH_FILL = 0, CVX_BRUSH_CARVE = 1, CVX_BRUSH_PAINT = 2 };
enum { CVX_SHAPE_BOX = 0, CVX_SHAPE_SPHERE = 1 };
/* The codes 2 .. 15 are not shapes and stay rejected as "bad shape": callers and tests rely on 2 and 5 being invalid.  Do not renumber. */
enum { CVX_SHAPE_CAPSULE = 16, CVX_SHAPE_ELLIPSOID = 17 };
#define CVX_BRUSH_MAX_STROKES 4096
typedef struct cvx_brush_stroke { /* 40 bytes */
	int32_t op;    /* CVX_BRUSH_* */
	int32_t shape; /* CVX_SHAPE_* */
	int32_t a[3];  /* box: min corner (inclusive); sphere, ellipsoid: centre voxel; capsule: first end voxel */
	int32_t b[3];  /* box: max corner (exclusive); sphere: b[0] = radius, b[1], b[2] ignored; ellipsoid: the radii; capsule: second end voxel */
	uint32_t argb; /* FILL / PAINT colour (ColorARGB32 byte order, as the blobs hold it) */
	int32_t pad_;  /* capsule: the radius; every other shape: ignored */
} cvx_brush_stroke;
int cvx_world_brush(cvx_context *ctx, const cvx_brush_stroke *strokes, int strokeCount, int levelCount, float *outDeviceMs);

/* cvx_world_pick: first-hit ray queries against LOD 0, one per ray.  A ray is origin + t * direction in the space of cvx_camera_data's
 * PositionXZ / PositionY (direction need not be normalised; t is in its units).  The hit is the first solid voxel whose cube the ray enters for
 * 0 <= t <= maxT: voxel, the face it came in through (0 .. 5 = -X, +X, -Y, +Y, -Z, +Z: a ray travelling +X enters through -X, face 0), its
 * colour and t.  A ray that starts inside a solid voxel hits it with face 6 and t = 0.  A miss: voxel {-1, -1, -1}, face -1, argb 0, t = maxT.
 * Rays that start outside the world are clipped to its box first.  The traversal is float64 (cvx_brush.h, PickRay); rays that graze a voxel
 * edge within ~1e-9 voxel may resolve either way.  `rays` / `hits` are host arrays of rayCount entries; the call is ordered on the context's
 * stream behind every edit, brush and draw enqueued before it and returns when the hits are copied back.  cvx_world_pick_device takes device
 * arrays and enqueues on hipStream (NULL = the context's stream) without waiting; the caller orders that stream after the context's work. */
typedef struct cvx_pick_ray { /* 32 bytes */
	float origin[3];
	float direction[3];
	float maxT;
	float pad_;
} cvx_pick_ray;
typedef struct cvx_pick_hit { /* 24 bytes */
	int32_t voxel[3];
	int32_t face;
	uint32_t argb;
	float t;
} cvx_pick_hit;
int cvx_world_pick(cvx_context *ctx, int rayCount, const cvx_pick_ray *rays, cvx_pick_hit *hits);
int cvx_world_pick_device(cvx_context *ctx, int rayCount, const cvx_pick_ray *raysDevice, cvx_pick_hit *hitsDevice, void *hipStream);

/* ---- stamping triangle meshes into the uploaded world ------------------------------------------------------------------------------------
 * cvx_world_stamp_mesh: voxelises a triangle mesh on the device with the host voxeliser's rule (VoxelizerHelper.GetVoxelsInternal,
 * VoxelizerHelper.cs:28-132, and the material step of WordBuilder.cs:76-88: what cvxh_world_from_obj runs) and merges the voxels into LOD 0, then
 * rebuilds LOD 1 .. levelCount (0 .. 5).  Vertices are in LOD-0 voxel coordinates (the space cvxh_mesh_rescale produces; the caller applies any
 * placement or rotation); triangle k is vertices[indices[3k .. 3k+2]].  Per triangle: the corners pushed out by half a voxel, every voxel of the
 * clamped box within half a voxel of the plane and inside the triangle, at most 262144 such hits (x, then z, then y order); the colour is the
 * interpolated vertex colour, times the texel of material (int8_t)vertex0.material when that index is in 0 .. materialCount - 1 and the material
 * has a texture (no texture: white); a texel with alpha < 1 emits no voxel (it still counts towards the 262144).  Parts outside the world are
 * clipped.  Several hits of one voxel merge into the average of their colours (per channel sum / count, alpha 255: ToFinalColumn).
 * op: CVX_BRUSH_FILL makes the stamped voxels solid with their colour (solid ones included), CVX_BRUSH_CARVE makes them air, CVX_BRUSH_PAINT
 * recolours the solid ones and leaves air alone.  The rectangle is the XZ box of the stamped voxels rounded outward to multiples of
 * 2^levelCount and clipped to the world; no stamped voxel: CVX_OK, nothing changes, *outDeviceMs = 0.  Ordering, atomicity, outDeviceMs and
 * CVX_ERR_CAPACITY / CVX_ERR_NOT_READY are cvx_world_brush's; a voxel list that does not fit in device memory is CVX_ERR_CAPACITY and leaves the
 * world as it was.  CVX_ERR_INVALID_ARGUMENT: a bad op, levelCount outside 0 .. 5, indexCount not a multiple of 3, an index outside
 * 0 .. vertexCount - 1, materialCount outside 0 .. 128, a texture with rgba but a width or height below 1 (or above 2^15), a vertex coordinate
 * that is not finite or whose magnitude is above 2^24.  Device memory while it runs, besides the mesh and its textures: ~72 bytes per triangle,
 * 12 bytes per (triangle, column) pair of the triangles' boxes, ~40 bytes per hit (the voxel list and its sort), and cvx_world_brush's scratch
 * for the rectangle.  With several GPUs every rank stamps its own context. */
typedef struct cvx_mesh_vertex { /* 28 bytes */
	float position[3];  /* LOD-0 voxel coordinates */
	uint8_t rgba[4];    /* vertex colour (alpha unused) */
	float uv[2];
	int32_t material;   /* index into `materials`; used as (int8_t)material, like the reference's (sbyte) */
} cvx_mesh_vertex;
typedef struct cvx_mesh_texture { /* 16 bytes */
	int32_t width, height;
	const uint8_t *rgba; /* width * height RGBA8 texels, row 0 = the BOTTOM row (cvxh_image_load); NULL: no texture */
} cvx_mesh_texture;
#define CVX_STAMP_MAX_MATERIALS 128
int cvx_world_stamp_mesh(cvx_context *ctx, const cvx_mesh_vertex *vertices, int vertexCount, const int32_t *indices, int64_t indexCount,
                         const cvx_mesh_texture *materials, int materialCount, int op, int levelCount, float *outDeviceMs);

/* ---- copying, moving and rotating voxel boxes inside the uploaded world ------------------------------------------------------------------
 * cvx_world_copy: places boxes of voxels the world already holds elsewhere in it (duplicate, move, quarter turns, mirror, scatter), computed on
 * the device and handed to cvx_world_edit's machinery like a brush.  Let W be LOD 0 before the call; the result R is:
 *   1. R = W; for every placement with move = 1, every voxel of its source box becomes air in R.
 *   2. The placements in array order: for every destination voxel d inside the world, s = W(T^-1(d)) -- every read is from W, the snapshot, so
 *      source and destination may overlap -- and the op decides R(d): CVX_COPY_REPLACE R(d) = s (air included); CVX_BRUSH_FILL: s solid ->
 *      R(d) = s; CVX_BRUSH_CARVE: s solid -> R(d) = air; CVX_BRUSH_PAINT: s solid and R(d) solid -> R(d) takes s's colour.  Colours are copied
 *      verbatim (the arena's ARGB words).
 * The transform T of a placement: (p, q, r) = v - srcMin in the source box of size (sx, sy, sz); mirror X (bit 2): p = sx-1-p; each of the k
 * quarter turns (bits 0-1): (p, r, sx, sz) = (sz-1-r, p, sz, sx); flip Y (bit 3): q = sy-1-q; the destination voxel is dst + (p, q, r).  After an
 * odd k the destination box has size (sz, sy, sx).  A source box lies inside the world with srcMin < srcMax per axis; destination voxels outside
 * the world are dropped; a placement whose destination lies wholly outside writes nothing (its move still carves).  The call edits the bounding
 * XZ rectangle of every clipped destination footprint and every moving placement's source footprint, rounded outward to multiples of
 * 2^levelCount and clipped to the world (cvx_world_brush's rectangle); nothing to change: CVX_OK and *outDeviceMs = 0.  Coordinates are LOD-0
 * voxels of the stored tile: a repeating world does not wrap them.  Ordering, atomicity, outDeviceMs, CVX_ERR_CAPACITY (the brush's format
 * limits, the arena limits) and CVX_ERR_NOT_READY are cvx_world_brush's; every error leaves the world as it was.  CVX_ERR_INVALID_ARGUMENT: a
 * bad op, move not 0 / 1, unknown transform bits, placementCount outside 1 .. CVX_COPY_MAX_PLACEMENTS, levelCount outside 0 .. 5, an empty
 * source box or one outside the world, a |dst| component above 2^30.  With several GPUs every rank applies the same placements to its own
 * context. */
enum { CVX_COPY_REPLACE = 3 }; /* op: also CVX_BRUSH_FILL / CVX_BRUSH_CARVE / CVX_BRUSH_PAINT */
#define CVX_COPY_MAX_PLACEMENTS 1024
typedef struct cvx_copy_placement { /* 48 bytes */
	int32_t srcMin[3];  /* source box in LOD-0 voxels, inclusive */
	int32_t srcMax[3];  /* exclusive */
	int32_t dst[3];     /* min corner of the destination box */
	int32_t transform;  /* bits 0-1: quarter turns k; bit 2: mirror X (before turning); bit 3: flip Y; other bits 0 */
	int32_t op;         /* CVX_COPY_REPLACE, CVX_BRUSH_FILL, CVX_BRUSH_CARVE, CVX_BRUSH_PAINT */
	int32_t move;       /* 1: the source box becomes air */
} cvx_copy_placement;
int cvx_world_copy(cvx_context *ctx, const cvx_copy_placement *placements, int placementCount, int levelCount, float *outDeviceMs);

/* ---- finding and removing the floating pieces of the uploaded world ----------------------------------------------------------------------
 * cvx_world_pieces: what a carve or a move has cut loose.  The voxels considered are the solid voxels of LOD 0 inside [boxMin, boxMax) after
 * clipping the box to the world (coordinates address the stored tile: a repeating world does not wrap them).  Two of them are connected when
 * they share a FACE (edge and corner contact does not connect); a piece is a connected component.  A piece is ANCHORED by the bits of `anchors`
 * (any combination; 0: nothing is anchored): CVX_ANCHOR_GROUND, it holds a voxel with y = 0; CVX_ANCHOR_OUTSIDE, it holds a voxel with a solid
 * face neighbour inside the world but outside the clipped box (a box cut out of a larger structure does not report the structure);
 * CVX_ANCHOR_LARGEST, it is the piece with the most voxels (ties: the earlier one in the order below).  Every other piece is FLOATING.
 * Order: a piece's seed is its voxel in its first column in (x, then z) order and, in that column, the highest y.  The floating pieces are listed
 * by ascending seed x, then ascending z, then DESCENDING y; the list does not depend on scheduling: the same world gives the same bytes.
 * `summary` (may be NULL) receives all four totals; `pieces` (may be NULL iff pieceCapacity = 0) the first min(pieceCapacity, floatingPieces)
 * floating pieces; a smaller capacity is not an error.
 * CVX_PIECES_REPORT never changes the world.  CVX_PIECES_REMOVE turns every voxel of every floating piece (whatever the capacity) into air
 * through cvx_world_edit's machinery like a brush: the rectangle is the XZ bounding box of the floating pieces rounded outward to multiples of
 * 2^levelCount and clipped to the world, LOD 1 .. levelCount (0 .. 5) are rebuilt over it, and columns of it that lose nothing are re-encoded
 * with the builder's rule (unchanged for every world the builder made).  No floating piece: CVX_OK, nothing changes.  outDeviceMs (may be
 * NULL): device time of the analysis and, for a REMOVE that removes something, the edit.
 * Ordering, atomicity and several GPUs as cvx_world_brush: the call is ordered on the context's stream behind everything enqueued before it,
 * returns when the results are on the host, every error leaves the world as it was, and every rank makes the same call on its own context.
 * CVX_ERR_INVALID_ARGUMENT: a NULL box, boxMin >= boxMax on an axis, a box wholly outside the world, unknown anchors bits or op, levelCount
 * outside 0 .. 5, a negative pieceCapacity, pieces NULL with a capacity above 0; CVX_ERR_NOT_READY: LOD 0 has not been uploaded;
 * CVX_ERR_CAPACITY: the scratch does not fit in device memory, the box holds 2^31 or more columns or solid runs, and on REMOVE the limits of
 * cvx_world_brush.  Device memory while it runs: 8 bytes per column of the clipped box and 64 bytes per solid run of LOD 0 inside it (its
 * interval, column and label, and the totals, box and anchor bits of the piece it may be the seed of), plus 48 bytes per listed piece; a REMOVE
 * adds cvx_world_brush's scratch for its rectangle. */
enum { CVX_PIECES_REPORT = 0, CVX_PIECES_REMOVE = 1 };
enum { CVX_ANCHOR_GROUND = 1, CVX_ANCHOR_OUTSIDE = 2, CVX_ANCHOR_LARGEST = 4 };
typedef struct cvx_piece { /* 48 bytes */
	int32_t min[3];  /* bounding box in LOD-0 voxels, inclusive */
	int32_t max[3];  /* exclusive */
	int32_t seed[3]; /* the piece's first voxel in the order above */
	int32_t pad_;
	int64_t voxels;
} cvx_piece;
typedef struct cvx_pieces_summary { /* 32 bytes */
	int64_t floatingPieces, floatingVoxels, anchoredPieces, anchoredVoxels;
} cvx_pieces_summary;
int cvx_world_pieces(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int op, int levelCount, cvx_piece *pieces,
                     int pieceCapacity, cvx_pieces_summary *summary, float *outDeviceMs);

/* ---- letting the floating pieces of the uploaded world fall ---------------------------------------------------------------------------------
 * cvx_world_settle: the floating pieces of cvx_world_pieces fall straight down until they rest (voxlap makes its loose pieces fall; the call a
 * host makes after a carve instead of CVX_PIECES_REMOVE).  Let W be LOD 0 before the call.
 *   Which pieces.  The floating pieces F_1 .. F_m are exactly the list cvx_world_pieces(..., CVX_PIECES_REPORT, ...) gives for the same box and
 *     anchors: the same clipping, anchor rules and order.  pieces[i] (may be NULL iff pieceCapacity = 0) describes F_i BEFORE the fall, the same
 *     bytes as REPORT; drops[i] (drops may be NULL) is how many voxels F_i fell.  Both receive the first min(pieceCapacity, m) entries; a smaller
 *     capacity is not an error, and all pieces fall whatever the capacity.
 *   Static.  Every solid voxel of W that belongs to no floating piece is static -- anywhere in its column, inside or outside the box -- and so is
 *     everything at y < 0.
 *   The fall, as unit steps.  Repeat: let M be the largest set of floating pieces such that every voxel (x, y, z) of a piece of M, at its current
 *     place, has y > 0 and (x, y - 1, z) is air or a voxel of a piece of M.  If M is empty, or maxDrop steps have been made
 *     (CVX_SETTLE_UNLIMITED: no bound), stop; otherwise every piece of M moves down by one.  Pieces are rigid: they never rotate or break, and they
 *     move in y only.
 *   Closed form (what the device computes).  For every node of a floating piece p (a solid run clipped to the box's y range) take the next solid
 *     voxel below it in its column, g >= 0 voxels of air away.  Static (the floor counts, with g = the node's lowest y): d_p <= g.  A voxel of
 *     another floating piece q: d_p <= d_q + g.  A voxel of p itself: no constraint.  d is the largest solution, i.e. the shortest-path distance
 *     to "static" in the piece graph (which may hold cycles: interlocked pieces fall and stop together), and drop = min(d, maxDrop).  The unit
 *     steps never violate a constraint and stop only when every piece has a tight chain down to something static, so both give the same drops.
 *   Result.  Static voxels stay; voxel (x, y, z) of F_i moves to (x, y - drop_i, z) with its colour word verbatim (a baked shade travels with it:
 *     relight with cvx_world_light); runs that come to touch merge.
 *   Animation.  A piece that has fallen only part of the way is still floating: k calls with maxDrop = 1 equal one call with maxDrop = k.
 *   Torn pieces.  As with CVX_PIECES_REMOVE, without CVX_ANCHOR_OUTSIDE a "piece" may be the clipped part of a larger structure, and it is torn
 *     from it: the part of a run above the box's top stays while the part inside falls.  A run that crosses the box's BOTTOM leaves its lower part
 *     static directly beneath the node (g = 0): that piece does not move.
 * Mechanics as CVX_PIECES_REMOVE: the rectangle is the XZ bounding box of the pieces with drop > 0 rounded outward to multiples of 2^levelCount
 * and clipped to the world, LOD 1 .. levelCount (0 .. 5) are rebuilt over it, and columns of it that nothing moves in are re-encoded with the
 * builder's rule.  Nothing falls: CVX_OK, the arena is untouched.  `summary` (may be NULL): floatingPieces / floatingVoxels as cvx_pieces_summary,
 * fallenPieces / fallenVoxels those with drop > 0, largestDrop.  outDeviceMs (may be NULL): device time of the analysis and, when something
 * falls, the edit.  Ordering, atomicity and several GPUs as cvx_world_brush; every error leaves the world as it was.  Errors are those of
 * cvx_world_pieces (its bad op aside), and CVX_ERR_INVALID_ARGUMENT for maxDrop < 0.  Device memory while it runs: cvx_world_pieces' and 16 more
 * bytes per solid run inside the box. */
#define CVX_SETTLE_UNLIMITED 0
typedef struct cvx_settle_summary { /* 40 bytes */
	int64_t floatingPieces, floatingVoxels; /* as cvx_pieces_summary */
	int64_t fallenPieces, fallenVoxels;     /* those with drop > 0 */
	int32_t largestDrop;
	int32_t pad_;
} cvx_settle_summary;
int cvx_world_settle(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int anchors, int maxDrop, int levelCount, cvx_piece *pieces,
                     int32_t *drops, int pieceCapacity, cvx_settle_summary *summary, float *outDeviceMs);

/* ---- finding and filling the enclosed cavities of the uploaded world -----------------------------------------------------------------------
 * cvx_world_cavities: what a stamped or built shell encloses (voxlap's sethollowfill: the call a host makes after cvx_world_stamp_mesh, so that a
 * later carve cuts into rock instead of an empty inside).  The voxels considered are the AIR voxels of LOD 0 inside [boxMin, boxMax) after
 * clipping the box to the world (coordinates address the stored tile: a repeating world does not wrap them).  Two of them are connected when
 * they share a FACE; a REGION is a connected component inside the clipped box.  A region is OPEN when for some face f of the clipped box with
 * bit f set in openFaces (bits 0..5 = -X,+X,-Y,+Y,-Z,+Z, the pick's face numbers) it holds a voxel lying on face f and the voxel across that
 * face is air: a voxel outside the world counts as air, below y = 0 and above dimY too; inside the world the arena decides.  Every other
 * region is an ENCLOSED CAVITY.  A box that cuts a cavity in two leaves its inner part open through the cut; with the cut face's bit cleared the
 * inner part counts as enclosed, and it alone is filled.  The SELECTED cavities are the enclosed ones of at most maxVoxels voxels (0: all).
 * Order: seed, bounding box, `voxels` and the order are exactly cvx_world_pieces': a cavity's seed is its voxel in its first column in (x, then
 * z) order and, there, the highest y; the list is by ascending seed x, then ascending z, then DESCENDING y, and does not depend on scheduling:
 * the same world gives the same bytes.  `summary` (may be NULL) receives the six totals; `cavities` (may be NULL iff cavityCapacity = 0) the
 * first min(cavityCapacity, selectedCavities) selected cavities; a smaller capacity is not an error.
 * CVX_CAVITIES_REPORT never changes the world.  CVX_CAVITIES_FILL makes every voxel of every selected cavity (whatever the capacity) solid
 * with the colour word argb, verbatim, through cvx_world_edit's machinery like CVX_PIECES_REMOVE: the rectangle is the XZ bounding box of the
 * selected cavities rounded outward to multiples of 2^levelCount and clipped to the world, LOD 1 .. levelCount (0 .. 5) are rebuilt over it,
 * columns of it that gain nothing are re-encoded with the builder's rule, and runs that come to touch merge.  Nothing selected: CVX_OK, the
 * arena is untouched.  outDeviceMs (may be NULL): device time of the analysis and, for a FILL that fills something, the edit.
 * Ordering, atomicity and several GPUs as cvx_world_pieces; every error leaves the world as it was.
 * CVX_ERR_INVALID_ARGUMENT: NULL params, boxMin >= boxMax on an axis, a box wholly outside the world, openFaces bits above 0x3F, a bad op,
 * maxVoxels < 0, levelCount outside 0 .. 5, a negative cavityCapacity, cavities NULL with a capacity above 0; CVX_ERR_NOT_READY: LOD 0 has not
 * been uploaded; CVX_ERR_CAPACITY: the scratch does not fit in device memory, the box holds 2^31 or more columns or air intervals, and on FILL
 * the format and arena limits of cvx_world_brush (a filled column needs one colour per voxel: at most 32767 solid voxels above a run).
 * Device memory while it runs: 8 bytes per column of the clipped box and 64 bytes per air interval of LOD 0 inside it (a maximal run of air
 * voxels of one column: its interval, column and label, and the totals, box and open bits of the region it may be the seed of), plus 48 bytes
 * per listed cavity; a FILL adds cvx_world_brush's scratch for its rectangle. */
enum { CVX_CAVITIES_REPORT = 0, CVX_CAVITIES_FILL = 1 };
#define CVX_CAVITY_OPEN_DEFAULT 0x3B   /* every face but -Y: the ground is watertight */
typedef struct cvx_cavity_params {     /* 48 bytes */
	int32_t boxMin[3];   /* LOD-0 voxels, inclusive */
	int32_t boxMax[3];   /* exclusive */
	int32_t openFaces;   /* bits 0..5 = -X,+X,-Y,+Y,-Z,+Z (the pick's face numbers): the faces of the clipped box air may escape through */
	int32_t op;          /* CVX_CAVITIES_* */
	uint32_t argb;       /* FILL: the colour word every filled voxel gets, verbatim */
	int32_t pad_;
	int64_t maxVoxels;   /* 0: no limit; else only cavities of at most this many voxels are selected */
} cvx_cavity_params;
typedef struct cvx_cavities_summary {  /* 48 bytes */
	int64_t enclosedCavities, enclosedVoxels;   /* every enclosed cavity, whatever maxVoxels */
	int64_t selectedCavities, selectedVoxels;   /* those within maxVoxels: what is listed and what FILL fills */
	int64_t openRegions, openVoxels;
} cvx_cavities_summary;
int cvx_world_cavities(cvx_context *ctx, const cvx_cavity_params *params, int levelCount, cvx_piece *cavities, int cavityCapacity,
                       cvx_cavities_summary *summary, float *outDeviceMs);

/* ---- lighting the uploaded world: sky occlusion and sun shadows ----------------------------------------------------------------------------
 * cvx_world_light: bakes a shade, an integer 0 .. 255, into every solid LOD-0 voxel v inside [boxMin, boxMax) clipped to the world (voxlap's
 * updatelighting: the call a host makes after an edit).  The shade is computed from occupancy alone -- no colour is read for it, no occupancy
 * changes --; every voxel outside the world is air, below y = 0 and above dimY too; coordinates address the stored tile: a repeating world does
 * not wrap them.  No surface normals are used: the worlds are thin shells, and the shell itself is the occluder.
 *   1. Sky: the 17 directions d = (dx, dy, dz), dx, dz in {-1, 0, 1}, dy in {0, 1}, not (0, 0, 0), weigh 2 (dy = 1) or 1 (dy = 0), 26 in all.
 *      d is OPEN when every voxel v + s * d, s = 1 .. skyRange, is air; sky = the weights of the open directions; skyTerm = skyLevel * sky / 26.
 *   2. Sun, for S = sunDir != (0, 0, 0), in exact integers: facing = the sum of |S_i| over the axes with S_i != 0 whose face neighbour
 *      v + sgn(S_i) * e_i is air, den = the sum of all |S_i|.  The shadow walk follows the ray from the centre of v along S: axis i crosses its
 *      k-th voxel plane at (2k - 1) / |S_i|; per step ALL axes that attain the smallest pending parameter advance together (an exact edge or
 *      corner crossing visits no in-between voxel; fractions compared by cross-multiplying in 64 bits); each voxel reached is tested: outside the
 *      world -> lit, solid -> shadowed; after sunRange voxels -> lit.  sunTerm = lit ? sunLevel * facing / den : 0.
 *   3. shade = min(255, floorLevel + skyTerm + sunTerm) (every division floors).
 *   4. target CVX_LIGHT_TO_RGB: each of R, G, B becomes (c * shade + 127) / 255, A stays.  The bake is one-shot: the colours the world holds are
 *      the albedo, lighting twice shades twice; a caller that relights keeps the unlit rectangle with cvx_world_read_region and puts it back with
 *      cvx_world_edit first.  CVX_LIGHT_TO_ALPHA: A becomes the shade, R, G, B stay (voxlap's convention, for hosts whose own blit shader
 *      multiplies); idempotent.  The coarse levels take their alpha by World.DownSample's rule, the alpha of the FIRST voxel of a coarse voxel in
 *      the reference's insertion order, not an average of the shades.  (A colour word's bytes are a, r, g, b: A is the low byte.)
 * Mechanics, ordering, atomicity, outDeviceMs and several GPUs are cvx_world_brush's: the rectangle is the clipped box's XZ footprint rounded
 * outward to multiples of 2^levelCount and clipped to the world; every column of it is re-emitted in the builder's encoding (so a foreign column
 * with split runs or shared colours gets one colour per voxel), with the new colours inside the box and the old ones elsewhere; LOD 1 ..
 * levelCount (0 .. 5) are rebuilt over it; every error leaves the world as it was.  A box wholly outside the world: CVX_OK, nothing changes,
 * *outDeviceMs = 0.  CVX_ERR_INVALID_ARGUMENT: NULL params, boxMin >= boxMax on an axis, a bad target, a level outside 0 .. 255, sunRange outside
 * 0 .. 4096, skyRange outside 0 .. 32, a |sunDir| component above 1024, levelCount outside 0 .. 5; CVX_ERR_NOT_READY: LOD 0 has not been
 * uploaded; CVX_ERR_CAPACITY: as cvx_world_brush. */
enum { CVX_LIGHT_TO_RGB = 0, CVX_LIGHT_TO_ALPHA = 1 };
typedef struct cvx_light_params { /* 64 bytes */
	int32_t boxMin[3];   /* LOD-0 voxels, inclusive */
	int32_t boxMax[3];   /* exclusive */
	int32_t sunDir[3];   /* TOWARDS the sun, integers, each |.| <= 1024; (0,0,0): no sun term */
	int32_t sunLevel;    /* 0 .. 255 */
	int32_t sunRange;    /* 0 .. 4096 voxels visited by the shadow walk; 0: nothing shadows */
	int32_t skyLevel;    /* 0 .. 255 */
	int32_t skyRange;    /* 0 .. 32 voxels tested per sky direction; 0: every direction is open */
	int32_t floorLevel;  /* 0 .. 255: what a fully occluded voxel keeps */
	int32_t target;      /* CVX_LIGHT_TO_RGB / CVX_LIGHT_TO_ALPHA */
	int32_t pad_;
} cvx_light_params;
int cvx_world_light(cvx_context *ctx, const cvx_light_params *params, int levelCount, float *outDeviceMs);

/* cvx_world_light_lamps: cvx_world_light with point lights (voxlap's vx5.lightsrc: torches, lamps, a flash baked after an explosion).  The bake
 * is one-shot, so a lamp cannot be added by a second call: its term goes into the same sum before the one min.  Everything cvx_world_light
 * documents holds (mechanics, ordering, atomicity, rectangle rounding, outDeviceMs, box clipping, errors; a box outside the world: CVX_OK and
 * 0 ms); with lampCount == 0 (lamps may be NULL then) the call gives the bytes cvx_world_light gives.  Lamps are white.
 * The rule, exact integers from end to end, for solid voxel v inside the clipped box and lamp l at voxel L (its CENTRE), D = L - v, d2 = |D|^2,
 * r2 = radius^2:
 *   1. D = 0 or d2 >= r2: the term is 0.
 *   2. facing = the sum of |D_i| over the axes with D_i != 0 whose face neighbour v + sgn(D_i) * e_i is air, den = the sum of all |D_i| (the
 *      sun's rule with S = D).
 *   3. The shadow walk is the sun's walk from the centre of v along D (plane crossings at (2k - 1) / |D_i|, all axes that tie advance
 *      together).  It ends when it ARRIVES at voxel L, which it does exactly, after at most |D_x| + |D_y| + |D_z| steps.  Every voxel reached
 *      before L is tested: outside the world is air and the walk goes on, a solid voxel means shadowed.  L itself is never tested: a lamp set
 *      into a wall lights the room.
 *   4. term_l = lit ? level * (r2 - d2) * facing / (r2 * den) : 0, ONE floored division (a falloff of 1 - (d / r)^2).
 *   5. shade = min(255, floorLevel + skyTerm + sunTerm + the sum of term_l over ALL lamps): an integer sum before one min, so no lamp order and
 *      no schedule shows in the result.
 * A lamp may lie in a solid voxel, in air, outside the box or outside the world.  CVX_ERR_INVALID_ARGUMENT besides cvx_world_light's (all
 * checked on the host before anything is enqueued): lampCount outside 0 .. CVX_LIGHT_MAX_LAMPS, lamps NULL with lampCount > 0, a radius outside
 * 1 .. CVX_LAMP_MAX_RADIUS, a level outside 0 .. 255, a |pos| component above 2^20. */
#define CVX_LIGHT_MAX_LAMPS   4096
#define CVX_LAMP_MAX_RADIUS   64
typedef struct cvx_lamp {     /* 32 bytes */
	int32_t pos[3];           /* the LOD-0 voxel whose CENTRE the lamp sits at; may lie outside the world or the box; |.| <= 2^20 */
	int32_t radius;           /* 1 .. 64 voxels */
	int32_t level;            /* 0 .. 255 */
	int32_t pad_[3];
} cvx_lamp;
int cvx_world_light_lamps(cvx_context *ctx, const cvx_light_params *params, const cvx_lamp *lamps, int lampCount, int levelCount, float *outDeviceMs);

/* ---- moving boxes through the uploaded world: collision and sliding ------------------------------------------------------------------------
 * cvx_world_move: moves axis-aligned boxes (players, NPCs, debris) through LOD 0 without entering solid voxels (voxlap's clipmove: the call a
 * host makes every frame).  The rule is integer from end to end (cvx_move.h): positions, sizes and displacements are in units of 1 / CVX_MOVE_UNIT
 * voxel, the same input gives the same bytes on every machine, and neither call changes the world.
 *   Occupancy.  Voxel (x, y, z) of the stored tile is solid as the arena says.  Outside it, the first rule that applies: y >= dimY is air;
 *     y < 0 is solid iff CVX_MOVE_SOLID_BELOW; x or z outside the tile is solid iff CVX_MOVE_SOLID_SIDES.  In a repeating world
 *     (cvx_set_world_repeat) x and z wrap by floor-mod instead and CVX_MOVE_SOLID_SIDES has no effect.
 *   Overlap.  The box occupies [pos_i, pos_i + size_i) per axis and covers the voxels floor(pos_i / 256) .. floor((pos_i + size_i - 1) / 256)
 *     (division floors for negatives).
 *   A leg on axis a by d != 0 from the box's current position; the cross-section is the covered voxel ranges of the other two axes.  Going +:
 *     with hi the last covered slab, the slabs k = hi + 1 .. floor((pos_a + size_a + d - 1) / 256) are entered in order; the first k with a solid
 *     voxel in the cross-section stops the box flush, moved = min(d, 256 k - (pos_a + size_a)).  Going -: with lo the first covered slab, k =
 *     lo - 1 down to floor((pos_a + d) / 256), moved = min(|d|, pos_a - 256 (k + 1)).  Slabs the box already covers are never tested (an embedded
 *     body can leave).  The leg sets its direction's blocked bit iff moved < |d|.
 *   Slide A from P0 = pos: legs Y, X, Z with delta's components, zero components skipped (the usual voxel-game move, not a simultaneous sweep).
 *   Step-up, tried iff stepUp > 0, delta_y <= 0, A set an X or Z blocked bit, and the body is grounded (A's Y leg was blocked going down, or
 *     delta_y = 0 and P0 is resting).  Attempt B from P0: a +Y leg by stepUp moving r, an X leg by delta_x, a Z leg by delta_z, a -Y leg by
 *     r - delta_y.  B replaces A iff |x_B - x_0| + |z_B - z_0| is strictly larger than A's; B's flags are the blocked bits of its X and Z legs, -Y
 *     if its last leg was blocked, and CVX_MOVED_STEPPED (the raise never sets +Y).
 *   CVX_MOVED_RESTING: at the final position pos_y % 256 = 0 and slab pos_y / 256 - 1 holds a solid voxel under the XZ footprint.
 *   CVX_MOVED_STARTS_SOLID: the box at P0 overlaps a solid voxel.  A body without it never ends overlapping one.  delta = 0 is a pure overlap
 *     and ground query.
 * cvx_world_move takes host arrays; it is ordered on the context's stream behind every draw, edit and brush enqueued before it (levels uploaded
 * but not placed yet are placed first) and returns when the results are copied back.  cvx_world_move_device takes device arrays and enqueues on
 * hipStream (NULL = the context's stream) without waiting; the caller orders that stream after the context's work.  lanesPerBody G: G consecutive
 * lanes of a wave own one body and share the columns of each leg (1: a thread per body, for thousands of small boxes; 64: a wave per body, for a
 * footprint of hundreds of columns); 0 = 16; the result does not depend on it.  The host-array call picks ONE G for the whole call from the
 * largest leg region among its bodies: put bodies of very different sizes (debris and a vehicle) into separate calls.
 * CVX_ERR_NOT_READY: LOD 0 has not been uploaded.  CVX_ERR_INVALID_ARGUMENT: a NULL pointer, bodyCount < 1, lanesPerBody not one of 0, 1, 4, 16,
 * 64, and in the host-array call any body outside the limits below, with a |pos| component above 2^28 or with unknown flag bits (nothing runs).
 * The device call cannot read its input on the host: for such a body the kernel writes pos back unchanged with CVX_MOVED_INVALID and walks
 * nothing; every loop of the kernel is bounded by the limits whatever the input. */
#define CVX_MOVE_UNIT 256            /* position units per LOD-0 voxel */
enum { CVX_MOVE_SOLID_BELOW = 1, CVX_MOVE_SOLID_SIDES = 2 };                 /* body.flags */
enum { CVX_MOVED_BLOCKED_MASK = 0x3F,  /* bits 0..5: stopped going -X,+X,-Y,+Y,-Z,+Z (the pick's face numbers) */
       CVX_MOVED_RESTING = 1 << 6, CVX_MOVED_STARTS_SOLID = 1 << 7, CVX_MOVED_STEPPED = 1 << 8, CVX_MOVED_INVALID = 1 << 31 };
typedef struct cvx_move_body {   /* 48 bytes */
	int32_t pos[3];    /* min corner, units */
	int32_t size[3];   /* units, 1 .. 64 * 256 per axis */
	int32_t delta[3];  /* requested displacement, units, |.| <= 256 * 256 */
	int32_t stepUp;    /* 0 .. 4 * 256 */
	int32_t flags;     /* CVX_MOVE_SOLID_* */
	int32_t pad_;
} cvx_move_body;
typedef struct cvx_move_result { /* 16 bytes */
	int32_t pos[3];
	int32_t flags;     /* CVX_MOVED_* */
} cvx_move_result;
int cvx_world_move(cvx_context *ctx, int bodyCount, const cvx_move_body *bodies, cvx_move_result *results);
int cvx_world_move_device(cvx_context *ctx, int bodyCount, const cvx_move_body *bodiesDevice, cvx_move_result *resultsDevice,
                          int lanesPerBody, void *hipStream);

/* ---- walking-distance fields over the uploaded world -----------------------------------------------------------------------------------------
 * cvx_world_nav_build: the question that precedes every cvx_world_move -- which way should this body go?  The call builds a DISTANCE FIELD (a
 * flow field) over the places a box of width x height x width voxels can stand in LOD 0, walking towards one or more goals with step-up and
 * drop limits; cvx_nav_query reads it for thousands of agents per frame.  The rule is exact integers in LOD-0 voxels of the stored tile (a
 * repeating world does not wrap); neither call changes the world.
 *   Blocked.  A CELL (x, y, z) is the voxel of the body's min corner.  B(x, y, z) is true when any voxel (x + i, y, z + k), 0 <= i, k < width, is
 *     solid in the arena; everything at y >= dimY is air, y < 0 is the floor (solid).  Cells exist only for x0 <= x <= x1 - width and
 *     z0 <= z <= z1 - width of the box clipped to the world: the body lies inside the clipped box in X and Z.  A box narrower than the body has
 *     no cells: CVX_OK and an empty field.
 *   Stand cell.  y0 <= y < y1 (the clipped box's y range selects floors only; headroom is read above y1 as well), B(x, y + j, z) false for
 *     j = 0 .. height - 1, and y = 0 or B(x, y - 1, z) true: exactly a body for which cvx_world_move with CVX_MOVE_SOLID_BELOW reports
 *     CVX_MOVED_RESTING without CVX_MOVED_STARTS_SOLID.
 *   Step.  From stand cell a = (x, y, z) to stand cell b = (x', y', z') with |x - x'| + |z - z'| = 1, when -maxDrop <= y' - y <= stepUp and, with
 *     t = max(y, y') + height, B(x, j, z) is false for y <= j < t and B(x', j, z') for y' <= j < t: the body rises in place or falls in the
 *     destination through clear air.  Steps are directed (a cliff may be descended and not climbed); every step costs 1.
 *   Distance.  A goal (gx, gy, gz) RESOLVES to the stand cell (gx, y, gz), y <= gy, with B(gx, j, gz) false for y <= j <= gy -- the floor the body
 *     would fall to -- or to nothing.  distance(c) = the fewest steps from c to any resolved goal; maxSteps > 0 leaves cells farther than that
 *     unreached.  No resolved goal: CVX_OK, nothing reached.
 *   Next.  For a reached cell with distance > 0 the target of a step with distance - 1: the first direction in the order -X, +X, -Z, +Z that has
 *     one, and in it the highest y'.  At a goal the cell itself.
 * The whole field is a function of the world and the arguments: no schedule and no goal order shows in it.  What the device computes: per cell
 * column the maximal air intervals [lo, hi) of the union of its width x width arena columns (the topmost open upwards); an interval with
 * hi - lo >= height and y0 <= lo < y1 is a NODE with stand cell (x, lo, z); a step a -> b exists iff -maxDrop <= lo_b - lo_a <= stepUp and
 * min(hi_a, hi_b) >= max(lo_a, lo_b) + height; distances by relaxation to the unique fixpoint.
 * A query position resolves exactly as a goal does: an airborne agent gets the floor below it; a position in solid, outside the cell grid or
 * over an interval too low for the body gets no cell.  cvx_nav_field_goals keeps the nodes and steps and solves for new goals (the player
 * moved).  The field is a SNAPSHOT: later edits do not change it, the host rebuilds after an edit.  It owns its device memory and must be
 * destroyed before its context; destroying NULL is a no-op.  `goals` and `cells` hold three int32 per entry.
 * `summary` (may be NULL): nodes, reached nodes, the goals that resolved (entries, duplicates included), the largest distance of a reached
 * node (0: none), the cell columns with two or more nodes, and the relax launches made (informative: not part of the deterministic result).
 * Ordering as cvx_world_pieces / cvx_world_move: build and _goals are ordered on the context's stream behind everything enqueued before them
 * (build places unplaced levels first) and return when the summary is on the host; cvx_nav_query returns when the steps are copied back;
 * cvx_nav_query_device enqueues on hipStream (NULL = the context's) without waiting.  outDeviceMs (may be NULL): device time of the call.
 * Errors, all checked on the host before anything is enqueued; a failing build leaves *outField NULL and frees everything.
 * CVX_ERR_INVALID_ARGUMENT: NULL pointers, boxMin >= boxMax on an axis, a box wholly outside the world, width outside 1 .. 8, height outside
 * 1 .. 64, stepUp outside 0 .. height, maxDrop outside 0 .. 4096, a negative maxSteps, goalCount outside 1 .. CVX_NAV_MAX_GOALS, a negative
 * count, a field of another context; CVX_ERR_NOT_READY: LOD 0 has not been uploaded; CVX_ERR_CAPACITY: the tables do not fit in device memory,
 * or 2^31 or more cell columns or nodes.  The device query cannot validate its input: a position that resolves to nothing gets no cell, and every
 * loop of it is bounded by the column's node count whatever the input.
 * Device memory of a field: 4 bytes per cell column and 16 bytes per node (its interval, distance and next); a build adds the count scan's
 * scratch while it runs (8 bytes per chunk of columns), _goals 12 bytes per goal, and cvx_nav_query 44 bytes per position. */
#define CVX_NAV_MAX_GOALS 4096
typedef struct cvx_nav_params {   /* 48 bytes */
	int32_t boxMin[3], boxMax[3]; /* LOD-0 voxels, inclusive / exclusive */
	int32_t width;                /* 1 .. 8   footprint, voxels, square */
	int32_t height;               /* 1 .. 64 */
	int32_t stepUp;               /* 0 .. height */
	int32_t maxDrop;              /* 0 .. 4096 */
	int32_t maxSteps;             /* 0: no bound */
	int32_t pad_;
} cvx_nav_params;
typedef struct cvx_nav_step {     /* 32 bytes */
	int32_t cell[3];              /* the stand cell the queried position resolves to; {-1,-1,-1}: none */
	int32_t distance;             /* steps to the nearest goal; -1: no cell or unreached */
	int32_t next[3];              /* the cell to step to (own cell at a goal); {-1,-1,-1} when distance < 0 */
	int32_t direction;            /* 0,1,4,5 = -X,+X,-Z,+Z (the pick's face numbers); -1: at a goal or distance < 0 */
} cvx_nav_step;
typedef struct cvx_nav_summary {  /* 40 bytes */
	int64_t nodes, reached;
	int32_t goalsResolved, largestDistance;
	int64_t columnsWithSeveralNodes;
	int32_t launches, pad_;       /* relax launches made: informative, not part of the deterministic result */
} cvx_nav_summary;
typedef struct cvx_nav_field cvx_nav_field;
int  cvx_world_nav_build(cvx_context *ctx, const cvx_nav_params *params, const int32_t *goals, int goalCount,
                         cvx_nav_field **outField, cvx_nav_summary *summary, float *outDeviceMs);
int  cvx_nav_field_goals(cvx_context *ctx, cvx_nav_field *field, const int32_t *goals, int goalCount, int maxSteps,
                         cvx_nav_summary *summary, float *outDeviceMs);
int  cvx_nav_query(cvx_context *ctx, const cvx_nav_field *field, int count, const int32_t *cells, cvx_nav_step *steps);
int  cvx_nav_query_device(cvx_context *ctx, const cvx_nav_field *field, int count, const int32_t *cellsDevice,
                          cvx_nav_step *stepsDevice, void *hipStream);
void cvx_nav_field_destroy(cvx_nav_field *field);

/* ---- the exposed faces of the uploaded world as coloured quads ---------------------------------------------------------------------------------
 * cvx_world_surface: the inverse of cvx_world_stamp_mesh -- a surface out of the edited world, for a physics engine's collision mesh, a
 * rasterised preview or minimap, an OBJ export, an overlay of what a brush changed.  The rule is exact integers in LOD-0 voxels of the stored
 * tile (a repeating world does not wrap the coordinates); the call only reads the arena.
 *   Box.  The voxels considered are the solid voxels of LOD 0 inside [boxMin, boxMax) after clipping the box to the world.
 *   Across a face.  Faces are numbered as the pick numbers them: 0..5 = -X,+X,-Y,+Y,-Z,+Z.  The voxel across face f of voxel v is read from the
 *     arena whenever it lies inside the world, inside the box or not: the meshes of adjacent boxes tile, no face appears twice and none is
 *     missing at the seam.  Outside the world it is solid iff bit f of solidOutside is set; CVX_SURFACE_OUTSIDE_DEFAULT makes the ground below
 *     y = 0 solid and everything else air, above dimY too.
 *   Exposed.  Face f of a solid voxel is exposed when the voxel across it is air.
 *   Quads.  For a side face (f = 0, 1, 4, 5) a quad is a maximal vertical run of voxels of one column inside the box's y range that all have
 *     face f exposed and all carry the same colour word (the arena's ARGB word, as cvx_world_pick reports it); how the column is encoded does
 *     not show: a span split into two runs still gives one quad.  With CVX_SURFACE_IGNORE_COLOUR colour does not end a run and the quad carries
 *     the colour of its top voxel: the collision mesh.  For f = 2, 3: one quad of length 1 per exposed voxel face.
 *   Order.  Ascending x, then ascending z, then ascending face, then DESCENDING y of the quad's top.  The list is a function of the world and
 *     the arguments: the same call twice gives the same bytes.
 * `summary` (may be NULL): the total number of quads, the sum of their lengths (= the exposed voxel faces) and the quads per face, whatever
 * the capacity.  `quads` receives the first min(quadCapacity, summary.quads) quads; a smaller capacity is not an error, and capacity 0 with
 * quads NULL is the way to ask for the count.  outDeviceMs (may be NULL): device time of the call.
 * cvx_world_surface is ordered on the context's stream behind everything enqueued before it, places unplaced levels first (as
 * cvx_world_pieces does) and returns when the results are on the host.  cvx_world_surface_device leaves the quads in quadsDevice (device
 * memory of quadCapacity entries; entries at and beyond min(quadCapacity, summary.quads) are not written); the summary still comes to the host
 * and the call still waits for it.
 * cvx_surface_triangles is a pure host function (no context, no device): four vertices and six indices per quad, quad k's vertices 4k .. 4k+3
 * indexed 0,1,2, 0,2,3.  The corners are those of the quad's rectangle on its face plane -- face 0 on X = x, face 1 on X = x + 1, both
 * spanning z .. z + 1 and y .. y + length; faces 2 / 3 on Y = y / Y = y + 1; faces 4 / 5 on Z = z / Z = z + 1 -- ordered so that
 * (v1 - v0) x (v2 - v0) points along the face's outward axis.  rgba is the vertex colour for which cvx_world_stamp_mesh writes exactly the
 * quad's colour word (alpha is ignored: 255); uv is 0 and material -1.  CVX_ERR_INVALID_ARGUMENT: a negative count, a NULL pointer with a
 * count above 0, 2^29 or more quads, a face outside 0 .. 5.
 * Errors of the two world calls, all checked on the host before anything is enqueued.  CVX_ERR_INVALID_ARGUMENT: a NULL box, boxMin >= boxMax
 * on an axis, a box wholly outside the world, solidOutside bits above 0x3F, unknown flag bits, a negative capacity, quads NULL with a capacity
 * above 0; CVX_ERR_NOT_READY: LOD 0 has not been uploaded; CVX_ERR_CAPACITY: the scratch does not fit in device memory, or the box holds 2^31
 * or more (column, face) pairs or quads.  Device memory while it runs: 24 bytes per column of the clipped box (a count per face) and 8 bytes
 * per 4096 (column, face) pairs for the scan; cvx_world_surface adds 24 bytes per quad it returns. */
#define CVX_SURFACE_OUTSIDE_DEFAULT 0x04   /* -Y: the ground below y = 0 is solid, everything else outside the world is air */
enum { CVX_SURFACE_IGNORE_COLOUR = 1 };    /* flags */
typedef struct cvx_surface_quad {  /* 24 bytes */
	int32_t voxel[3];  /* the quad's lowest voxel */
	int32_t face;      /* 0..5 = -X,+X,-Y,+Y,-Z,+Z */
	int32_t length;    /* voxels along +Y; 1 for the -Y / +Y faces */
	uint32_t argb;     /* the colour word */
} cvx_surface_quad;
typedef struct cvx_surface_summary {  /* 64 bytes */
	int64_t quads;            /* total quads */
	int64_t unitFaces;        /* the sum of their lengths: the exposed voxel faces */
	int64_t quadsPerFace[6];
} cvx_surface_summary;
int cvx_world_surface(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags,
                      cvx_surface_quad *quads, int64_t quadCapacity, cvx_surface_summary *summary, float *outDeviceMs);
int cvx_world_surface_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int solidOutside, int flags,
                             cvx_surface_quad *quadsDevice, int64_t quadCapacity, cvx_surface_summary *summary, float *outDeviceMs);
int cvx_surface_triangles(const cvx_surface_quad *quads, int64_t quadCount, cvx_mesh_vertex *vertices, int32_t *indices);

/* ---- dense voxel boxes in and out of the uploaded world --------------------------------------------------------------------------------------
 * cvx_world_read_voxels / cvx_world_write_voxels: the world as everything outside this library holds voxels, a plain 3-D array -- terrain made
 * by the caller's own kernels or torch ops, an imported volume, a prefab that is not in the world yet, the input of a simulation step or a model,
 * an undo buffer that stays on the device.  No RLE columns are encoded or decoded on the host.
 *   Box and layout.  Coordinates are LOD-0 voxels of the stored tile: a repeating world does not wrap them.  The box is [boxMin, boxMax) with
 *     size s = boxMax - boxMin > 0 per axis, every |coordinate| <= 2^30 and s.x * s.y * s.z < 2^31; it may stick out of the world on any side.
 *     Voxel (x, y, z) of the box is element ((x - boxMin.x) * s.z + (z - boxMin.z)) * s.y + (y - boxMin.y) of the arrays: the world's column
 *     order (x, then z) with y ascending and fastest.  A C-contiguous array (a torch tensor) of shape (X, Z, Y) maps onto it directly.
 *   Read.  solid[i] is 1 for a solid voxel, else 0; argb[i] is the arena's colour word of a solid voxel, as cvx_world_pick reports it, and 0 for
 *     air and for everything outside the world.  Either pointer may be NULL, not both.  The call only reads the arena and places unplaced levels
 *     first (as cvx_world_surface does).  cvx_world_read_voxels takes host arrays, is ordered on the context's stream behind everything enqueued
 *     before it and returns when the data is on the host; outDeviceMs (may be NULL): device time of the kernel.  cvx_world_read_voxels_device
 *     takes device arrays and enqueues on hipStream (NULL = the context's stream) without waiting; the caller orders that stream after the
 *     context's work (cvx_world_pick_device's words).
 *   Write.  A box voxel is SET iff solid[i] != 0 when `solid` is given, else iff argb[i] != 0; with a mask a set voxel may carry colour word 0.
 *     Colour words are stored verbatim.  argb may be NULL only for CVX_BRUSH_CARVE, which then requires `solid`.  Let W be LOD 0 before the
 *     call; for every box voxel v inside the world the op decides R(v): CVX_COPY_REPLACE R(v) = set ? solid(argb[i]) : air; CVX_BRUSH_FILL: set
 *     -> R(v) = solid(argb[i]), solid voxels included; CVX_BRUSH_CARVE: set -> R(v) = air; CVX_BRUSH_PAINT: set and W(v) solid -> R(v) takes
 *     argb[i].  Everything else is W.  The call edits the box's XZ footprint clipped to the world, rounded outward to multiples of 2^levelCount
 *     and clipped again (cvx_world_brush's rectangle), and rebuilds LOD 1 .. levelCount (0 .. 5); columns of the rectangle outside the footprint
 *     are re-encoded with the builder's rule, as the brush does (unchanged for every world the builder made); runs that come to touch merge
 *     across the box's top and bottom.  A box that lies wholly outside the world (on any axis): CVX_OK, nothing is written, *outDeviceMs = 0.
 *     Ordering, atomicity, outDeviceMs, CVX_ERR_CAPACITY (the brush's format limits, the arena limits) and CVX_ERR_NOT_READY are
 *     cvx_world_brush's; every error leaves the world as it was.  cvx_world_write_voxels_device reads its device arrays on the context's stream:
 *     the caller makes sure they are complete when it calls and leaves them alone until it returns (like the host call, when the edit is done).
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued: NULL box pointers, an empty box, a coordinate beyond 2^30,
 * 2^31 or more voxels, a bad op, levelCount outside 0 .. 5, both arrays NULL on a read, argb NULL on a write unless the op is CARVE with `solid`
 * given.  Device memory while a call runs: the host-array calls hold the box's arrays (4 bytes per voxel for argb, 1 for solid); a write adds
 * cvx_world_brush's scratch for its rectangle, 4 more bytes per column of it (the run counts) and the rectangle's new columns.  The device calls
 * of a read take none.  With several GPUs every rank applies the same write to its own context. */
int cvx_world_read_voxels(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], uint32_t *argb, uint8_t *solid, float *outDeviceMs);
int cvx_world_read_voxels_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], uint32_t *argbDevice, uint8_t *solidDevice,
                                 void *hipStream);
int cvx_world_write_voxels(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const uint32_t *argb, const uint8_t *solid, int op,
                           int levelCount, float *outDeviceMs);
int cvx_world_write_voxels_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], const uint32_t *argbDevice,
                                  const uint8_t *solidDevice, int op, int levelCount, float *outDeviceMs);

/* ---- exact squared-distance fields of boxes of the uploaded world -----------------------------------------------------------------------------
 * cvx_world_distance: how far every voxel of a box is from the nearest solid (or air) voxel -- sphere and capsule collision for particles and
 * projectiles, clearance for AI and camera placement, contact shadows, fog that hugs the terrain, outlines, and the editor's grow, shrink, round
 * off and shell: thresholds of the field written back through cvx_world_write_voxels.  The rule is exact integers in LOD-0 voxels of the stored
 * tile (a repeating world does not wrap the coordinates); the calls only read the arena.
 *   Box and layout.  cvx_world_read_voxels': the box is [boxMin, boxMax) with size s = boxMax - boxMin > 0 per axis, every |coordinate| <= 2^30
 *     and s.x * s.y * s.z < 2^31; it may stick out of the world on any side or lie wholly outside it.  Voxel (x, y, z) of the box is element
 *     ((x - boxMin.x) * s.z + (z - boxMin.z)) * s.y + (y - boxMin.y) of `out`: a C-contiguous int32 array (a torch tensor) of shape (X, Z, Y).
 *   Solid(v).  Inside the world: what the arena holds at LOD 0.  Outside the world: solid iff, on some axis, v lies beyond the world on the side
 *     of face f and bit f of solidOutside is set; faces are numbered as for cvx_world_surface, 0..5 = -X,+X,-Y,+Y,-Z,+Z.
 *     CVX_SURFACE_OUTSIDE_DEFAULT (0x04) makes every voxel with y < 0 solid, an infinite ground, and everything else outside the world air.
 *   Distances.  With R = maxDistance, 1 <= R <= 255: D_S(v) is the minimum of |s - v|^2 (the squared Euclidean distance between voxel centres,
 *     an integer) over all s with Solid(s) and |s - v|^2 <= R^2, CVX_DISTANCE_FAR when there is none; s ranges over all of space, not only over
 *     the box.  D_A(v) is the same over the s with !Solid(s).  CVX_DISTANCE_TO_SOLID: out = D_S(v), 0 on solid voxels; CVX_DISTANCE_TO_AIR:
 *     out = D_A(v), 0 on air voxels; CVX_DISTANCE_SIGNED: out = Solid(v) ? -D_A(v) : D_S(v), -CVX_DISTANCE_FAR deep inside.
 *   The result of a voxel depends on the world and the arguments only, not on the box: the fields of adjacent boxes tile, and the same call
 *     twice gives the same bytes.
 * Both calls are ordered on the context's stream behind everything enqueued before them, place unplaced levels first (as cvx_world_surface
 * does), return when the result is complete and free their scratch before they return.  cvx_world_distance takes a host array;
 * cvx_world_distance_device leaves the field in outDevice (device memory of s.x * s.y * s.z int32).  outDeviceMs (may be NULL): device time of
 * the kernels.
 * CVX_ERR_INVALID_ARGUMENT, all checked on the host before anything is enqueued: NULL pointers, an empty box, a coordinate beyond 2^30, 2^31
 * or more voxels, maxDistance outside 1 .. 255, an unknown mode, solidOutside bits above 0x3F; CVX_ERR_NOT_READY: LOD 0 has not been uploaded;
 * CVX_ERR_CAPACITY: the scratch does not fit in device memory.  Device memory while a call runs: 2 bytes per voxel of the box's XZ footprint
 * grown by R on all four sides times its height (the distances along Y), 2 more per voxel of the footprint grown by R in X only -- together
 * 2 * s.y * (s.x + 2R) * (2 * s.z + 2R) bytes: 4 per voxel of the box, 4 * s.y per halo column of the strips beside it in X, 2 * s.y per halo
 * column of the strips and corners beyond it in Z; cvx_world_distance adds the 4 bytes per voxel of the field itself.  Every mode takes the
 * same. */
#define CVX_DISTANCE_FAR 0x7FFFFFFF
enum { CVX_DISTANCE_TO_SOLID = 0, CVX_DISTANCE_TO_AIR = 1, CVX_DISTANCE_SIGNED = 2 };
int cvx_world_distance(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int maxDistance, int mode, int solidOutside,
                       int32_t *out, float *outDeviceMs);
int cvx_world_distance_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int maxDistance, int mode, int solidOutside,
                              int32_t *outDevice, float *outDeviceMs);

/* ---- reading the uploaded world back, and compacting its arena --------------------------------------------------------------------------
 * After edits and brushes the device holds the only up-to-date copy of the world; these calls bring it back (to save it, or to keep a rectangle
 * for undo) and reclaim the space edits left behind.  Every read-back column is in the builder's encoding (WordBuilder.cs:181-268, what
 * cvx_world_brush emits): maximal runs from the top, the top air run first, air runs with ColorsIndex -1, both guards 0, ColorsIndex of a solid
 * run = the solid voxels above it, worldMin / worldMax as the RLEColumn constructor computes them (World.cs:190-234, LOD-0 voxels), header pad 0,
 * the pool in column order, an all-zero header for an empty column.  The builder and World.DownSample (host and device) produce nothing else, so
 * for every world the host library builds the blob is byte-identical to what was uploaded.  A column uploaded in another encoding (a foreign blob
 * with a split run, split air runs, colour indices that share colours, a column with no solid voxel) comes back with the same voxels and colours
 * in builder form, not byte-identical.
 * The calls are ordered on the context's stream behind every draw, edit and brush enqueued before them; levels uploaded but not placed yet are
 * placed first (what the next draw would do); they return once the copy is done, never change the world and free their scratch before they
 * return.  CVX_ERR_INVALID_ARGUMENT: a NULL out pointer, lod outside 0 .. 5, a rectangle outside the level; CVX_ERR_NOT_READY: the level (or
 * another one of the world) was never uploaded; CVX_ERR_CAPACITY: out of device or host memory, or a blob beyond 2^31 elements.
 * *outStorage is malloc'd: release it with cvx_free. */
/* A rectangle of level `lod` (in that level's own columns) as a sub-world blob: the layout cvx_world_set_columns / cvx_world_edit take and
 * cvxh_world_extract_region makes (column (x, z) is header (x - x0) * sizeZ + (z - z0), *outColumnCount = sizeX * sizeZ). */
int cvx_world_read_region(cvx_context *ctx, int lod, int x0, int z0, int sizeX, int sizeZ, void **outStorage, int64_t *outByteLength, int32_t *outColumnCount);
/* The whole level as cvx_world_upload takes it and cvxh_world_info.storage holds it: *outColumnCount = World.ColumnCount (World.cs:17,
 * dimX * dimZ / (lod + 1)^2), which for lod >= 2 is more headers than the level has columns; the extra trailing headers are zero. */
int cvx_world_read_level(cvx_context *ctx, int lod, void **outStorage, int64_t *outByteLength, int32_t *outColumnCount);
/* Lays every level that has an edit tail out again without the space edits left behind; rendering, picks and read-back are unchanged.  All on the
 * device: per level the colour blocks get the depth their deepest column needs now (a column-after-column level packs its columns), run-list
 * blocks and colours are packed in column order, the records are rewritten to the new places; the level keeps its colour layout, and gets the
 * headroom of a first edit.  Levels never edited are copied as they are; a context that never edited is left alone.  Ordered like the read-back
 * (a CVX_DRAW_ASYNC draw enqueued before the call renders the old world); the call returns once the new arena is in place.  The peak is the old
 * arena plus the new one: CVX_ERR_CAPACITY (out of device memory) leaves the world as it was.  outReclaimedBytes (may be NULL): the drop of
 * cvx_world_edit_stats' used bytes; outDeviceMs (may be NULL): device time of the compaction. */
int cvx_world_compact(cvx_context *ctx, int64_t *outReclaimedBytes, float *outDeviceMs);

const char *cvx_version(void);

#ifdef __cplusplus
}
#endif
#endif
