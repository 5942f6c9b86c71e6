// cvx_context.h -- state and helpers shared by the translation units of libcpuvox_gpu.so (cvx_gpu.hip: context, raybuffers,
// draw / read-back / blit; cvx_world.hip: world validation, upload, LOD construction).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "cpuvox_gpu.h"
#include "cvx_copy.h" // cvxb::CopyWorld
#include "cvx_device.h"

struct RefHeader { // World.RLEColumn, World.cs:161-169
	int32_t storageOffset;
	uint16_t runCount;
	uint16_t worldMin;
	uint16_t worldMax;
};
static_assert(sizeof(RefHeader) == 12, "reference header is 12 bytes");

struct LastDraw { // what read-back / blit need to know about a buffer pair
	bool valid = false;
	cvx_segment_data segments[4];
	float vp[2];
	int tileBase[4];
	int width = 0, height = 0;
};


struct cvx_context {
	int device = 0;
	hipStream_t ownStream = nullptr;
	hipStream_t stream = nullptr;
	// one HIP event pair per draw since the last cvx_draw_time_stats(reset): kernel time on ctx->stream
	std::vector<hipEvent_t> evPairs; // 2 * pairs
	size_t evUsed = 0;               // pairs in use
	double accumulatedMs = 0.0;      // folded-in pairs
	int accumulatedDraws = 0;
	float lastMs = 0.f;
	std::string error;

	// world: every level is laid out on the host by cvx_world_upload (records, run list, element pool) and placed into ONE
	// device arena by the next draw (SyncWorld); levels that were not uploaded again are copied over from the old arena
	struct HostLevel {
		std::vector<uint4> records;     // 1 per column, row-major (cvx_device.h); empty once the level lives in the arena
		std::vector<uint2> runs;        // run list: every solid run of the columns whose record cannot hold them
		std::vector<uint2> counts;      // per column, what only the counting build reads
		std::vector<uint32_t> elements; // the columns' colours in blocks of 4 x 8 columns (cvx_device.h), a line of zeros on both sides
		size_t recordsBytes = 0, runsBytes = 0, countsBytes = 0, elementsBytes = 0;
		bool pending = false;           // host vectors hold data that is not in the arena yet
		int rowShift = 0;
		int colorShift = 7;             // log2 of the bytes between two colours of a column (cvx_device.h)
		int64_t solidColumns = 0, listedColumns = 0; // non-empty columns of the level, and how many of them keep their runs in the run list (code 0)
	};
	HostLevel hostLevel[CVX_LOD_LEVELS];
	uint8_t *arena = nullptr;
	size_t arenaBytes = 0;
	bool levelSet[CVX_LOD_LEVELS] = {};
	DevWorld hostWorld{};
	DevWorld *devWorld = nullptr;
	bool worldDirty = true;
	// in-place edits (cvx_edit.hip): per level, the tail behind the run list and the colours that replaced columns take their places from.  A level
	// gets one on its first edit (the arena is laid out again, with headroom); cvx_world_upload of the level drops it.  The host sizes
	// (HostLevel::runsBytes / elementsBytes) of a level with a tail cover the tail, so that SyncWorld carries it over like any other part.
	struct EditLevel {
		bool ready = false;
		int64_t runsUsed = 0, runsCap = 0;         // run-list entries (uint2) in use / in the region
		int64_t elementsUsed = 0, elementsCap = 0; // colour slots in use / usable; one line of zeros follows the usable ones
		int64_t abandonedBytes = 0;                // places of replaced columns and moved blocks nothing refers to any more
		uint32_t *blockBase = nullptr, *blockDepth = nullptr; // device, colorShift 7: first slot and depth (colours) of every 4 x 8 block
		size_t blockCap = 0;
	};
	EditLevel edit[CVX_LOD_LEVELS];
	// cvx_world_pick (cvx_brush.hip): device copies of the rays and hits of the last call, grown on demand
	void *pickScratch = nullptr;
	size_t pickScratchBytes = 0;

	// raybuffers
	int resX = 0, resY = 0;
	int bufferCount = 2; // RenderManager.BUFFER_COUNT, RenderManager.cs:14
	int tilesTD = 0, tilesLR = 0;
	size_t poolBytesTD = 0, poolBytesLR = 0;
	std::vector<uint32_t *> poolTD, poolLR; // per buffer: offsets into one allocation each
	uint32_t *poolBaseTD = nullptr, *poolBaseLR = nullptr;
	bool poolsExternal = false;
	std::vector<LastDraw> last;
	uint32_t *screen = nullptr;
	uint32_t *screenBatch = nullptr; // cvx_blit_segments_batch without a caller buffer: screenBatchFrames images, grown on demand
	int screenBatchFrames = 0;
	void *blitParamsDev = nullptr;   // BlitParams of a batch (device) + their pinned staging copy
	void *blitParamsPinned = nullptr;
	int blitParamsCapacity = 0;
	uint32_t *staging = nullptr;
	size_t stagingBytes = 0;

	// per-draw scratch (grown on demand, reused)
	DevFrame *devFrames = nullptr;
	size_t devFramesCap = 0;
	DevTile *devTiles = nullptr;
	size_t devTilesCap = 0;
	struct UploadSlot {
		void *pinned = nullptr;
		size_t bytes = 0;
		hipEvent_t done = nullptr;
		bool inFlight = false;
	};
	static constexpr int kUploadSlots = 3;
	UploadSlot upload[kUploadSlots];
	unsigned uploadNext = 0;
	std::vector<DevFrame> hostFrames;
	std::vector<DevTile> hostTiles;
	std::vector<float> hostTileCost; // estimated DDA steps of the tile's middle ray (launch order: longest first)
	std::vector<int> hostTileWords;  // LDS mask words per lane the tile needs
	int maskWordsNeeded = 1;         // LDS mask words per lane of the widest [origMin, origMax] window in the current launch
	int ldsWordsNeeded = CVX_WAVE;   // LDS words (mask words x lanes) of the largest wave of the current launch
	int maxWaveMaskWords = 40 * CVX_WAVE; // LDS budget per wave: 10 KB = 16 waves per CU; wider tiles are cut into narrower waves
	bool maxWaveMaskWordsAuto = true;     // ... chosen per launch by DrawBatch's cost model unless CVX_MAX_WAVE_MASK_WORDS pins it

	int lonePixels = 0;              // lone_kernel: pixels of the longest window [origMin, origMax] of the launch (its LDS row)
	int launchLone = 0;              // the current launch goes to lone_kernel (cvx_lone.h): 1 = one mask register, 2 = two (windows of more than 2048 pixels)
#ifndef CVX_LONE_DEFAULT_MODE
#define CVX_LONE_DEFAULT_MODE 1
#endif
	int loneMode = CVX_LONE_DEFAULT_MODE; // 1: lone_kernel for launches of at most loneWaveBudget rays; 0 never, 2 always (experiment build: CVX_LONE=0 / 1; variants: -DCVX_LONE_DEFAULT_MODE)
	int worldRepeat = 0;             // cvx_set_world_repeat: 1 = the world repeats in X and Z (draws and picks enqueued from then on), 0 = bounded
	int loneWaveBudget = 12288;      // AUTO: launches of up to this many rays (= waves, tiles x 64) go to lone_kernel: 2 - 3 frames at 1080p; three quarters of it above
	                                 // 2560 x 1440 (4K: frames of up to ~9 000 rays).  Budget sweep over launches of 2 - 6 frames, per-pose crossover at 4K: profiles/r06_latency.md

	int shardIndex = 0, shardCount = 1;
	bool countersEnabled = false;
	DevCounters *devCounters = nullptr;
	int splitWaveBudget = 4096;                // DrawBatch cuts tiles into sub-tiles while the launch stays below this many waves
	int forcedSplit = 0;                       // CVX_TILE_SPLIT=1|2|...|64 (diagnostics): fixed split factor
	float tileCostPixelWeight = 0.f;           // launch-order estimate += weight * pixels of the tile's window (CVX_TILE_COST_PIXELS, diagnostics)
	bool tileCostMiddleRay = false;            // CVX_TILE_COST_MIDDLE_RAY=1 (diagnostics): estimate from the tile's middle ray instead of its longer edge ray
	int minMaskWords = 0;                      // CVX_MIN_MASK_WORDS (diagnostics): lower bound of the LDS mask words per lane, i.e. an occupancy cap
#ifdef CVX_EXPERIMENTS
	int64_t lastLaunch[8] = { -1, 0, 0, 0, 0, 0, 0, 0 }; // cvx_debug_last_launch (include/cpuvox_gpu_diag.h): the shape of the last draw's launch
#endif
};

namespace cvxi {

// Records the message on the context (or for cvx_last_error(NULL) when ctx is null) and returns `code`.
int Fail(cvx_context *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

inline bool IsPow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// The runtime calls DeviceCall makes, as a table, so that its ownership rules compile and run without a device (tests/device_call_rules.cpp)
struct DeviceApi {
	hipError_t (*malloc)(void **, size_t);
	hipError_t (*free)(void *);
	hipError_t (*eventCreate)(hipEvent_t *);
	hipError_t (*eventRecord)(hipEvent_t, hipStream_t);
	hipError_t (*eventDestroy)(hipEvent_t);
	hipError_t (*eventElapsedTime)(float *, hipEvent_t, hipEvent_t);
	hipError_t (*getLastError)();
	const char *(*getErrorString)(hipError_t);
};
const DeviceApi &HipApi(); // cvx_gpu.hip: the HIP runtime

// What one world call borrows from the device -- its scratch blocks and the event pair around its work on ctx->stream -- given back by the
// destructor on every path.  It owns nothing of the context's lifetime (the arena, the buffers grown on demand, the draw-time event pairs).
class DeviceCall {
public:
	static constexpr int kBlocks = 24; // (the mesh stamp holds 19; every other call five at the most)

	DeviceCall(cvx_context *ctx, const char *call) : DeviceCall(ctx, call, ctx->stream, HipApi()) {}
	DeviceCall(cvx_context *ctx, const char *call, hipStream_t stream, const DeviceApi &api) : ctx(ctx), call(call), stream(stream), api(api) {}
	DeviceCall(const DeviceCall &) = delete;
	DeviceCall &operator=(const DeviceCall &) = delete;
	~DeviceCall()
	{
		for (int i = 0; i < blockCount; i++) { if (blocks[i]) { (void)api.free(blocks[i]); } }
		if (ev[0] && !adopted) { (void)api.eventDestroy(ev[0]); }
		if (ev[1]) { (void)api.eventDestroy(ev[1]); }
	}

	// Creates the event pair and records the first event on the stream.  With `start`, an event the caller recorded earlier and goes on
	// owning, only the second event is created.
	hipError_t Begin(hipEvent_t start = nullptr)
	{
		adopted = start != nullptr;
		ev[0] = start;
		hipError_t e = adopted ? hipSuccess : api.eventCreate(&ev[0]);
		if (e == hipSuccess) { e = api.eventCreate(&ev[1]); }
		if (e == hipSuccess && !adopted) { e = api.eventRecord(ev[0], stream); }
		return e;
	}
	// `bytes` of device memory that the destructor frees
	template <class T> hipError_t Allocate(T **out, size_t bytes)
	{
		*out = nullptr;
		if (blockCount == kBlocks) { return hipErrorInvalidValue; }
		void *p = nullptr;
		const hipError_t e = api.malloc(&p, bytes);
		if (e == hipSuccess) {
			blocks[blockCount++] = p;
			*out = static_cast<T *>(p);
		} else {
			failedBytes = bytes;
		}
		return e;
	}
	// `bytes` of host memory for a copy back.  What a copy names must outlive the device blocks (freeing those waits for a copy still under way):
	// a member, destroyed behind the destructor's body
	void *Host(size_t bytes) { return host.resize(bytes), host.data(); }
	// Hands the block to the caller: the destructor no longer frees it
	template <class T> T *Keep(T *block)
	{
		for (int i = 0; i < blockCount; i++) { if (blocks[i] == block) { blocks[i] = nullptr; } }
		return block;
	}
	// Records the second event on the stream
	hipError_t End() { return api.eventRecord(ev[1], stream); }
	// The pair's events, for a caller that records one itself or hands its start on (EditFromDevice's `done`, cvxnav::Solve's `start`)
	hipEvent_t Event(int which) const { return ev[which]; }
	// Device milliseconds between the two events once the stream has run both; 0 if the runtime cannot tell
	float Ms() const
	{
		float ms = 0.f;
		return ev[1] && api.eventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess ? ms : 0.f;
	}
	// The failure path of a world call: hipErrorOutOfMemory clears the thread's last error (hipGetLastError keeps returning it otherwise,
	// also to the next call's launch checks) and returns oomCode, anything else is CVX_ERR_HIP "<call> failed: <error>"
	int Fail(hipError_t e, int oomCode = CVX_ERR_CAPACITY)
	{
		if (e != hipErrorOutOfMemory) { return cvxi::Fail(ctx, CVX_ERR_HIP, "%s failed: %s", call, api.getErrorString(e)); }
		(void)api.getLastError();
		if (failedBytes) { return cvxi::Fail(ctx, oomCode, "%s: out of device memory (an allocation of %zu bytes)", call, failedBytes); }
		return cvxi::Fail(ctx, oomCode, "%s: out of device memory", call);
	}

private:
	cvx_context *ctx;
	const char *call;
	hipStream_t stream;
	const DeviceApi &api;
	void *blocks[kBlocks];
	int blockCount = 0;
	hipEvent_t ev[2] = { nullptr, nullptr };
	bool adopted = false;
	size_t failedBytes = 0;
	std::vector<uint8_t> host;
};

// the world calls' kernels: a thread per column, node or pair, kThreads to a workgroup (`per`: what a workgroup takes where that is not a thread's share)
constexpr unsigned kThreads = 256;
inline unsigned Grid(size_t n, unsigned per = kThreads) { return (unsigned)((n + per - 1) / per); }

// The layout of one scratch allocation: layout(b) is the offset of the next b bytes, every offset a multiple of 16; `bytes` is what to allocate.
struct ScratchLayout {
	size_t bytes = 0;
	size_t operator()(size_t b)
	{
		const size_t at = bytes;
		bytes = (bytes + b + 15) & ~(size_t)15;
		return at;
	}
};

#ifdef __HIPCC__
__device__ inline uint32_t Load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, typename F> __device__ inline T WaveReduce(T v, F f)
{
	for (int d = 32; d > 0; d >>= 1) { v = f(v, __shfl_xor(v, d, 64)); }
	return v;
}

__device__ __forceinline__ uint32_t LanesBelow(uint64_t mask) // the set bits of `mask` below this lane
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The `Uniform` of the rules' wave-side job builders (cvxb::ModelsLaneVoxel, ContactsColumnJobOf, PairBodyJobOf, ModelPickBodyOf): the value is the
// same in every lane, keep it in a scalar register
struct WaveUniform {
	__device__ __forceinline__ int32_t operator()(int32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
	__device__ __forceinline__ float operator()(float v) const { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
	__device__ __forceinline__ double operator()(double v) const
	{
		const unsigned long long w = (unsigned long long)__double_as_longlong(v);
		return __longlong_as_double((long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(w >> 32)) << 32) |
		                                        (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)w)));
	}
};

// The waves of a launch of `wavesPerGroup` waves a workgroup take jobs 0 .. count - 1 in turn (a launch has at most so many workgroups, whatever
// the jobs): f(job, lane), the job in scalar registers and as the loop's own 64-bit counter -- narrowed here, before the call, it cost the write
// walks of the contacts scalar registers (profiles/model_calls_refactor.md); the callers narrow it where they use it.
template <class F> __device__ __forceinline__ void ForEachWaveJob(uint32_t count, int wavesPerGroup, F f)
{
	const uint32_t waves = gridDim.x * (uint32_t)wavesPerGroup;
	const int lane = (int)(threadIdx.x % CVX_WAVE);
	for (uint64_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wavesPerGroup + threadIdx.x / CVX_WAVE)); at < count; at += waves) { f(at, lane); }
}
#endif

// One column of a world blob in the reference's layout (World.cs:161-209): element range inside the pool, both guards
// present, positive run lengths that fit the column height, colours inside the pool.  Everything the kernels dereference
// later is covered here.  *solidRuns receives the number of solid runs, *colourCount (optional) the number of colours the runs address.
int ValidateColumn(cvx_context *ctx, int64_t i, const RefHeader &h, const uint32_t *elements, int64_t elementCount, int maxY, size_t *solidRuns, int64_t *colourCount = nullptr);

// cvx_lone.hip (its own translation unit: the latency kernel is compiled with its own optimisation level, Makefile): launches lone_kernel<hi> (repeat:
// lone_repeat_kernel<hi>) with one workgroup per ray (rays = 64 x tiles), `ldsBytes` of dynamic LDS (merge buffer + the ray's pixel row)
void LaunchLone(bool hi, bool repeat, unsigned rays, size_t ldsBytes, hipStream_t stream, const DevFrame *frames, const DevTile *tiles, const DevWorld *world);

// Repeating worlds (cvx_set_world_repeat): far clip / pick distance bound, and the check of the world's dimensions every draw and pick makes in that mode
// (X and Z at least 2^(LOD levels - 1): wrapping by the level-0 mask keeps the bits NextLOD reads, SegmentDDAData.cs:37, and the LOD blocks tile)
#define CVX_REPEAT_MAX_DISTANCE 1048576.0f
int ValidateRepeat(cvx_context *ctx);

// cvx_gpu.hip: lays the uploaded levels out in the arena if any is pending (what the next draw would do first)
int SyncWorld(cvx_context *ctx);
// cvx_gpu.hip: the world gate of a call that reads the arena.  RequireWorld is the last of its argument checks: CVX_ERR_NOT_READY until LOD 0 has been
// uploaded.  PrepareWorld makes the context's device current and lays the arena out (SyncWorld).  Two functions: the capacity checks that need the
// world's dimensions run between them, and a refusal must leave the device alone.
int RequireWorld(cvx_context *ctx);
int PrepareWorld(cvx_context *ctx);
// cvx_gpu.hip: LOD 0 of the arena as the kernels of the world calls read it (cvx_copy.h); valid from SyncWorld to the next call that lays the arena out again
cvxb::CopyWorld WorldOf(const cvx_context *ctx);
// cvx_world.hip: exclusive prefix sum of n counts in place on `stream`, *total (device) = their sum; chunkSums: (n + CVX_SCAN_CHUNK - 1) / CVX_SCAN_CHUNK words of 8 bytes
void ExclusiveScan(hipStream_t stream, uint32_t *values, int n, unsigned long long *chunkSums, unsigned long long *total);
int ScanChunk();
// cvx_world.hip: World.DownSample(1 .. levelCount) of a validated LOD-0 blob at dSrc (device) that STAYS on the device: headers[j - 1] / elements[j - 1]
// = level j (hipFree them), columnsZ as in the blob (dimZ >> j)
int BuildLodChainOnDevice(cvx_context *ctx, const uint8_t *dSrc, int64_t elementsOfColumns, int dimX, int dimY, int dimZ, int columnCount, int levelCount,
                          uint32_t **headers, uint32_t **elements);
// cvx_readback.hip: the device half of a read-back -- count, scan, write into a device blob -- in two steps around the caller's ONE
// synchronisation, so that a caller with several rectangles (a snapshot's levels) brings all totals back at once.  The rectangle of level `lod`
// is validated and the world laid out (SyncWorld).
struct RegionRead {
	int lod, x0, z0, sizeX, sizeZ;
	uint32_t *offsets;        // RegionReadCount: per column its elements, scanned into offsets (in D's scratch)
	unsigned long long total; // ... and their sum, valid once the stream has run the copy RegionReadCount enqueues: R must not move until then
};
// Allocates the scratch from D, enqueues the count, the scan and the copy of the total to R->total.  Does not wait.
hipError_t RegionReadCount(cvx_context *ctx, DeviceCall &D, RegionRead *R);
// Enqueues the write of the rectangle's headers to dBlob and of its element pool (R.total elements) to dBlob + headerBytes.  Does not wait.
hipError_t RegionReadWrite(cvx_context *ctx, const RegionRead &R, uint8_t *dBlob, size_t headerBytes);
// cvx_edit.hip: releases the edit state's device tables (cvx_destroy)
void FreeEditState(cvx_context *ctx);
// cvx_edit.hip: cvx_world_edit behind its host validation and upload, for a valid sub-world blob already on the device at dSrc (cvx_world_brush
// builds one there): World.DownSample of it into LOD 1 .. levelCount and the patch of every level.  `done` (may be null): recorded behind the last
// patch.  Returns once the stream has run it.
int EditFromDevice(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, const uint8_t *dSrc, int64_t elementsOfColumns, int columnCount, int levelCount,
                   hipEvent_t done);
// cvx_edit.hip: the tail of EditFromDevice alone, for a caller that holds every level already (a snapshot's restore): the patch of LOD 0 ..
// levelCount over (rectangle >> level) from valid blobs on the device, headers[l] / elements[l] = level l; nothing is downsampled.  `done` and the
// return as EditFromDevice.
int PatchLevelsFromDevice(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, const uint32_t *const *headers, const uint32_t *const *elements, int levelCount,
                          hipEvent_t done);

// ---- the column-edit pipeline (cvx_edit.hip): what every call that builds its sub-world blob on the device goes through ----
// The LOD-0 rectangle of an edit: n = sizeX * sizeZ columns, aligned to 2^levelCount
struct EditRectangle {
	int x0, z0, sizeX, sizeZ, n;
};
// Rounds the footprint [x0, x1) x [z0, z1) (inside the world) out to 2^levelCount and clips it to the world.  Fails with CVX_ERR_INVALID_ARGUMENT
// when the world is too narrow for that rounding and with CVX_ERR_CAPACITY ("<what> %d x %d columns", e.g. "a brush over") when the headers of
// that many columns would not fit the blob.
int RoundEditRectangle(cvx_context *ctx, int64_t x0, int64_t x1, int64_t z0, int64_t z1, int levelCount, const char *what, EditRectangle *out);

// What ColumnEdit owns and hands to the caller's two launchers
struct ColumnEditJob {
	EditRectangle R;
	uint32_t *counts;             // R.n words: the count launcher's kernel leaves every column's elements there, the scan turns them into offsets
	unsigned long long *total;    // device: the scan's total
	unsigned int *overLimit;      // device, zero before the count launcher: its kernel raises it for a column the format cannot hold
	uint8_t *extra;               // ColumnEditCall::extraScratchBytes of the same allocation, 16-byte aligned
	uint32_t *headers, *elements; // the write launcher only: the blob, R.n headers of 3 words and the element pool
};
// A caller that keeps the total and the flag in a device struct of its own (already zeroed) and wants that struct back whole: the ONE copy
// of the pipeline is `bytes` from `from` (device) to `to` (host); the total (8 bytes) and the flag (4 bytes) lie at these byte offsets in both.
struct ColumnEditTotals {
	void *from;
	void *to;
	size_t bytes;
	size_t totalAt, overLimitAt;
};
struct ColumnEditCall {
	const char *call;                      // HIP failures: DeviceCall::Fail under this name ...
	int oomCode;                           // ... with this code for hipErrorOutOfMemory: CVX_ERR_HIP or CVX_ERR_CAPACITY, as the call's header promises
	const char *overLimitSubject;          // "<a brushed column> would need ..." (what the format cannot hold)
	const char *elementsSubject;           // "<the brushed columns> need %llu elements"
	const char *overLimitNote = "";        // appended to the first message
	size_t extraScratchBytes = 0;          // the caller's share of the pipeline's one scratch allocation (strokes, placements, lamps)
	const ColumnEditTotals *totals = nullptr; // null: the pipeline's own pair, zeroed on the stream
	hipEvent_t done = nullptr;             // null: the pipeline times itself, *outMs = device time from its first enqueue to the last patch;
	                                       // else the caller's event, recorded behind the last patch: the caller recorded its start long before and
	                                       // takes the time itself -- ColumnEdit then creates no events and does NOT write *outMs
};
// A reference to a caller's launcher (a lambda: hipError_t(const Job &)) for the length of the call it is handed to: nothing is owned or allocated.
// The launcher enqueues on ctx->stream and returns the first error of its own uploads; launch errors are picked up by the driver that calls it.
template <class Job> class Launcher {
	void *object;
	hipError_t (*invoke)(void *, const Job &);

public:
	template <class F, class = std::enable_if_t<!std::is_same_v<std::decay_t<F>, Launcher>>>
	Launcher(F &&f)
		: object(const_cast<void *>(static_cast<const void *>(&f))),
		  invoke([](void *o, const Job &J) -> hipError_t { return (*static_cast<std::remove_reference_t<F> *>(o))(J); })
	{
	}
	hipError_t operator()(const Job &J) const { return invoke(object, J); }
};
using ColumnEditLauncher = Launcher<ColumnEditJob>;
// cvx_gpu.hip: the relaxations' "relaunch until a launch lowers nothing".  Per round: clears *changed (device), launch(k) enqueues launch k = 0, 1, ..
// on ctx->stream, the word comes back, the stream is synchronised; a launch that leaves it 0 is the last.  Returns the number of launches, or -1
// when `bound` launches did not settle it (the stream is synchronised then).  *error: the first HIP error, which ends the loop as well.
int64_t LaunchUntilUnchanged(cvx_context *ctx, unsigned int *changed, int64_t bound, Launcher<int64_t> launch, hipError_t *error);
// Steps 2 .. 6 of the pipeline (cvx_edit.hip's header) on ctx->stream: scratch, launchCount (its uploads, then its count kernel), cvxi::ExclusiveScan, one
// copy back and one synchronisation, the two capacity checks, the blob's allocation, launchWrite (its write kernel and whatever shades the blob),
// EditFromDevice.  Everything the pipeline allocated is released on every path; nothing in the arena is written before EditFromDevice.
// outMs (may be null) is written only when call.done is null, see there.
int ColumnEdit(cvx_context *ctx, const EditRectangle &R, int levelCount, const ColumnEditCall &call, ColumnEditLauncher launchCount, ColumnEditLauncher launchWrite,
               float *outMs);

// ---- the query drivers (cvx_query_call.hip): what the calls that read the world into a caller's arrays or capped list share ----
// Up to three arrays of a read, each optional: to[k], bytes[k] long, is the caller's (null: not wanted).  The launcher gets where its kernel writes
// array k (null where to[k] is) and the stream to launch on.
struct ReadArraysJob {
	void *array[3];
	hipStream_t stream;
};
// `device`: the arrays are device memory; the launch goes straight through on hipStream (null: ctx->stream), nothing is timed or waited for and
// *outDeviceMs is left alone.  Else: one scratch block for the arrays, the launch on ctx->stream, the timing window closed behind it, a copy per
// array, one synchronisation, then *outDeviceMs.
int ReadArrays(cvx_context *ctx, const char *call, void *const to[3], const size_t bytes[3], bool device, void *hipStream, Launcher<ReadArraysJob> launch,
               float *outDeviceMs);
// The capped list of a call: the world holds `found` items, the caller's `list` (device memory with `device`) takes `capacity` of them
struct ListCall {
	size_t itemBytes;
	unsigned long long found;
	int64_t capacity;
	void *list;
	bool device;
};
struct ListJob {
	void *into;     // device: items 0 .. limit - 1 go here
	uint32_t limit; // min(found, capacity), above 0
};
// The tail of such a call, behind its count inside D's window: launchWrite (not called for an empty list) writes into the caller's device list or a
// staged block that one copy brings to D.Host; D.End(); one synchronisation.  Nothing is handed out before the call can no longer fail: the caller's
// host list is written last here, its summary and time by the caller behind a CVX_OK.
int FinishList(cvx_context *ctx, DeviceCall &D, const ListCall &list, Launcher<ListJob> launchWrite);

// cvx_brush.hip: releases the picking scratch (cvx_destroy)
void FreeBrushState(cvx_context *ctx);
} // namespace cvxi

#define CVX_HIP(ctx, call)                                                                                              \
	do {                                                                                                                \
		hipError_t e_ = (call);                                                                                         \
		if (e_ != hipSuccess) {                                                                                         \
			return cvxi::Fail(ctx, CVX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
		}                                                                                                               \
	} while (0)
