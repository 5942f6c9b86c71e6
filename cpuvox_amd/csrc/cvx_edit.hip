// cvx_edit.hip -- libcpuvox_gpu.so, in-place edits of the device-resident world: cvx_world_set_columns (World.SetVoxelColumn, World.cs:151-159, for a
// rectangle of one level), cvx_world_edit (a LOD-0 rectangle + World.DownSample of it into LOD 1 .. levelCount) and cvx_world_edit_stats.
// See include/cpuvox_gpu.h for the contract, cvx_device.h for the arena and DESIGN.md section 3 for the edit tail.
//
// After SyncWorld the host copies of the tables are gone: an edit is device work on the arena.  Per edited level
//   1. plan   (a thread per replaced column): its record words with the upload's rule (cvx_edit.h), and whether its colours (column-after-column
//             levels) and its run-list block fit the place of the column it replaces -- else a request for tail space;
//             (colour blocks, a thread per 4 x 8 block the rectangle touches) the depth the block needs: deeper than it is -> the whole block moves
//   2. the requests are prefix-scanned into tail offsets; the host reads the totals, and lays the arena out again when a tail is too short
//   3. move   (a workgroup per moving block): the block's colours to its new place, the records of its columns outside the rectangle to it
//   4. write  (a thread per replaced column): colours, run-list block, counts entry, record.
// Nothing is written before step 3, so a failure up to there (validation, capacity) leaves the world as it was.
//
// The calls that build their sub-world on the device (brush, copy, dense write, light, stamp, pieces REMOVE, settle, cavities FILL) share one host
// pipeline, written here beside the cvxi::EditFromDevice it ends with: cvxi::RoundEditRectangle, then cvxi::ColumnEdit --
//   1. the footprint rounded out to 2^levelCount and clipped; a world narrower than that and a rectangle of 2^31 / 12 columns or more are refused
//   2. one scratch allocation (counts, scan sums, {total, overLimit}, the caller's share), two events unless the caller has its own
//   3. the caller's count launcher, cvxi::ExclusiveScan, ONE copy back, ONE synchronisation
//   4. refused: a column the format cannot hold (the flag), 2^31 - 3 n elements or more
//   5. the blob's allocation (n headers of 12 bytes, then the element pool), the caller's write launcher
//   6. cvxi::EditFromDevice; the device time from the two events; everything released on every path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_edit.h"

using cvxi::Fail;

namespace cvxedit {

struct EditArgs {
	uint8_t *arena;
	uint32_t recordsOff, runsOff, countsOff, elementsOff;
	int rowShift, blocked, lod, dimY;
	int usedX, usedZ, blocksZ;
	int x0, z0, sizeX, sizeZ, n;
	int bx0, bz0, bzN, blockCount; // blocks the rectangle touches: bx0 .. bx0 + blockCount / bzN - 1, bz0 .. bz0 + bzN - 1
	const uint32_t *headers;       // sub-world: 3 words per column, rectangle order
	const uint32_t *elements;
	uint4 *rec;                    // scratch, per column: record words without colorsBase / run block
	uint2 *cnt;                    //   counts entry
	uint32_t *colours;             //   colours
	uint32_t *runReq;              //   run-list entries wanted from the tail (-> offset after the scan)
	uint32_t *colReq;              //   colour slots wanted from the tail, column-after-column levels (-> offset)
	uint32_t *flags;               //   1: run block in the tail, 2: colours in the tail
	uint32_t *blockReq;            // per touched block: slots wanted from the tail (-> offset)
	uint32_t *blockNeed;           //   the depth it moves with (0: stays)
	uint32_t *blockBase, *blockDepth;
	unsigned long long *abandoned;
	uint32_t runsTail, elementsTail; // first free run-list entry / colour slot of the tail (write phase)
};

__device__ __forceinline__ uint4 *Records(const EditArgs &A) { return reinterpret_cast<uint4 *>(A.arena + A.recordsOff); }
__device__ __forceinline__ uint32_t *Runs(const EditArgs &A) { return reinterpret_cast<uint32_t *>(A.arena + A.runsOff); }
__device__ __forceinline__ bool InRect(const EditArgs &A, int cx, int cz) { return cx >= A.x0 && cx < A.x0 + A.sizeX && cz >= A.z0 && cz < A.z0 + A.sizeZ; }

// First edit of a colour-block level: every block's base slot and depth, read back from the records (a block with no column keeps base 0: "none yet")
__global__ __launch_bounds__(256) void edit_block_table_kernel(EditArgs A, size_t recordCount)
{
	const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (at >= recordCount) { return; }
	const int cx = (int)(at >> A.rowShift), cz = (int)(at & (((size_t)1 << A.rowShift) - 1));
	if (cz >= A.usedZ) { return; }
	const uint4 r = Records(A)[at];
	if (r.x == 0u) { return; }
	const uint32_t c = cvxe::RecordColours(r.x, r.y, r.z, r.w, Runs(A), A.lod);
	const size_t b = (size_t)(cx / CVX_COLOR_BLOCK_X) * (size_t)A.blocksZ + (size_t)(cz / CVX_COLOR_BLOCK_Z);
	atomicMax(&A.blockDepth[b], c);
	A.blockBase[b] = (r.x & 0x3FFFFFFFu) - (uint32_t)((cx % CVX_COLOR_BLOCK_X) * CVX_COLOR_BLOCK_Z + cz % CVX_COLOR_BLOCK_Z);
}

__global__ __launch_bounds__(256) void edit_plan_columns_kernel(EditArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const uint32_t *h = A.headers + 3 * (size_t)i;
	const cvxe::ColumnWords c = cvxe::BuildColumnWords(h, A.elements, A.lod, A.dimY);
	const bool present = (h[1] & 0xFFFFu) != 0u;
	const uint4 old = Records(A)[((size_t)cx << A.rowShift) + (size_t)cz];
	const uint32_t oldColours = cvxe::RecordColours(old.x, old.y, old.z, old.w, Runs(A), A.lod);
	const uint32_t oldRuns = cvxe::RecordRunEntries(old.x, old.w);
	const uint32_t newRuns = (present && c.code == 0u) ? ((c.solid + 1u) & ~1u) : 0u;
	uint32_t flags = 0, runReq = 0, colReq = 0;
	unsigned long long lost = 0;
	if (newRuns > oldRuns) { runReq = newRuns; flags |= 1u; lost += 8ull * oldRuns; }
	else { lost += 8ull * (oldRuns - newRuns); }
	if (!A.blocked) {
		if (!present) { lost += 4ull * oldColours; }
		else if (old.x != 0u && c.colours <= oldColours) { lost += 4ull * (oldColours - c.colours); }
		else { colReq = c.colours; flags |= 2u; lost += 4ull * oldColours; }
		A.colReq[i] = colReq;
	}
	A.rec[i] = uint4{ c.x, c.y, c.z, c.w };
	A.cnt[i] = uint2{ c.c0, c.c1 };
	A.colours[i] = present ? c.colours : 0u;
	A.runReq[i] = runReq;
	A.flags[i] = flags;
	if (lost) { atomicAdd(A.abandoned, lost); }
}

__global__ __launch_bounds__(256) void edit_plan_blocks_kernel(EditArgs A)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= A.blockCount) { return; }
	const int bx = A.bx0 + t / A.bzN, bz = A.bz0 + t % A.bzN;
	const size_t b = (size_t)bx * (size_t)A.blocksZ + (size_t)bz;
	uint32_t need = 0;
	for (int p = 0; p < CVX_COLOR_STRIDE; p++) {
		const int cx = bx * CVX_COLOR_BLOCK_X + p / CVX_COLOR_BLOCK_Z, cz = bz * CVX_COLOR_BLOCK_Z + p % CVX_COLOR_BLOCK_Z;
		if (cx >= A.usedX || cz >= A.usedZ) { continue; }
		uint32_t c;
		if (InRect(A, cx, cz)) {
			c = A.colours[(size_t)(cx - A.x0) * (size_t)A.sizeZ + (size_t)(cz - A.z0)];
		} else {
			const uint4 r = Records(A)[((size_t)cx << A.rowShift) + (size_t)cz];
			c = cvxe::RecordColours(r.x, r.y, r.z, r.w, Runs(A), A.lod);
		}
		need = max(need, c);
	}
	const uint32_t depth = A.blockDepth[b];
	if (need > depth) {
		A.blockReq[t] = need * CVX_COLOR_STRIDE;
		A.blockNeed[t] = need;
		if (depth) { atomicAdd(A.abandoned, 4ull * CVX_COLOR_STRIDE * depth); }
	} else {
		A.blockReq[t] = 0u;
		A.blockNeed[t] = 0u;
	}
}

// a workgroup per touched block; blocks that stay return at once
__global__ __launch_bounds__(64) void edit_move_blocks_kernel(EditArgs A)
{
	const int t = blockIdx.x;
	const uint32_t need = A.blockNeed[t];
	if (need == 0u) { return; }
	const int bx = A.bx0 + t / A.bzN, bz = A.bz0 + t % A.bzN;
	const size_t b = (size_t)bx * (size_t)A.blocksZ + (size_t)bz;
	const uint32_t oldBase = A.blockBase[b], oldDepth = A.blockDepth[b];
	const uint32_t newBase = A.elementsTail + A.blockReq[t];
	uint32_t *colours = reinterpret_cast<uint32_t *>(A.arena + A.elementsOff);
	if (oldBase != 0u) {
		for (uint32_t q = threadIdx.x; q < oldDepth * CVX_COLOR_STRIDE; q += blockDim.x) { colours[newBase + q] = colours[oldBase + q]; }
	}
	if (threadIdx.x < CVX_COLOR_STRIDE) {
		const int p = threadIdx.x;
		const int cx = bx * CVX_COLOR_BLOCK_X + p / CVX_COLOR_BLOCK_Z, cz = bz * CVX_COLOR_BLOCK_Z + p % CVX_COLOR_BLOCK_Z;
		if (cx < A.usedX && cz < A.usedZ && !InRect(A, cx, cz)) {
			uint4 &r = Records(A)[((size_t)cx << A.rowShift) + (size_t)cz];
			if (r.x != 0u) { r.x = (r.x & 0xC0000000u) | (newBase + (uint32_t)p); }
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		A.blockBase[b] = newBase;
		A.blockDepth[b] = need;
	}
}

__global__ __launch_bounds__(256) void edit_write_columns_kernel(EditArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const size_t at = ((size_t)cx << A.rowShift) + (size_t)cz;
	const uint32_t *h = A.headers + 3 * (size_t)i;
	uint4 *records = Records(A);
	uint2 *counts = reinterpret_cast<uint2 *>(A.arena + A.countsOff);
	const uint32_t runCount = h[1] & 0xFFFFu;
	if (runCount == 0u) {
		records[at] = uint4{ 0u, 0u, 0u, 0u };
		counts[at] = uint2{ 0u, 0u };
		return;
	}
	const uint4 old = records[at];
	uint4 rec = A.rec[i];
	const uint32_t flags = A.flags[i], n = A.colours[i];
	uint32_t colorsBase, stride;
	if (A.blocked) {
		const size_t b = (size_t)(cx / CVX_COLOR_BLOCK_X) * (size_t)A.blocksZ + (size_t)(cz / CVX_COLOR_BLOCK_Z);
		const uint32_t base = A.blockBase[b];
		colorsBase = (base ? base : (uint32_t)CVX_COLOR_STRIDE) + (uint32_t)((cx % CVX_COLOR_BLOCK_X) * CVX_COLOR_BLOCK_Z + cz % CVX_COLOR_BLOCK_Z);
		stride = CVX_COLOR_STRIDE;
	} else {
		colorsBase = (flags & 2u) ? A.elementsTail + A.colReq[i] : (old.x & 0x3FFFFFFFu);
		stride = 1u;
	}
	uint32_t *colours = reinterpret_cast<uint32_t *>(A.arena + A.elementsOff);
	const uint32_t src = h[0] + runCount + 2u;
	for (uint32_t k = 0; k < n; k++) { colours[colorsBase + k * stride] = A.elements[src + k]; }
	if ((rec.x >> 30) == 0u) { // listed: the run-list block
		const uint32_t solid = rec.w;
		uint32_t block = 0u;
		if (solid > 0u) {
			block = (flags & 1u) ? A.runsTail + A.runReq[i] : old.z;
			uint32_t *runs = Runs(A) + 2 * (size_t)block;
			cvxe::BuildListedRuns(h, A.elements, A.lod, A.dimY, runs);
			if (solid & 1u) { runs[2 * solid] = 0u; runs[2 * solid + 1] = 0u; }
		}
		rec.z = block;
	}
	rec.x |= colorsBase;
	records[at] = rec;
	counts[at] = A.cnt[i];
}

} // namespace cvxedit

namespace {

using cvxedit::EditArgs;

constexpr unsigned kThreads = 256;

unsigned Grid(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// one level's share of an edit: the rectangle, its columns on the device, and the plan's totals (its scratch is the call's, ApplyJobs)
struct Job {
	int lod = 0, x0 = 0, z0 = 0, sizeX = 0, sizeZ = 0;
	const uint32_t *headers = nullptr, *elements = nullptr;
	EditArgs A{};
	unsigned long long *totals = nullptr; // device: [0] run entries, [1] colour slots (columns), [2] colour slots (blocks), [3] abandoned bytes, then chunk sums
	unsigned long long host[4] = { 0, 0, 0, 0 };
};

// Validates the columns of a sub-world blob (cvx_world_upload's rules) for a sizeX x sizeZ rectangle; *elementsOfColumns as UploadSourceBlob.
int ValidateRegion(cvx_context *ctx, const void *storage, int64_t byteLength, int columnCount, int64_t columns, int maxY, int64_t *elementsOfColumns)
{
	if (!storage || byteLength < 0) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad storage"); }
	if ((int64_t)columnCount < columns || (int64_t)columnCount * 12 > byteLength) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "columnCount %d inconsistent with the rectangle (%lld columns) / byteLength", columnCount, (long long)columns);
	}
	const int64_t elementCount = (byteLength - (int64_t)columnCount * 12) / 4;
	if (elementCount >= ((int64_t)1 << 31)) { return Fail(ctx, CVX_ERR_CAPACITY, "an element pool of %lld entries", (long long)elementCount); }
	const RefHeader *src = static_cast<const RefHeader *>(storage);
	const uint32_t *elements = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(storage) + (size_t)columnCount * 12);
	*elementsOfColumns = 0;
	for (int64_t i = 0; i < columns; i++) {
		if (src[i].runCount == 0) { continue; }
		size_t solid = 0;
		int64_t colours = 0;
		const int rc = cvxi::ValidateColumn(ctx, i, src[i], elements, elementCount, maxY, &solid, &colours);
		if (rc != CVX_OK) { return rc; }
		*elementsOfColumns += (int64_t)src[i].runCount + 2 + colours;
	}
	return CVX_OK;
}

int CheckRect(cvx_context *ctx, int lod, int x0, int z0, int sizeX, int sizeZ)
{
	const int usedX = ctx->hostWorld.dimX >> lod, usedZ = ctx->hostWorld.dimZ >> lod;
	if (sizeX < 1 || sizeZ < 1 || x0 < 0 || z0 < 0 || (int64_t)x0 + sizeX > usedX || (int64_t)z0 + sizeZ > usedZ) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "rectangle (%d, %d) + %d x %d outside LOD %d's %d x %d columns", x0, z0, sizeX, sizeZ, lod, usedX, usedZ);
	}
	return CVX_OK;
}

// The world must be complete and laid out in the arena before an edit can work on it
int Prepare(cvx_context *ctx)
{
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	return cvxi::PrepareWorld(ctx);
}

// Lays the arena out again with the tails `runsCap` / `elementsCap` for the levels that have (or get) one, by device-to-device copies (SyncWorld's
// layout).  Levels that get a tail for the first time start it behind what the upload placed.
int Relayout(cvx_context *ctx, const bool tail[CVX_LOD_LEVELS], const int64_t needRuns[CVX_LOD_LEVELS], const int64_t needElements[CVX_LOD_LEVELS])
{
	cvx_context::EditLevel next[CVX_LOD_LEVELS];
	size_t runsBytes[CVX_LOD_LEVELS], elementsBytes[CVX_LOD_LEVELS], runsCopy[CVX_LOD_LEVELS], elementsCopy[CVX_LOD_LEVELS];
	for (int i = 0; i < CVX_LOD_LEVELS; i++) {
		const cvx_context::HostLevel &H = ctx->hostLevel[i];
		cvx_context::EditLevel e = ctx->edit[i];
		if (!e.ready && tail[i]) {
			e.ready = true;
			e.runsUsed = e.runsCap = (int64_t)(H.runsBytes / 8);
			e.elementsUsed = e.elementsCap = (int64_t)(H.elementsBytes / 4); // (behind the upload's line of zeros)
			e.abandonedBytes = 0;
		}
		if (e.ready) {
			// headroom: what this edit needs + an eighth of what is in use (at least 64 KiB of colours, 32 KiB of runs)
			if (e.runsUsed + needRuns[i] > e.runsCap || tail[i]) {
				e.runsCap = std::max(e.runsCap, (e.runsUsed + needRuns[i] + std::max<int64_t>(e.runsUsed / 8, 4096) + 1) & ~(int64_t)1);
			}
			if (e.elementsUsed + needElements[i] > e.elementsCap || tail[i]) {
				e.elementsCap = std::max(e.elementsCap, (e.elementsUsed + needElements[i] + std::max<int64_t>(e.elementsUsed / 8, 16384) + 31) & ~(int64_t)31);
			}
			if (e.elementsCap + CVX_COLOR_STRIDE >= ((int64_t)1 << 30)) {
				return Fail(ctx, CVX_ERR_CAPACITY, "LOD %d: %.2f G colour slots after the edit (the records address 2^30)", i, (double)e.elementsCap / 1e9);
			}
			runsBytes[i] = (size_t)e.runsCap * 8;
			elementsBytes[i] = (size_t)(e.elementsCap + CVX_COLOR_STRIDE) * 4; // (a line of zeros behind the tail)
			runsCopy[i] = (size_t)e.runsUsed * 8;
			elementsCopy[i] = (size_t)e.elementsUsed * 4;
		} else {
			runsBytes[i] = runsCopy[i] = H.runsBytes;
			elementsBytes[i] = elementsCopy[i] = H.elementsBytes;
		}
		next[i] = e;
	}
	size_t cursor = 0;
	auto place = [&](size_t bytes) { const size_t at = cursor; cursor = (cursor + bytes + 255) & ~(size_t)255; return at; };
	size_t recordsAt[CVX_LOD_LEVELS], runsAt[CVX_LOD_LEVELS], countsAt[CVX_LOD_LEVELS], elementsAt[CVX_LOD_LEVELS];
	for (int i = 0; i < CVX_LOD_LEVELS; i++) {
		const cvx_context::HostLevel &H = ctx->hostLevel[i];
		const size_t guard = (((size_t)16 << H.rowShift) + 64 + 255) & ~(size_t)255;
		recordsAt[i] = place(guard + H.recordsBytes + guard) + guard;
		runsAt[i] = place(runsBytes[i]);
		countsAt[i] = place(H.countsBytes);
		elementsAt[i] = place(elementsBytes[i]);
	}
	if (cursor >= ((size_t)1 << 32)) {
		return Fail(ctx, CVX_ERR_CAPACITY, "the edited world needs %.2f GiB of device tables: more than the 4 GiB the 32-bit offsets of the kernel can address", (double)cursor / (double)((size_t)1 << 30));
	}
	CVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	cvxi::DeviceCall D(ctx, "the arena layout of the edit");
	uint8_t *arena = nullptr;
	hipError_t e = D.Allocate(&arena, cursor);
	if (e == hipSuccess) { e = hipMemsetAsync(arena, 0, cursor, ctx->stream); }
	for (int i = 0; i < CVX_LOD_LEVELS && e == hipSuccess; i++) {
		const cvx_context::HostLevel &H = ctx->hostLevel[i];
		const DevWorldLevel &old = ctx->hostWorld.level[i];
		e = hipMemcpyAsync(arena + recordsAt[i], ctx->arena + old.recordsOff, H.recordsBytes, hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess) { e = hipMemcpyAsync(arena + runsAt[i], ctx->arena + old.runsOff, runsCopy[i], hipMemcpyDeviceToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(arena + countsAt[i], ctx->arena + old.countsOff, H.countsBytes, hipMemcpyDeviceToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(arena + elementsAt[i], ctx->arena + old.elementsOff, elementsCopy[i], hipMemcpyDeviceToDevice, ctx->stream); }
	}
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	(void)hipFree(ctx->arena);
	ctx->arena = D.Keep(arena);
	ctx->arenaBytes = cursor;
	ctx->hostWorld.arena = arena;
	for (int i = 0; i < CVX_LOD_LEVELS; i++) {
		cvx_context::HostLevel &H = ctx->hostLevel[i];
		DevWorldLevel &L = ctx->hostWorld.level[i];
		L.recordsOff = (uint32_t)recordsAt[i];
		L.runsOff = (uint32_t)runsAt[i];
		L.countsOff = (uint32_t)countsAt[i];
		L.elementsOff = (uint32_t)elementsAt[i];
		H.runsBytes = runsBytes[i]; // (SyncWorld carries a level it does not upload over with these sizes: the tail included)
		H.elementsBytes = elementsBytes[i];
		next[i].blockBase = ctx->edit[i].blockBase;
		next[i].blockDepth = ctx->edit[i].blockDepth;
		next[i].blockCap = ctx->edit[i].blockCap;
		ctx->edit[i] = next[i];
	}
	CVX_HIP(ctx, hipMemcpyAsync(ctx->devWorld, &ctx->hostWorld, sizeof(DevWorld), hipMemcpyHostToDevice, ctx->stream));
	return CVX_OK;
}

// Steps 1 .. 4 (file comment) for one rectangle per level; the columns of every job are on the device and valid.  D: the call, which owns the plans' scratch.
int ApplyJobs(cvx_context *ctx, cvxi::DeviceCall &D, std::vector<Job> &jobs)
{
	const DevWorld &W = ctx->hostWorld;
	// 1. plan
	for (Job &j : jobs) {
		const cvx_context::HostLevel &H = ctx->hostLevel[j.lod];
		const DevWorldLevel &L = W.level[j.lod];
		cvx_context::EditLevel &E = ctx->edit[j.lod];
		EditArgs &A = j.A;
		A.arena = ctx->arena;
		A.recordsOff = L.recordsOff;
		A.runsOff = L.runsOff;
		A.countsOff = L.countsOff;
		A.elementsOff = L.elementsOff;
		A.rowShift = H.rowShift;
		A.blocked = H.colorShift == 7;
		A.lod = j.lod;
		A.dimY = W.dimY;
		A.usedX = W.dimX >> j.lod;
		A.usedZ = W.dimZ >> j.lod;
		A.blocksZ = (A.usedZ + CVX_COLOR_BLOCK_Z - 1) / CVX_COLOR_BLOCK_Z;
		A.x0 = j.x0;
		A.z0 = j.z0;
		A.sizeX = j.sizeX;
		A.sizeZ = j.sizeZ;
		A.n = j.sizeX * j.sizeZ;
		A.bx0 = j.x0 / CVX_COLOR_BLOCK_X;
		A.bz0 = j.z0 / CVX_COLOR_BLOCK_Z;
		A.bzN = (j.z0 + j.sizeZ - 1) / CVX_COLOR_BLOCK_Z - A.bz0 + 1;
		A.blockCount = A.blocked ? ((j.x0 + j.sizeX - 1) / CVX_COLOR_BLOCK_X - A.bx0 + 1) * A.bzN : 0;
		A.headers = j.headers;
		A.elements = j.elements;
		const size_t n = (size_t)A.n, T = (size_t)A.blockCount;
		const size_t chunks = (std::max(n, T) + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
		cvxi::ScratchLayout carve;
		const size_t oRec = carve(n * 16), oCnt = carve(n * 8), oCol = carve(n * 4), oRun = carve(n * 4), oColReq = carve(n * 4), oFlags = carve(n * 4),
		             oBlockReq = carve(T * 4 + 4), oBlockNeed = carve(T * 4 + 4), oTotals = carve(4 * 8 + chunks * 8);
		uint8_t *scratch = nullptr;
		const hipError_t allocated = D.Allocate(&scratch, carve.bytes);
		if (allocated != hipSuccess) { return D.Fail(allocated, CVX_ERR_HIP); }
		A.rec = reinterpret_cast<uint4 *>(scratch + oRec);
		A.cnt = reinterpret_cast<uint2 *>(scratch + oCnt);
		A.colours = reinterpret_cast<uint32_t *>(scratch + oCol);
		A.runReq = reinterpret_cast<uint32_t *>(scratch + oRun);
		A.colReq = reinterpret_cast<uint32_t *>(scratch + oColReq);
		A.flags = reinterpret_cast<uint32_t *>(scratch + oFlags);
		A.blockReq = reinterpret_cast<uint32_t *>(scratch + oBlockReq);
		A.blockNeed = reinterpret_cast<uint32_t *>(scratch + oBlockNeed);
		j.totals = reinterpret_cast<unsigned long long *>(scratch + oTotals);
		A.abandoned = j.totals + 3;
		CVX_HIP(ctx, hipMemsetAsync(j.totals, 0, 4 * 8, ctx->stream));
		if (A.blocked) {
			const int64_t usedX = A.usedX, blocksX = (usedX + CVX_COLOR_BLOCK_X - 1) / CVX_COLOR_BLOCK_X;
			const size_t blocks = (size_t)(blocksX * A.blocksZ);
			if (!E.ready) { // block tables from the records (again: a level that was uploaded anew)
				if (E.blockCap < blocks) {
					if (E.blockBase) { (void)hipFree(E.blockBase); }
					if (E.blockDepth) { (void)hipFree(E.blockDepth); }
					E.blockBase = E.blockDepth = nullptr;
					E.blockCap = 0;
					CVX_HIP(ctx, hipMalloc((void **)&E.blockBase, blocks * 4));
					CVX_HIP(ctx, hipMalloc((void **)&E.blockDepth, blocks * 4));
					E.blockCap = blocks;
				}
				CVX_HIP(ctx, hipMemsetAsync(E.blockBase, 0, blocks * 4, ctx->stream));
				CVX_HIP(ctx, hipMemsetAsync(E.blockDepth, 0, blocks * 4, ctx->stream));
				A.blockBase = E.blockBase;
				A.blockDepth = E.blockDepth;
				const size_t recordCount = (size_t)usedX << H.rowShift;
				hipLaunchKernelGGL(cvxedit::edit_block_table_kernel, dim3(Grid(recordCount)), dim3(kThreads), 0, ctx->stream, A, recordCount);
			}
			A.blockBase = E.blockBase;
			A.blockDepth = E.blockDepth;
		}
		hipLaunchKernelGGL(cvxedit::edit_plan_columns_kernel, dim3(Grid(n)), dim3(kThreads), 0, ctx->stream, A);
		if (A.blocked) { hipLaunchKernelGGL(cvxedit::edit_plan_blocks_kernel, dim3(Grid(T)), dim3(kThreads), 0, ctx->stream, A); }
		unsigned long long *chunkSums = j.totals + 4;
		cvxi::ExclusiveScan(ctx->stream, A.runReq, A.n, chunkSums, j.totals + 0);
		if (A.blocked) {
			cvxi::ExclusiveScan(ctx->stream, A.blockReq, A.blockCount, chunkSums, j.totals + 2);
		} else {
			cvxi::ExclusiveScan(ctx->stream, A.colReq, A.n, chunkSums, j.totals + 1);
		}
		CVX_HIP(ctx, hipGetLastError());
		CVX_HIP(ctx, hipMemcpyAsync(j.host, j.totals, sizeof j.host, hipMemcpyDeviceToHost, ctx->stream));
	}
	CVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	// 2. tail space
	bool tail[CVX_LOD_LEVELS] = {};
	int64_t needRuns[CVX_LOD_LEVELS] = {}, needElements[CVX_LOD_LEVELS] = {};
	bool relayout = false;
	for (const Job &j : jobs) {
		const cvx_context::EditLevel &E = ctx->edit[j.lod];
		needRuns[j.lod] = (int64_t)j.host[0];
		needElements[j.lod] = (int64_t)(j.host[1] + j.host[2]);
		tail[j.lod] = !E.ready;
		if (!E.ready || E.runsUsed + needRuns[j.lod] > E.runsCap || E.elementsUsed + needElements[j.lod] > E.elementsCap) { relayout = true; }
	}
	if (relayout) {
		const int rc = Relayout(ctx, tail, needRuns, needElements);
		if (rc != CVX_OK) { return rc; }
	}
	// 3, 4. move blocks, write columns
	for (Job &j : jobs) {
		cvx_context::EditLevel &E = ctx->edit[j.lod];
		const DevWorldLevel &L = ctx->hostWorld.level[j.lod];
		EditArgs &A = j.A;
		A.arena = ctx->arena;
		A.recordsOff = L.recordsOff;
		A.runsOff = L.runsOff;
		A.countsOff = L.countsOff;
		A.elementsOff = L.elementsOff;
		A.runsTail = (uint32_t)E.runsUsed;
		A.elementsTail = (uint32_t)E.elementsUsed;
		if (A.blocked && A.blockCount > 0) { hipLaunchKernelGGL(cvxedit::edit_move_blocks_kernel, dim3((unsigned)A.blockCount), dim3(64), 0, ctx->stream, A); }
		hipLaunchKernelGGL(cvxedit::edit_write_columns_kernel, dim3(Grid((size_t)A.n)), dim3(kThreads), 0, ctx->stream, A);
		CVX_HIP(ctx, hipGetLastError());
		E.runsUsed += needRuns[j.lod];
		E.elementsUsed += needElements[j.lod];
		E.abandonedBytes += (int64_t)j.host[3];
	}
	return CVX_OK;
}

} // namespace

namespace cvxi {
// The body of cvx_world_edit behind its validation and upload: World.DownSample of the sub-world (sizeX x dimY x sizeZ) on the device -- the
// coarse columns over the rectangle never go to the host -- and steps 1 .. 4 for LOD 0 .. levelCount.  dSrc is valid and stays the caller's.
// On success `done` (may be null) is recorded behind the last patch; the call returns once the stream has run it.
int EditFromDevice(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, const uint8_t *dSrc, int64_t elementsOfColumns, int columnCount, int levelCount,
                   hipEvent_t done)
{
	struct Lods { // BuildLodChainOnDevice's levels, which it leaves to its caller to free
		uint32_t *headers[CVX_LOD_LEVELS] = {}, *elements[CVX_LOD_LEVELS] = {};
		~Lods()
		{
			for (int j = 0; j < CVX_LOD_LEVELS; j++) {
				if (headers[j]) { (void)hipFree(headers[j]); }
				if (elements[j]) { (void)hipFree(elements[j]); }
			}
		}
	} lods;
	if (levelCount > 0) {
		const int rc = BuildLodChainOnDevice(ctx, dSrc, elementsOfColumns, sizeX, ctx->hostWorld.dimY, sizeZ, columnCount, levelCount, lods.headers + 1, lods.elements + 1);
		if (rc != CVX_OK) { return rc; }
	}
	const uint32_t *headers[CVX_LOD_LEVELS], *elements[CVX_LOD_LEVELS];
	for (int l = 0; l <= levelCount; l++) {
		headers[l] = l == 0 ? reinterpret_cast<const uint32_t *>(dSrc) : lods.headers[l];
		elements[l] = l == 0 ? reinterpret_cast<const uint32_t *>(dSrc + (size_t)columnCount * 12) : lods.elements[l];
	}
	return PatchLevelsFromDevice(ctx, x0, z0, sizeX, sizeZ, headers, elements, levelCount, done);
}

// Steps 1 .. 4 for LOD 0 .. levelCount, one job per level, from blobs that hold every level already: EditFromDevice's tail, and all of a
// snapshot's restore (cvx_snapshot.hip), which keeps the coarse columns it captured and therefore downsamples nothing.
int PatchLevelsFromDevice(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, const uint32_t *const *headers, const uint32_t *const *elements, int levelCount,
                          hipEvent_t done)
{
	DeviceCall D(ctx, "edit");
	std::vector<Job> jobs;
	for (int l = 0; l <= levelCount; l++) {
		Job j;
		j.lod = l;
		j.x0 = x0 >> l;
		j.z0 = z0 >> l;
		j.sizeX = sizeX >> l;
		j.sizeZ = sizeZ >> l;
		j.headers = headers[l];
		j.elements = elements[l];
		jobs.push_back(j);
	}
	int rc = ApplyJobs(ctx, D, jobs);
	hipError_t e = hipSuccess;
	if (rc == CVX_OK && done) { e = hipEventRecord(done, ctx->stream); }
	const hipError_t s = hipStreamSynchronize(ctx->stream);
	if (rc == CVX_OK && (e != hipSuccess || s != hipSuccess)) { rc = D.Fail(e != hipSuccess ? e : s, CVX_ERR_HIP); }
	return rc;
}

int RoundEditRectangle(cvx_context *ctx, int64_t x0, int64_t x1, int64_t z0, int64_t z1, int levelCount, const char *what, EditRectangle *out)
{
	const int dimX = ctx->hostWorld.dimX, dimZ = ctx->hostWorld.dimZ;
	const int64_t align = ((int64_t)1 << levelCount) - 1;
	x0 &= ~align;
	z0 &= ~align;
	x1 = std::min<int64_t>((x1 + align) & ~align, dimX);
	z1 = std::min<int64_t>((z1 + align) & ~align, dimZ);
	if (((x1 - x0) & align) || ((z1 - z0) & align)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the world (%d x %d columns) is narrower than 2^levelCount = %lld", dimX, dimZ, (long long)align + 1);
	}
	const int sizeX = (int)(x1 - x0), sizeZ = (int)(z1 - z0);
	if ((int64_t)sizeX * sizeZ >= ((int64_t)1 << 31) / 12) { return Fail(ctx, CVX_ERR_CAPACITY, "%s %d x %d columns", what, sizeX, sizeZ); }
	*out = EditRectangle{ (int)x0, (int)z0, sizeX, sizeZ, sizeX * sizeZ };
	return CVX_OK;
}

int ColumnEdit(cvx_context *ctx, const EditRectangle &R, int levelCount, const ColumnEditCall &call, ColumnEditLauncher launchCount, ColumnEditLauncher launchWrite,
               float *outMs)
{
	DeviceCall held(ctx, call.call); // what the pipeline allocates, released on every path
	uint8_t *scratch = nullptr, *blob = nullptr;
	const size_t n = (size_t)R.n, chunks = (n + ScanChunk() - 1) / ScanChunk();
	cvxi::ScratchLayout carve;
	const size_t oExtra = carve(call.extraScratchBytes), oCounts = carve(n * 4), oTotals = carve(call.totals ? 0 : 2 * 8), oChunks = carve(chunks * 8);
	struct { unsigned long long total, overLimit; } own = { 0, 0 };
	// 2. the scratch, the events
	hipError_t e = held.Allocate(&scratch, carve.bytes);
	if (e == hipSuccess && !call.done) { e = held.Begin(); }
	if (e == hipSuccess && !call.totals) { e = hipMemsetAsync(scratch + oTotals, 0, sizeof own, ctx->stream); }
	if (e != hipSuccess) { return held.Fail(e, call.oomCode); }
	const ColumnEditTotals T = call.totals ? *call.totals : ColumnEditTotals{ scratch + oTotals, &own, sizeof own, 0, 8 };
	ColumnEditJob J{ R, reinterpret_cast<uint32_t *>(scratch + oCounts), reinterpret_cast<unsigned long long *>(static_cast<uint8_t *>(T.from) + T.totalAt),
	                 reinterpret_cast<unsigned int *>(static_cast<uint8_t *>(T.from) + T.overLimitAt), scratch + oExtra, nullptr, nullptr };
	// 3. count, scan, one copy back, one synchronisation
	e = launchCount(J);
	if (e == hipSuccess) {
		ExclusiveScan(ctx->stream, J.counts, R.n, reinterpret_cast<unsigned long long *>(scratch + oChunks), J.total);
		e = hipGetLastError();
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(T.to, T.from, T.bytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return held.Fail(e, call.oomCode); }
	// 4. what the blob's format cannot hold
	unsigned long long total;
	unsigned int overLimit;
	std::memcpy(&total, static_cast<const uint8_t *>(T.to) + T.totalAt, sizeof total);
	std::memcpy(&overLimit, static_cast<const uint8_t *>(T.to) + T.overLimitAt, sizeof overLimit);
	if (overLimit) {
		return Fail(ctx, CVX_ERR_CAPACITY, "%s would need more than 65535 runs, a run longer than 32767 voxels or a colour index above 32767%s", call.overLimitSubject,
		            call.overLimitNote);
	}
	if (total >= ((unsigned long long)1 << 31) - (unsigned long long)n * 3) { return Fail(ctx, CVX_ERR_CAPACITY, "%s need %llu elements", call.elementsSubject, total); }
	// 5. the sub-world blob
	e = held.Allocate(&blob, std::max<size_t>(n * 12 + (size_t)total * 4, 4));
	if (e == hipSuccess) {
		J.headers = reinterpret_cast<uint32_t *>(blob);
		J.elements = reinterpret_cast<uint32_t *>(blob + n * 12);
		e = launchWrite(J);
	}
	if (e == hipSuccess) { e = hipGetLastError(); }
	if (e != hipSuccess) { return held.Fail(e, call.oomCode); }
	// 6. cvx_world_edit's machinery
	const int rc = EditFromDevice(ctx, R.x0, R.z0, R.sizeX, R.sizeZ, blob, (int64_t)total, R.n, levelCount, call.done ? call.done : held.Event(1));
	if (rc == CVX_OK && !call.done && outMs) { *outMs = held.Ms(); }
	return rc;
}

void FreeEditState(cvx_context *ctx)
{
	for (cvx_context::EditLevel &E : ctx->edit) {
		if (E.blockBase) { (void)hipFree(E.blockBase); }
		if (E.blockDepth) { (void)hipFree(E.blockDepth); }
		E = cvx_context::EditLevel();
	}
}
} // namespace cvxi

extern "C" {

int cvx_world_set_columns(cvx_context *ctx, int lod, int x0, int z0, int sizeX, int sizeZ, const void *storage, int64_t byteLength, int columnCount)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (lod < 0 || lod >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad lod %d", lod); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	int rc = CheckRect(ctx, lod, x0, z0, sizeX, sizeZ);
	if (rc != CVX_OK) { return rc; }
	int64_t elementsOfColumns = 0;
	rc = ValidateRegion(ctx, storage, byteLength, columnCount, (int64_t)sizeX * sizeZ, ctx->hostWorld.dimY >> lod, &elementsOfColumns);
	if (rc != CVX_OK) { return rc; }
	rc = Prepare(ctx);
	if (rc != CVX_OK) { return rc; }
	cvxi::DeviceCall D(ctx, "cvx_world_set_columns");
	uint8_t *dSrc = nullptr;
	hipError_t e = D.Allocate(&dSrc, (size_t)std::max<int64_t>(byteLength, 4));
	if (e != hipSuccess) { return D.Fail(e, CVX_ERR_HIP); }
	std::vector<Job> jobs(1);
	jobs[0].lod = lod;
	jobs[0].x0 = x0;
	jobs[0].z0 = z0;
	jobs[0].sizeX = sizeX;
	jobs[0].sizeZ = sizeZ;
	jobs[0].headers = reinterpret_cast<const uint32_t *>(dSrc);
	jobs[0].elements = reinterpret_cast<const uint32_t *>(dSrc + (size_t)columnCount * 12);
	e = hipMemcpyAsync(dSrc, storage, (size_t)byteLength, hipMemcpyHostToDevice, ctx->stream);
	rc = e == hipSuccess ? ApplyJobs(ctx, D, jobs) : D.Fail(e, CVX_ERR_HIP);
	e = hipStreamSynchronize(ctx->stream);
	if (rc == CVX_OK && e != hipSuccess) { rc = D.Fail(e, CVX_ERR_HIP); }
	return rc;
}

int cvx_world_edit(cvx_context *ctx, int x0, int z0, int sizeX, int sizeZ, const void *storage, int64_t byteLength, int columnCount, int levelCount,
                   float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int align = (1 << levelCount) - 1;
	if ((x0 & align) || (z0 & align) || (sizeX & align) || (sizeZ & align)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "rectangle (%d, %d) + %d x %d is not aligned to %d columns (2^levelCount)", x0, z0, sizeX, sizeZ, align + 1);
	}
	int rc = CheckRect(ctx, 0, x0, z0, sizeX, sizeZ);
	if (rc != CVX_OK) { return rc; }
	const int dimY = ctx->hostWorld.dimY;
	int64_t elementsOfColumns = 0;
	rc = ValidateRegion(ctx, storage, byteLength, columnCount, (int64_t)sizeX * sizeZ, dimY, &elementsOfColumns);
	if (rc != CVX_OK) { return rc; }
	rc = Prepare(ctx);
	if (rc != CVX_OK) { return rc; }
	cvxi::DeviceCall D(ctx, "cvx_world_edit");
	uint8_t *dSrc = nullptr;
	hipError_t e = D.Allocate(&dSrc, (size_t)std::max<int64_t>(byteLength, 4));
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = hipMemcpyAsync(dSrc, storage, (size_t)byteLength, hipMemcpyHostToDevice, ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e, CVX_ERR_HIP); }
	rc = cvxi::EditFromDevice(ctx, x0, z0, sizeX, sizeZ, dSrc, elementsOfColumns, columnCount, levelCount, D.Event(1));
	e = hipStreamSynchronize(ctx->stream);
	if (rc == CVX_OK && e != hipSuccess) { rc = D.Fail(e, CVX_ERR_HIP); }
	if (rc == CVX_OK && outDeviceMs) { *outDeviceMs = D.Ms(); }
	return rc;
}

int cvx_world_edit_stats(cvx_context *ctx, int64_t *usedBytes, int64_t *abandonedBytes, int64_t *spareBytes)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	int64_t abandoned = 0, spare = 0;
	for (const cvx_context::EditLevel &E : ctx->edit) {
		if (!E.ready) { continue; }
		abandoned += E.abandonedBytes;
		spare += (E.runsCap - E.runsUsed) * 8 + (E.elementsCap - E.elementsUsed) * 4;
	}
	if (usedBytes) { *usedBytes = (int64_t)ctx->arenaBytes - spare; }
	if (abandonedBytes) { *abandonedBytes = abandoned; }
	if (spareBytes) { *spareBytes = spare; }
	return CVX_OK;
}

} // extern "C"
