// cvx_readback.hip -- libcpuvox_gpu.so, reading the device-resident world back (cvx_world_read_region, cvx_world_read_level) and compacting
// its arena (cvx_world_compact).  See include/cpuvox_gpu.h for the contracts, cvx_readback.h for the per-column rule and DESIGN.md section 3.
//
// A read-back follows the brush's pattern:
//   1. count  (a thread per column of the rectangle): the column from its record (cvxr::ReadColumn), the elements its blob column takes
//   2. the counts are prefix-scanned into element offsets; ONE copy brings the total to the host
//   3. write  (same threads): the headers and the element pool, in the reference's layout
//   4. ONE device-to-host copy into the caller's buffer.
// Steps 1 .. 3 are cvxi::RegionReadCount / RegionReadWrite: a snapshot's capture (cvx_snapshot.hip) runs them per level and keeps the blob on the device.
// A compaction lays the arena out again with Relayout's placement (cvx_edit.hip) and fills it on the device, level by level:
//   1. count  (a thread per record): the run-list entries of a listed column and, for a column-after-column level, the colours of every column;
//             (a thread per 4 x 8 block, colour-block levels) the depth of the block = the most colours one of its columns holds
//   2. the counts are prefix-scanned into new places; ONE copy per level brings the totals to the host, which sizes the new arena
//   3. move   (a thread per record): the record with its new colorsBase / run-list block, its run-list block, its colours (column after column);
//             (a workgroup per block) the block's colours, and the edit's block tables
// The old arena is only read; nothing of the world changes before the new one is complete, and a failure up to there leaves it as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "cvx_context.h"
#include "cvx_edit.h"
#include "cvx_readback.h"

using cvxi::Fail;

namespace cvxread {

struct ReadArgs {
	const uint8_t *arena;
	uint32_t recordsOff, runsOff, elementsOff;
	int rowShift, colorShift, lod, dimY;
	int x0, z0, sizeZ, n;
	uint32_t *counts;   // per column: elements (-> offset after the scan)
	uint32_t *headers;  // write: n headers of 3 words
	uint32_t *elements;
};

__device__ __forceinline__ cvxb::ArenaColumn ColumnAt(const uint8_t *arena, uint32_t recordsOff, uint32_t runsOff, int rowShift, int cx, int cz)
{
	const uint4 r = reinterpret_cast<const uint4 *>(arena + recordsOff)[((size_t)cx << rowShift) + (size_t)cz];
	return cvxb::ArenaColumn{ r.x, r.y, r.z, r.w, reinterpret_cast<const uint32_t *>(arena + runsOff) };
}

__global__ __launch_bounds__(256) void read_count_kernel(ReadArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const cvxb::ArenaColumn col = ColumnAt(A.arena, A.recordsOff, A.runsOff, A.rowShift, A.x0 + i / A.sizeZ, A.z0 + i % A.sizeZ);
	const uint32_t *colours = reinterpret_cast<const uint32_t *>(A.arena + A.elementsOff);
	A.counts[i] = cvxr::ReadElements(cvxr::ReadColumn(col, colours, A.colorShift, A.lod, A.dimY, nullptr, nullptr));
}

__global__ __launch_bounds__(256) void read_write_kernel(ReadArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const cvxb::ArenaColumn col = ColumnAt(A.arena, A.recordsOff, A.runsOff, A.rowShift, A.x0 + i / A.sizeZ, A.z0 + i % A.sizeZ);
	const uint32_t *colours = reinterpret_cast<const uint32_t *>(A.arena + A.elementsOff);
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	// (the colours go behind the runs' second guard, a place known once the runs are counted: the walk runs twice, the second time writing)
	const cvxr::ReadResult r = cvxr::ReadColumn(col, colours, A.colorShift, A.lod, A.dimY, nullptr, nullptr);
	cvxr::ReadHeader(r, off, A.headers + 3 * (size_t)i);
	if (r.runCount == 0u) { return; }
	cvxr::ReadColumn(col, colours, A.colorShift, A.lod, A.dimY, e + 1, e + r.runCount + 2u);
	e[0] = 0u;
	e[r.runCount + 1u] = 0u;
}

struct CompactArgs {
	const uint8_t *src;           // the arena as it is (read only)
	uint8_t *dst;                 // the new arena (zeroed)
	uint32_t srcRecords, srcRuns, srcElements;
	uint32_t dstRecords, dstRuns, dstElements;
	int rowShift, lod, blocked, usedX, usedZ, blocksZ, blockCount;
	size_t recordCount;
	uint32_t *runOff;             // per record: run-list entries (-> new block index after the scan)
	uint32_t *colOff;             // per record (column after column) or per block: colour slots (-> new place, behind the leading line of zeros)
	uint32_t *depth;              // per block: its new depth (colours)
	uint32_t *blockBase, *blockDepth; // the edit's block tables (written by the move)
};

__device__ __forceinline__ uint4 SrcRecord(const CompactArgs &A, size_t at) { return reinterpret_cast<const uint4 *>(A.src + A.srcRecords)[at]; }
__device__ __forceinline__ const uint32_t *SrcRuns(const CompactArgs &A) { return reinterpret_cast<const uint32_t *>(A.src + A.srcRuns); }

__global__ __launch_bounds__(256) void compact_count_kernel(CompactArgs A)
{
	const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (at >= A.recordCount) { return; }
	const uint4 r = SrcRecord(A, at);
	A.runOff[at] = cvxe::RecordRunEntries(r.x, r.w);
	if (!A.blocked) { A.colOff[at] = cvxe::RecordColours(r.x, r.y, r.z, r.w, SrcRuns(A), A.lod); }
}

__global__ __launch_bounds__(256) void compact_count_blocks_kernel(CompactArgs A)
{
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= A.blockCount) { return; }
	const int bx = b / A.blocksZ, bz = b % A.blocksZ;
	uint32_t depth = 0;
	for (int p = 0; p < CVX_COLOR_STRIDE; p++) {
		const int cx = bx * CVX_COLOR_BLOCK_X + p / CVX_COLOR_BLOCK_Z, cz = bz * CVX_COLOR_BLOCK_Z + p % CVX_COLOR_BLOCK_Z;
		if (cx >= A.usedX || cz >= A.usedZ) { continue; }
		const uint4 r = SrcRecord(A, ((size_t)cx << A.rowShift) + (size_t)cz);
		depth = max(depth, cvxe::RecordColours(r.x, r.y, r.z, r.w, SrcRuns(A), A.lod));
	}
	A.depth[b] = depth;
	A.colOff[b] = depth * CVX_COLOR_STRIDE;
}

// A thread per record: the record in its new place with its new colorsBase and run-list block, the run-list block, and (column after column)
// the colours
__global__ __launch_bounds__(256) void compact_move_records_kernel(CompactArgs A)
{
	const size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (at >= A.recordCount) { return; }
	uint4 r = SrcRecord(A, at);
	if (r.x == 0u) { return; } // (the new table is zero)
	const int cx = (int)(at >> A.rowShift), cz = (int)(at & (((size_t)1 << A.rowShift) - 1));
	uint32_t colorsBase;
	if (A.blocked) {
		const size_t b = (size_t)(cx / CVX_COLOR_BLOCK_X) * (size_t)A.blocksZ + (size_t)(cz / CVX_COLOR_BLOCK_Z);
		colorsBase = (uint32_t)CVX_COLOR_STRIDE + A.colOff[b] + (uint32_t)((cx % CVX_COLOR_BLOCK_X) * CVX_COLOR_BLOCK_Z + cz % CVX_COLOR_BLOCK_Z);
	} else {
		colorsBase = (uint32_t)CVX_COLOR_STRIDE + A.colOff[at];
		const uint32_t n = cvxe::RecordColours(r.x, r.y, r.z, r.w, SrcRuns(A), A.lod);
		const uint32_t *from = reinterpret_cast<const uint32_t *>(A.src + A.srcElements) + (r.x & 0x3FFFFFFFu);
		uint32_t *to = reinterpret_cast<uint32_t *>(A.dst + A.dstElements) + colorsBase;
		for (uint32_t k = 0; k < n; k++) { to[k] = from[k]; }
	}
	if ((r.x >> 30) == 0u) { // listed: the run-list block, even-sized (its padding entry included)
		const uint32_t entries = cvxe::RecordRunEntries(r.x, r.w), block = A.runOff[at];
		const uint2 *from = reinterpret_cast<const uint2 *>(SrcRuns(A)) + r.z;
		uint2 *to = reinterpret_cast<uint2 *>(A.dst + A.dstRuns) + block;
		for (uint32_t k = 0; k < entries; k++) { to[k] = from[k]; }
		r.z = block;
	}
	r.x = (r.x & 0xC0000000u) | colorsBase;
	reinterpret_cast<uint4 *>(A.dst + A.dstRecords)[at] = r;
}

// A workgroup per 4 x 8 block of a colour-block level: the block's colours to its new place (colour k of column p of the block at
// newBase + k * 32 + p, k below the column's own colours), then the edit's block tables
__global__ __launch_bounds__(64) void compact_move_blocks_kernel(CompactArgs A)
{
	__shared__ uint32_t oldBase[CVX_COLOR_STRIDE], count[CVX_COLOR_STRIDE];
	const int b = blockIdx.x;
	const int bx = b / A.blocksZ, bz = b % A.blocksZ;
	const uint32_t newBase = (uint32_t)CVX_COLOR_STRIDE + A.colOff[b], depth = A.depth[b];
	if (threadIdx.x < CVX_COLOR_STRIDE) {
		const int p = threadIdx.x;
		const int cx = bx * CVX_COLOR_BLOCK_X + p / CVX_COLOR_BLOCK_Z, cz = bz * CVX_COLOR_BLOCK_Z + p % CVX_COLOR_BLOCK_Z;
		uint32_t base = 0, n = 0;
		if (cx < A.usedX && cz < A.usedZ) {
			const uint4 r = SrcRecord(A, ((size_t)cx << A.rowShift) + (size_t)cz);
			if (r.x != 0u) {
				base = r.x & 0x3FFFFFFFu;
				n = cvxe::RecordColours(r.x, r.y, r.z, r.w, SrcRuns(A), A.lod);
			}
		}
		oldBase[p] = base;
		count[p] = n;
	}
	__syncthreads();
	const uint32_t *from = reinterpret_cast<const uint32_t *>(A.src + A.srcElements);
	uint32_t *to = reinterpret_cast<uint32_t *>(A.dst + A.dstElements);
	for (uint32_t q = threadIdx.x; q < depth * CVX_COLOR_STRIDE; q += blockDim.x) {
		const uint32_t k = q / CVX_COLOR_STRIDE, p = q % CVX_COLOR_STRIDE;
		if (k < count[p]) { to[newBase + q] = from[oldBase[p] + k * CVX_COLOR_STRIDE]; }
	}
	if (threadIdx.x == 0) {
		A.blockBase[b] = newBase;
		A.blockDepth[b] = depth;
	}
}

} // namespace cvxread

namespace {

constexpr unsigned kThreads = 256;

unsigned Grid(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The read kernels' arguments for a rectangle, from the arena as it lies now
cvxread::ReadArgs ArgsOf(const cvx_context *ctx, const cvxi::RegionRead &R)
{
	const DevWorldLevel &L = ctx->hostWorld.level[R.lod];
	cvxread::ReadArgs A{};
	A.arena = ctx->arena;
	A.recordsOff = L.recordsOff;
	A.runsOff = L.runsOff;
	A.elementsOff = L.elementsOff;
	A.rowShift = L.rowShift;
	A.colorShift = L.colorShift;
	A.lod = R.lod;
	A.dimY = ctx->hostWorld.dimY;
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.sizeX * R.sizeZ;
	A.counts = R.offsets;
	return A;
}

} // namespace

// The device half of a read-back (cvx_context.h), shared by ReadBack below and the snapshot's capture (cvx_snapshot.hip)
hipError_t cvxi::RegionReadCount(cvx_context *ctx, DeviceCall &D, RegionRead *R)
{
	const int n = R->sizeX * R->sizeZ;
	uint8_t *scratch = nullptr;
	const size_t chunks = ((size_t)n + ScanChunk() - 1) / ScanChunk();
	ScratchLayout carve;
	const size_t oCounts = carve((size_t)n * 4), oTotal = carve(8), oChunks = carve(chunks * 8);
	R->total = 0;
	hipError_t e = D.Allocate(&scratch, carve.bytes);
	if (e != hipSuccess || n == 0) { return e; } // (n = 0: a level without columns, LOD 5 of a world 16 columns wide -- its blob is the zero headers alone)
	R->offsets = reinterpret_cast<uint32_t *>(scratch + oCounts);
	unsigned long long *dTotal = reinterpret_cast<unsigned long long *>(scratch + oTotal);
	hipLaunchKernelGGL(cvxread::read_count_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, ArgsOf(ctx, *R));
	ExclusiveScan(ctx->stream, R->offsets, n, reinterpret_cast<unsigned long long *>(scratch + oChunks), dTotal);
	e = hipGetLastError();
	if (e == hipSuccess) { e = hipMemcpyAsync(&R->total, dTotal, sizeof R->total, hipMemcpyDeviceToHost, ctx->stream); }
	return e;
}

hipError_t cvxi::RegionReadWrite(cvx_context *ctx, const RegionRead &R, uint8_t *dBlob, size_t headerBytes)
{
	const int n = R.sizeX * R.sizeZ;
	if (n == 0) { return hipSuccess; }
	cvxread::ReadArgs A = ArgsOf(ctx, R);
	A.headers = reinterpret_cast<uint32_t *>(dBlob);
	A.elements = reinterpret_cast<uint32_t *>(dBlob + headerBytes);
	hipLaunchKernelGGL(cvxread::read_write_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, A);
	return hipGetLastError();
}

namespace {

// The rectangle [x0, x0 + sizeX) x [z0, z0 + sizeZ) of level `lod` (validated) as a blob of `columnCount` headers (>= the rectangle's columns;
// the ones behind it stay zero) and the element pool, in malloc'd memory.
int ReadBack(cvx_context *ctx, const char *call, int lod, int x0, int z0, int sizeX, int sizeZ, int64_t columnCount, void **outStorage, int64_t *outByteLength,
             int32_t *outColumnCount)
{
	const int n = sizeX * sizeZ;
	std::unique_ptr<void, void (*)(void *)> blob(nullptr, std::free); // (outlives D: freeing the device blocks waits for a copy still under way)
	cvxi::DeviceCall D(ctx, call);
	uint8_t *dBlob = nullptr;
	cvxi::RegionRead R{ lod, x0, z0, sizeX, sizeZ, nullptr, 0 };
	// 1, 2. count, scan, one copy back
	hipError_t e = cvxi::RegionReadCount(ctx, D, &R);
	if (e == hipSuccess && n > 0) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	const unsigned long long total = R.total;
	if (total >= ((unsigned long long)1 << 31)) { // (storageOffset is an int32)
		return Fail(ctx, CVX_ERR_CAPACITY, "LOD %d: the read-back needs %llu elements", lod, total);
	}
	// 3, 4. the blob on the device, one copy to the host
	const size_t headerBytes = (size_t)columnCount * 12, blobBytes = headerBytes + (size_t)total * 4;
	blob.reset(std::malloc(std::max<size_t>(blobBytes, 1)));
	if (!blob) { return Fail(ctx, CVX_ERR_CAPACITY, "read-back: no host memory for %zu bytes", blobBytes); }
	e = D.Allocate(&dBlob, std::max<size_t>(blobBytes, 4));
	if (e == hipSuccess && headerBytes > (size_t)n * 12) { e = hipMemsetAsync(dBlob + (size_t)n * 12, 0, headerBytes - (size_t)n * 12, ctx->stream); }
	if (e == hipSuccess) { e = cvxi::RegionReadWrite(ctx, R, dBlob, headerBytes); }
	if (e == hipSuccess) { e = hipMemcpyAsync(blob.get(), dBlob, blobBytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	*outStorage = blob.release();
	*outByteLength = (int64_t)blobBytes;
	*outColumnCount = (int32_t)columnCount;
	return CVX_OK;
}

// Bad arguments first, then a level that is not there, then the rectangle against the level
int CheckRead(cvx_context *ctx, int lod, void **outStorage, int64_t *outByteLength, int32_t *outColumnCount)
{
	if (!outStorage || !outByteLength || !outColumnCount) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "an out pointer is NULL"); }
	*outStorage = nullptr;
	*outByteLength = 0;
	*outColumnCount = 0;
	if (lod < 0 || lod >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad lod %d", lod); }
	return CVX_OK;
}

int Prepare(cvx_context *ctx, int lod)
{
	if (!ctx->levelSet[lod]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD %d has not been uploaded", lod); }
	return cvxi::PrepareWorld(ctx);
}

// Per level of a compaction: the scratch of the counts and the totals the host sizes the new arena with
struct Level {
	bool compact = false;
	uint8_t *scratch = nullptr;
	cvxread::CompactArgs A{};
	unsigned long long *dTotals = nullptr; // [0] run-list entries, [1] colour slots, then chunk sums
	unsigned long long host[2] = { 0, 0 };
};

} // namespace

extern "C" {

int cvx_world_read_region(cvx_context *ctx, int lod, int x0, int z0, int sizeX, int sizeZ, void **outStorage, int64_t *outByteLength, int32_t *outColumnCount)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	int rc = CheckRead(ctx, lod, outStorage, outByteLength, outColumnCount);
	if (rc != CVX_OK) { return rc; }
	if (sizeX < 1 || sizeZ < 1 || x0 < 0 || z0 < 0) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "rectangle (%d, %d) + %d x %d", x0, z0, sizeX, sizeZ); }
	if (!ctx->levelSet[lod]) { return Fail(ctx, CVX_ERR_NOT_READY, "world LOD %d has not been uploaded", lod); }
	const int usedX = ctx->hostWorld.dimX >> lod, usedZ = ctx->hostWorld.dimZ >> lod;
	if ((int64_t)x0 + sizeX > usedX || (int64_t)z0 + sizeZ > usedZ) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "rectangle (%d, %d) + %d x %d outside LOD %d's %d x %d columns", x0, z0, sizeX, sizeZ, lod, usedX, usedZ);
	}
	if ((int64_t)sizeX * sizeZ >= ((int64_t)1 << 31) / 12) { return Fail(ctx, CVX_ERR_CAPACITY, "a read-back of %d x %d columns", sizeX, sizeZ); }
	rc = Prepare(ctx, lod);
	if (rc != CVX_OK) { return rc; }
	return ReadBack(ctx, "cvx_world_read_region", lod, x0, z0, sizeX, sizeZ, (int64_t)sizeX * sizeZ, outStorage, outByteLength, outColumnCount);
}

int cvx_world_read_level(cvx_context *ctx, int lod, void **outStorage, int64_t *outByteLength, int32_t *outColumnCount)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	int rc = CheckRead(ctx, lod, outStorage, outByteLength, outColumnCount);
	if (rc != CVX_OK) { return rc; }
	rc = Prepare(ctx, lod);
	if (rc != CVX_OK) { return rc; }
	const int dimX = ctx->hostWorld.dimX, dimZ = ctx->hostWorld.dimZ;
	const int64_t columnCount = ((int64_t)dimX * dimZ) / ((int64_t)(lod + 1) * (lod + 1)); // World.ColumnCount, World.cs:17
	const int usedX = dimX >> lod, usedZ = dimZ >> lod;
	if ((int64_t)usedX * usedZ >= ((int64_t)1 << 31) / 12 || columnCount >= ((int64_t)1 << 31)) {
		return Fail(ctx, CVX_ERR_CAPACITY, "a read-back of %d x %d columns", usedX, usedZ);
	}
	return ReadBack(ctx, "cvx_world_read_level", lod, 0, 0, usedX, usedZ, columnCount, outStorage, outByteLength, outColumnCount);
}

int cvx_world_compact(cvx_context *ctx, int64_t *outReclaimedBytes, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (outReclaimedBytes) { *outReclaimedBytes = 0; }
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	int rc = cvxi::PrepareWorld(ctx);
	if (rc != CVX_OK) { return rc; }
	bool any = false;
	for (const cvx_context::EditLevel &E : ctx->edit) { any = any || E.ready; }
	if (!any) { return CVX_OK; } // (nothing was edited: the arena is the upload's)
	int64_t usedBefore = 0;
	if ((rc = cvx_world_edit_stats(ctx, &usedBefore, nullptr, nullptr)) != CVX_OK) { return rc; }

	const DevWorld &W = ctx->hostWorld;
	Level lv[CVX_LOD_LEVELS];
	static const char *const call = "cvx_world_compact";
	cvxi::DeviceCall D(ctx, call);
	uint8_t *arena = nullptr;
	hipError_t e = D.Begin();
	if (e != hipSuccess) { return D.Fail(e); }
	// 1, 2. count and scan every edited level, one copy of its totals back
	for (int i = 0; i < CVX_LOD_LEVELS; i++) {
		const cvx_context::HostLevel &H = ctx->hostLevel[i];
		const cvx_context::EditLevel &E = ctx->edit[i];
		if (!E.ready) { continue; }
		Level &l = lv[i];
		l.compact = true;
		cvxread::CompactArgs &A = l.A;
		const DevWorldLevel &L = W.level[i];
		A.src = ctx->arena;
		A.srcRecords = L.recordsOff;
		A.srcRuns = L.runsOff;
		A.srcElements = L.elementsOff;
		A.rowShift = H.rowShift;
		A.lod = i;
		A.blocked = H.colorShift == 7;
		A.usedX = W.dimX >> i;
		A.usedZ = W.dimZ >> i;
		A.blocksZ = (A.usedZ + CVX_COLOR_BLOCK_Z - 1) / CVX_COLOR_BLOCK_Z;
		A.blockCount = A.blocked ? ((A.usedX + CVX_COLOR_BLOCK_X - 1) / CVX_COLOR_BLOCK_X) * A.blocksZ : 0;
		A.recordCount = (size_t)A.usedX << H.rowShift;
		if (A.blocked && ((size_t)A.blockCount > E.blockCap || !E.blockBase || !E.blockDepth)) { return Fail(ctx, CVX_ERR_HIP, "LOD %d: the edit's block tables are missing", i); }
		A.blockBase = E.blockBase;
		A.blockDepth = E.blockDepth;
		const size_t colEntries = A.blocked ? (size_t)A.blockCount : A.recordCount;
		const size_t chunks = (std::max(A.recordCount, colEntries) + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
		cvxi::ScratchLayout carve;
		const size_t oRun = carve(A.recordCount * 4), oCol = carve(colEntries * 4 + 4), oDepth = carve((size_t)A.blockCount * 4 + 4), oTotals = carve(2 * 8 + chunks * 8);
		e = D.Allocate(&l.scratch, carve.bytes);
		if (e != hipSuccess) { return D.Fail(e); }
		A.runOff = reinterpret_cast<uint32_t *>(l.scratch + oRun);
		A.colOff = reinterpret_cast<uint32_t *>(l.scratch + oCol);
		A.depth = reinterpret_cast<uint32_t *>(l.scratch + oDepth);
		l.dTotals = reinterpret_cast<unsigned long long *>(l.scratch + oTotals);
		hipLaunchKernelGGL(cvxread::compact_count_kernel, dim3(Grid(A.recordCount)), dim3(kThreads), 0, ctx->stream, A);
		if (A.blocked) { hipLaunchKernelGGL(cvxread::compact_count_blocks_kernel, dim3(Grid((size_t)A.blockCount)), dim3(kThreads), 0, ctx->stream, A); }
		cvxi::ExclusiveScan(ctx->stream, A.runOff, (int)A.recordCount, l.dTotals + 2, l.dTotals + 0);
		cvxi::ExclusiveScan(ctx->stream, A.colOff, (int)colEntries, l.dTotals + 2, l.dTotals + 1);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(l.host, l.dTotals, sizeof l.host, hipMemcpyDeviceToHost, ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
	}
	// (behind every draw enqueued before the call: the old arena may be freed once the new one is in place)
	e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) { return D.Fail(e); }
	// the new layout: Relayout's placement (cvx_edit.hip), every compacted level with the headroom of a first edit
	cvx_context::EditLevel next[CVX_LOD_LEVELS];
	size_t runsBytes[CVX_LOD_LEVELS], elementsBytes[CVX_LOD_LEVELS];
	for (int i = 0; i < CVX_LOD_LEVELS; i++) {
		const cvx_context::HostLevel &H = ctx->hostLevel[i];
		cvx_context::EditLevel n = ctx->edit[i];
		if (lv[i].compact) {
			n.runsUsed = (int64_t)lv[i].host[0];
			n.elementsUsed = (int64_t)CVX_COLOR_STRIDE + (int64_t)lv[i].host[1]; // (behind the leading line of zeros)
			n.runsCap = (n.runsUsed + std::max<int64_t>(n.runsUsed / 8, 4096) + 1) & ~(int64_t)1;
			n.elementsCap = (n.elementsUsed + std::max<int64_t>(n.elementsUsed / 8, 16384) + 31) & ~(int64_t)31;
			n.abandonedBytes = 0;
			if (n.elementsCap + CVX_COLOR_STRIDE >= ((int64_t)1 << 30)) { return Fail(ctx, CVX_ERR_CAPACITY, "LOD %d: %.2f G colour slots (the records address 2^30)", i, (double)n.elementsCap / 1e9); }
			runsBytes[i] = (size_t)n.runsCap * 8;
			elementsBytes[i] = (size_t)(n.elementsCap + CVX_COLOR_STRIDE) * 4; // (a line of zeros behind the tail)
		} else {
			runsBytes[i] = H.runsBytes;
			elementsBytes[i] = H.elementsBytes;
		}
		next[i] = n;
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
	if (cursor >= ((size_t)1 << 32)) { return Fail(ctx, CVX_ERR_CAPACITY, "the compacted world needs %.2f GiB of device tables", (double)cursor / (double)((size_t)1 << 30)); }
	// 3. the new arena (old + new at the peak: out of memory leaves the world as it was)
	e = D.Allocate(&arena, cursor);
	if (e != hipSuccess) { return D.Fail(e); }
	e = hipMemsetAsync(arena, 0, cursor, ctx->stream);
	for (int i = 0; i < CVX_LOD_LEVELS && e == hipSuccess; i++) {
		const cvx_context::HostLevel &H = ctx->hostLevel[i];
		const DevWorldLevel &old = W.level[i];
		e = hipMemcpyAsync(arena + countsAt[i], ctx->arena + old.countsOff, H.countsBytes, hipMemcpyDeviceToDevice, ctx->stream);
		if (e != hipSuccess) { break; }
		if (!lv[i].compact) { // a level never edited: as it is
			e = hipMemcpyAsync(arena + recordsAt[i], ctx->arena + old.recordsOff, H.recordsBytes, hipMemcpyDeviceToDevice, ctx->stream);
			if (e == hipSuccess) { e = hipMemcpyAsync(arena + runsAt[i], ctx->arena + old.runsOff, H.runsBytes, hipMemcpyDeviceToDevice, ctx->stream); }
			if (e == hipSuccess) { e = hipMemcpyAsync(arena + elementsAt[i], ctx->arena + old.elementsOff, H.elementsBytes, hipMemcpyDeviceToDevice, ctx->stream); }
			continue;
		}
		cvxread::CompactArgs &A = lv[i].A;
		A.dst = arena;
		A.dstRecords = (uint32_t)recordsAt[i];
		A.dstRuns = (uint32_t)runsAt[i];
		A.dstElements = (uint32_t)elementsAt[i];
		hipLaunchKernelGGL(cvxread::compact_move_records_kernel, dim3(Grid(A.recordCount)), dim3(kThreads), 0, ctx->stream, A);
		if (A.blocked && A.blockCount > 0) { hipLaunchKernelGGL(cvxread::compact_move_blocks_kernel, dim3((unsigned)A.blockCount), dim3(64), 0, ctx->stream, A); }
		e = hipGetLastError();
	}
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	// the swap (the stream is idle: nothing reads the old arena any more)
	(void)hipFree(ctx->arena);
	ctx->arena = D.Keep(arena);
	ctx->arenaBytes = cursor;
	ctx->hostWorld.arena = ctx->arena;
	for (int i = 0; i < CVX_LOD_LEVELS; i++) {
		cvx_context::HostLevel &H = ctx->hostLevel[i];
		DevWorldLevel &L = ctx->hostWorld.level[i];
		L.recordsOff = (uint32_t)recordsAt[i];
		L.runsOff = (uint32_t)runsAt[i];
		L.countsOff = (uint32_t)countsAt[i];
		L.elementsOff = (uint32_t)elementsAt[i];
		H.runsBytes = runsBytes[i]; // (SyncWorld carries a level it does not upload over with these sizes)
		H.elementsBytes = elementsBytes[i];
		ctx->edit[i] = next[i];
	}
	e = hipMemcpyAsync(ctx->devWorld, &ctx->hostWorld, sizeof(DevWorld), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	int64_t usedAfter = 0;
	if ((rc = cvx_world_edit_stats(ctx, &usedAfter, nullptr, nullptr)) != CVX_OK) { return rc; }
	if (outReclaimedBytes) { *outReclaimedBytes = usedBefore - usedAfter; }
	return CVX_OK;
}

} // extern "C"
