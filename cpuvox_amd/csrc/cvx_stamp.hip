// cvx_stamp.hip -- libcpuvox_gpu.so, stamping triangle meshes into the device-resident world (cvx_world_stamp_mesh).  See include/cpuvox_gpu.h
// for the contract, cvx_stamp.h for the rules and DESIGN.md section 3.
//
// A stamp is a brush whose strokes are the voxels of a mesh.  The work per triangle is very uneven (a wall of a model can hold most of its
// voxels), so the unit of work is a (triangle, column) pair of the triangles' clamped boxes, one thread each:
//   1. setup    (a thread per triangle): cvxs::TriangleSetup, the columns of its box; scanned into the pairs' first indices
//   2. count    (a thread per pair): the hits of the column (cvxs::TriangleHit over the box's y range); scanned, in (triangle, x, z) order
//   3. cap      the per-triangle rank of a pair's first hit is its scanned offset minus that of the triangle's first pair: a pair keeps the
//               hits whose rank is below 262144 (the host voxeliser's loop order is x, z, y), scanned into the voxel list's offsets
//   4. emit     (a thread per pair, the same walk): (key, colour) per kept hit, key = column << yBits | (dimY - 1 - y); a transparent texel
//               gives a key past every real one
//   5. sort     LSD radix sort of the keys with their colours, 4 bits a pass (stable: the ranks come from wave ballots in item order)
//   6. merge    the first of every run of equal keys averages them (cvxs::MergeStamped) into the stamped-voxel list, sorted by column and
//               top-down within a column; the XZ box of the voxels comes back to the host with their number
//   7. the rectangle's columns through cvxi::ColumnEdit (cvx_edit.hip), count and write with cvxs::StampColumn; a column finds its stamped
//      voxels by binary search in the list.
// Nothing in the arena is written before step 7's hand-over, so a rejected stamp leaves the world as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_stamp.h"

using cvxi::Fail;

namespace cvxstamp {

constexpr int kRadixBits = 4, kRadixDigits = 1 << kRadixBits;
constexpr int kRadixThreads = 256, kRadixWaves = kRadixThreads / CVX_WAVE, kRadixRounds = 8, kRadixTile = kRadixThreads * kRadixRounds;

struct Mesh {
	const cvx_mesh_vertex *vertices;
	const int32_t *indices;
	const cvxs::Texture *materials;
	int materialCount;
	const uint8_t *texels;
	int dimX, dimY, dimZ;
};

struct Pairs {
	const cvxs::TriSetup *setup;
	const uint32_t *pairStart; // per triangle: its first pair (exclusive scan of the box columns)
	int triangles;
	uint32_t count;            // pairs
};

// the triangle of pair j: the last one whose first pair is <= j (triangles without columns share their successor's first pair)
__device__ __forceinline__ int TriangleOf(const Pairs &P, uint32_t j)
{
	int lo = 0, hi = P.triangles; // first index with pairStart > j
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (P.pairStart[mid] <= j) { lo = mid + 1; } else { hi = mid; }
	}
	return lo - 1;
}

__device__ __forceinline__ void PairColumn(const cvxs::TriSetup &s, uint32_t local, int *x, int *z)
{
	const uint32_t nz = (uint32_t)(s.hi[2] - s.lo[2] + 1);
	*x = s.lo[0] + (int)(local / nz);
	*z = s.lo[2] + (int)(local % nz);
}

__global__ __launch_bounds__(256) void setup_kernel(Mesh M, int triangles, cvxs::TriSetup *setup, uint32_t *columns)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= triangles) { return; }
	const cvx_mesh_vertex v0 = M.vertices[M.indices[3 * (int64_t)t]], v1 = M.vertices[M.indices[3 * (int64_t)t + 1]], v2 = M.vertices[M.indices[3 * (int64_t)t + 2]];
	cvxs::TriSetup s;
	if (!cvxs::TriangleSetup(v0, v1, v2, M.dimX, M.dimY, M.dimZ, &s)) {
		s.lo[0] = s.lo[1] = s.lo[2] = 0;
		s.hi[0] = s.hi[1] = s.hi[2] = -1;
		columns[t] = 0u;
	} else {
		columns[t] = (uint32_t)(s.hi[0] - s.lo[0] + 1) * (uint32_t)(s.hi[2] - s.lo[2] + 1);
	}
	setup[t] = s;
}

// hits[j] = the column's hits (transparent ones included); a copy goes to offsets[j] for the scan
__global__ __launch_bounds__(256) void count_kernel(Pairs P, uint32_t *hits, uint32_t *offsets)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= P.count) { return; }
	const int t = TriangleOf(P, j);
	const cvxs::TriSetup s = P.setup[t];
	int x, z;
	PairColumn(s, j - P.pairStart[t], &x, &z);
	uint32_t n = 0;
	for (int y = s.lo[1]; y <= s.hi[1]; y++) {
		float bx, by, bz;
		n += cvxs::TriangleHit(s, x, y, z, &bx, &by, &bz) ? 1u : 0u;
	}
	hits[j] = n;
	offsets[j] = n;
}

// hits[j] -> the hits the pair keeps under the per-triangle cap (offsets: the scanned hits)
__global__ __launch_bounds__(256) void cap_kernel(Pairs P, uint32_t *hits, const uint32_t *offsets)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= P.count) { return; }
	const int t = TriangleOf(P, j);
	const uint32_t rank = offsets[j] - offsets[P.pairStart[t]];
	const uint32_t cap = (uint32_t)cvxs::kVoxelizeBufferMax;
	hits[j] = rank >= cap ? 0u : std::min(hits[j], cap - rank);
}

struct EmitArgs {
	Mesh M;
	Pairs P;
	const uint32_t *emitStart; // scanned kept hits
	uint32_t emitTotal;
	int yBits;
	unsigned long long sentinel;
	unsigned long long *keys;
	uint32_t *colours;
};

__global__ __launch_bounds__(256) void emit_kernel(EmitArgs A)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= A.P.count) { return; }
	const uint32_t start = A.emitStart[j], end = j + 1 < A.P.count ? A.emitStart[j + 1] : A.emitTotal;
	if (start == end) { return; }
	const int t = TriangleOf(A.P, j);
	const cvxs::TriSetup s = A.P.setup[t];
	int x, z;
	PairColumn(s, j - A.P.pairStart[t], &x, &z);
	const Mesh &M = A.M;
	const cvx_mesh_vertex v0 = M.vertices[M.indices[3 * (int64_t)t]], v1 = M.vertices[M.indices[3 * (int64_t)t + 1]], v2 = M.vertices[M.indices[3 * (int64_t)t + 2]];
	const unsigned long long column = ((unsigned long long)x * (unsigned)M.dimZ + (unsigned)z) << A.yBits;
	uint32_t at = start;
	for (int y = s.lo[1]; y <= s.hi[1] && at < end; y++) {
		float bx, by, bz;
		if (!cvxs::TriangleHit(s, x, y, z, &bx, &by, &bz)) { continue; }
		uint32_t argb;
		const bool keep = cvxs::TriangleColour(v0, v1, v2, bx, by, bz, M.materials, M.materialCount, M.texels, &argb);
		A.keys[at] = keep ? column | (unsigned long long)(M.dimY - 1 - y) : A.sentinel;
		A.colours[at] = argb;
		at++;
	}
}

// ---- radix sort (keys + colours), kRadixBits a pass ------------------------------------------------------------------------------------------

// counts[d * blocks + b] = the items of tile b with digit d
__global__ __launch_bounds__(kRadixThreads) void radix_count_kernel(const unsigned long long *keys, uint32_t n, int shift, uint32_t *counts)
{
	__shared__ uint32_t bins[kRadixDigits];
	if (threadIdx.x < kRadixDigits) { bins[threadIdx.x] = 0u; }
	__syncthreads();
	const uint32_t base = blockIdx.x * (uint32_t)kRadixTile;
	for (int r = 0; r < kRadixRounds; r++) {
		const uint32_t i = base + (uint32_t)(r * kRadixThreads) + threadIdx.x;
		if (i < n) { atomicAdd(&bins[(keys[i] >> shift) & (kRadixDigits - 1)], 1u); }
	}
	__syncthreads();
	if (threadIdx.x < kRadixDigits) { counts[threadIdx.x * gridDim.x + blockIdx.x] = bins[threadIdx.x]; }
}

// Stable scatter: items are ranked in (round, wave, lane) order, which is their order in the tile.  starts: the scanned counts.
__global__ __launch_bounds__(kRadixThreads) void radix_scatter_kernel(const unsigned long long *keysIn, const uint32_t *valsIn, uint32_t n, int shift,
                                                                     const uint32_t *starts, unsigned long long *keysOut, uint32_t *valsOut)
{
	__shared__ uint32_t next[kRadixDigits];                 // where the digit's next item of the tile goes
	__shared__ uint32_t waveCount[kRadixWaves][kRadixDigits];
	__shared__ uint32_t waveStart[kRadixWaves][kRadixDigits];
	const int lane = threadIdx.x % CVX_WAVE, wave = threadIdx.x / CVX_WAVE;
	if (threadIdx.x < kRadixDigits) { next[threadIdx.x] = starts[threadIdx.x * gridDim.x + blockIdx.x]; }
	const uint32_t base = blockIdx.x * (uint32_t)kRadixTile;
	const unsigned long long lower = (1ull << lane) - 1ull;
	for (int r = 0; r < kRadixRounds; r++) {
		const uint32_t i = base + (uint32_t)(r * kRadixThreads) + threadIdx.x;
		const bool valid = i < n;
		unsigned long long key = 0ull;
		uint32_t val = 0u, digit = 0u;
		if (valid) {
			key = keysIn[i];
			val = valsIn[i];
			digit = (uint32_t)(key >> shift) & (kRadixDigits - 1);
		}
		// the lanes of this wave with the same digit
		unsigned long long peers = __ballot(valid);
		for (int b = 0; b < kRadixBits; b++) {
			const bool bit = (digit >> b) & 1u;
			const unsigned long long vote = __ballot(bit);
			peers &= bit ? vote : ~vote;
		}
		if (threadIdx.x < kRadixWaves * kRadixDigits) { (&waveCount[0][0])[threadIdx.x] = 0u; }
		__syncthreads();
		const uint32_t rank = (uint32_t)__popcll(peers & lower);
		if (valid && rank == 0u) { waveCount[wave][digit] = (uint32_t)__popcll(peers); }
		__syncthreads();
		if (threadIdx.x < kRadixDigits) {
			uint32_t at = next[threadIdx.x];
			for (int w = 0; w < kRadixWaves; w++) {
				waveStart[w][threadIdx.x] = at;
				at += waveCount[w][threadIdx.x];
			}
			next[threadIdx.x] = at;
		}
		__syncthreads();
		if (valid) {
			const uint32_t to = waveStart[wave][digit] + rank;
			keysOut[to] = key;
			valsOut[to] = val;
		}
	}
}

// ---- merging the duplicates -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void head_kernel(const unsigned long long *keys, uint32_t n, unsigned long long sentinel, uint32_t *heads)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) { return; }
	heads[i] = keys[i] != sentinel && (i == 0u || keys[i] != keys[i - 1]) ? 1u : 0u;
}

struct MergeArgs {
	const unsigned long long *keys;
	const uint32_t *colours;
	uint32_t n;
	const uint32_t *index;   // scanned heads
	unsigned long long sentinel;
	int yBits, dimY, dimZ;
	uint32_t *column, *y, *argb; // the stamped-voxel list
	int *box;                // x0, z0, -x1, -z1 (all atomicMin)
};

__global__ __launch_bounds__(256) void merge_kernel(MergeArgs A)
{
	__shared__ int box[4];
	if (threadIdx.x < 4) { box[threadIdx.x] = INT32_MAX; }
	__syncthreads();
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < A.n) {
		const unsigned long long key = A.keys[i];
		if (key != A.sentinel && (i == 0u || A.keys[i - 1] != key)) {
			uint32_t e = i + 1;
			while (e < A.n && A.keys[e] == key) { e++; }
			const uint32_t u = A.index[i];
			const uint32_t column = (uint32_t)(key >> A.yBits);
			A.column[u] = column;
			A.y[u] = (uint32_t)(A.dimY - 1) - (uint32_t)(key & ((1ull << A.yBits) - 1ull));
			A.argb[u] = cvxs::MergeStamped(A.colours + i, (int)(e - i));
			const int x = (int)(column / (uint32_t)A.dimZ), z = (int)(column % (uint32_t)A.dimZ);
			atomicMin(&box[0], x);
			atomicMin(&box[1], z);
			atomicMin(&box[2], -x);
			atomicMin(&box[3], -z);
		}
	}
	__syncthreads();
	if (threadIdx.x < 4 && box[threadIdx.x] != INT32_MAX) { atomicMin(&A.box[threadIdx.x], box[threadIdx.x]); }
}

// ---- the rectangle's columns (cvx_world_brush's count / write with the stamp rule) -------------------------------------------------------------

struct ColumnArgs {
	const uint8_t *arena;
	uint32_t recordsOff, runsOff, elementsOff;
	int rowShift, colorShift, dimY, dimZ;
	int x0, z0, sizeZ, n;
	int op;
	const uint32_t *column, *y, *argb; // the stamped-voxel list
	uint32_t voxels;
	uint32_t *counts;                  // per column: elements (-> offset after the scan)
	unsigned int *overLimit;
	uint32_t *headers;                 // write: the sub-world blob, n headers of 3 words
	uint32_t *elements;
};

__device__ __forceinline__ uint32_t LowerBound(const uint32_t *v, uint32_t n, uint32_t key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (v[mid] < key) { lo = mid + 1; } else { hi = mid; }
	}
	return lo;
}

__device__ __forceinline__ cvxb::BrushResult Stamp(const ColumnArgs &A, int i, uint32_t *outRuns, uint32_t *outColours, cvxb::ArenaColumn *colOut = nullptr)
{
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
	const uint4 r = reinterpret_cast<const uint4 *>(A.arena + A.recordsOff)[((size_t)cx << A.rowShift) + (size_t)cz];
	const cvxb::ArenaColumn col{ r.x, r.y, r.z, r.w, reinterpret_cast<const uint32_t *>(A.arena + A.runsOff) };
	if (colOut) { *colOut = col; }
	const uint32_t key = (uint32_t)cx * (uint32_t)A.dimZ + (uint32_t)cz;
	const uint32_t first = LowerBound(A.column, A.voxels, key), end = LowerBound(A.column, A.voxels, key + 1u);
	const uint32_t *colours = reinterpret_cast<const uint32_t *>(A.arena + A.elementsOff);
	return cvxs::StampColumn(col, colours, A.colorShift, A.y + first, A.argb + first, (int)(end - first), A.op, A.dimY, outRuns, outColours);
}

__global__ __launch_bounds__(256) void column_count_kernel(ColumnArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const cvxb::BrushResult r = Stamp(A, i, nullptr, nullptr);
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void column_write_kernel(ColumnArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	// (the colours go behind the runs' second guard, a place known once the runs are counted: the walk runs twice, the second time writing)
	const cvxb::BrushResult r = Stamp(A, i, nullptr, nullptr);
	uint32_t *h = A.headers + 3 * (size_t)i;
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	Stamp(A, i, e + 1, e + r.runCount + 2u);
	cvxb::BlobEmitHeader(h, e, off, r);
}

} // namespace cvxstamp

namespace {

constexpr unsigned kThreads = 256;

unsigned Grid(size_t n, unsigned threads = kThreads) { return (unsigned)((n + threads - 1) / threads); }

int BitWidth(uint64_t v)
{
	int b = 0;
	while (v) { b++; v >>= 1; }
	return b;
}

} // namespace

extern "C" {

int cvx_world_stamp_mesh(cvx_context *ctx, const cvx_mesh_vertex *vertices, int vertexCount, const int32_t *indices, int64_t indexCount,
                         const cvx_mesh_texture *materials, int materialCount, int op, int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (op < CVX_BRUSH_FILL || op > CVX_BRUSH_PAINT) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad op %d", op); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (vertexCount < 0 || (vertexCount > 0 && !vertices)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad vertices (vertexCount %d)", vertexCount); }
	if (indexCount < 0 || indexCount % 3 != 0 || (indexCount > 0 && !indices)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad indices (indexCount %lld, not a multiple of 3 or no array)", (long long)indexCount);
	}
	if (indexCount / 3 >= ((int64_t)1 << 28)) { return Fail(ctx, CVX_ERR_CAPACITY, "%lld triangles", (long long)(indexCount / 3)); }
	if (materialCount < 0 || materialCount > CVX_STAMP_MAX_MATERIALS || (materialCount > 0 && !materials)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "materialCount %d outside 0 .. %d", materialCount, CVX_STAMP_MAX_MATERIALS);
	}
	for (int64_t i = 0; i < indexCount; i++) {
		if (indices[i] < 0 || indices[i] >= vertexCount) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "index %lld = %d outside 0 .. %d", (long long)i, indices[i], vertexCount - 1); }
	}
	for (int i = 0; i < vertexCount; i++) {
		for (int a = 0; a < 3; a++) {
			const float p = vertices[i].position[a];
			if (!(std::fabs(p) <= 16777216.f)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "vertex %d: coordinate %g is not finite or above 2^24", i, (double)p); }
		}
	}
	// textures: one device buffer of texels, a table of (width, height, offset)
	std::vector<cvxs::Texture> textures((size_t)materialCount);
	int64_t texelBytes = 0;
	for (int m = 0; m < materialCount; m++) {
		const cvx_mesh_texture &t = materials[m];
		textures[(size_t)m] = cvxs::Texture{ 0, 0, -1 };
		if (!t.rgba) { continue; }
		if (t.width < 1 || t.height < 1 || t.width > 32768 || t.height > 32768) {
			return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "material %d: texture of %d x %d texels", m, t.width, t.height);
		}
		textures[(size_t)m] = cvxs::Texture{ t.width, t.height, texelBytes };
		texelBytes += (int64_t)t.width * t.height * 4;
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	const int triangles = (int)(indexCount / 3);
	if (triangles == 0) { return CVX_OK; }
	const int dimX = ctx->hostWorld.dimX, dimY = ctx->hostWorld.dimY, dimZ = ctx->hostWorld.dimZ;
	int rc = cvxi::PrepareWorld(ctx);
	if (rc != CVX_OK) { return rc; }

	static const char *const call = "cvx_world_stamp_mesh";
	cvxi::DeviceCall D(ctx, call);
	hipStream_t stream = ctx->stream;
	const size_t chunk = (size_t)cvxi::ScanChunk();
	auto chunksOf = [&](size_t n) { return (n + chunk - 1) / chunk; };
#define CVX_ST_HIP(call)                                                                                         \
	do {                                                                                                         \
		const hipError_t e_ = (call);                                                                            \
		if (e_ != hipSuccess) { return D.Fail(e_); }                                                             \
	} while (0)
#define CVX_ST_ALLOC(ptr, count)                                                                      \
	do {                                                                                              \
		const hipError_t e_ = D.Allocate(&(ptr), std::max<size_t>((count) * sizeof *(ptr), 16)); \
		if (e_ != hipSuccess) { return D.Fail(e_); }                                                  \
	} while (0)

	// the mesh
	cvx_mesh_vertex *dVertices = nullptr;
	int32_t *dIndices = nullptr;
	cvxs::Texture *dTextures = nullptr;
	uint8_t *dTexels = nullptr;
	unsigned long long *dTotals = nullptr; // [0] pairs [1] hits [2] kept hits [3] voxels [4] elements [5] over-limit [6..7] box (4 ints) [8] spare
	CVX_ST_ALLOC(dVertices, (size_t)vertexCount);
	CVX_ST_ALLOC(dIndices, (size_t)indexCount);
	CVX_ST_ALLOC(dTextures, (size_t)materialCount);
	CVX_ST_ALLOC(dTexels, (size_t)texelBytes);
	CVX_ST_ALLOC(dTotals, 9);
	CVX_ST_HIP(D.Begin());
	CVX_ST_HIP(hipMemcpyAsync(dVertices, vertices, (size_t)vertexCount * sizeof(cvx_mesh_vertex), hipMemcpyHostToDevice, stream));
	CVX_ST_HIP(hipMemcpyAsync(dIndices, indices, (size_t)indexCount * sizeof(int32_t), hipMemcpyHostToDevice, stream));
	if (materialCount > 0) { CVX_ST_HIP(hipMemcpyAsync(dTextures, textures.data(), textures.size() * sizeof(cvxs::Texture), hipMemcpyHostToDevice, stream)); }
	for (int m = 0; m < materialCount; m++) {
		if (textures[(size_t)m].offset >= 0) {
			CVX_ST_HIP(hipMemcpyAsync(dTexels + textures[(size_t)m].offset, materials[m].rgba, (size_t)materials[m].width * materials[m].height * 4,
			                          hipMemcpyHostToDevice, stream));
		}
	}
	CVX_ST_HIP(hipMemsetAsync(dTotals, 0, 9 * sizeof(unsigned long long), stream));
	cvxstamp::Mesh M{ dVertices, dIndices, dTextures, materialCount, dTexels, dimX, dimY, dimZ };

	// 1. triangle setup, the pairs
	cvxs::TriSetup *dSetup = nullptr;
	uint32_t *dPairStart = nullptr;
	unsigned long long *dChunks = nullptr;
	size_t chunkCap = 0; // the scans' chunk sums, grown to the longest scan
#define CVX_ST_CHUNKS(count)                                                  \
	do {                                                                      \
		if (chunksOf(count) > chunkCap) {                                     \
			chunkCap = chunksOf(count);                                       \
			CVX_ST_ALLOC(dChunks, chunkCap);                                  \
		}                                                                     \
	} while (0)
	CVX_ST_ALLOC(dSetup, (size_t)triangles);
	CVX_ST_ALLOC(dPairStart, (size_t)triangles);
	CVX_ST_CHUNKS((size_t)triangles);
	hipLaunchKernelGGL(cvxstamp::setup_kernel, dim3(Grid((size_t)triangles)), dim3(kThreads), 0, stream, M, triangles, dSetup, dPairStart);
	cvxi::ExclusiveScan(stream, dPairStart, triangles, dChunks, dTotals + 0);
	CVX_ST_HIP(hipGetLastError());
	unsigned long long totals[9] = {};
	CVX_ST_HIP(hipMemcpyAsync(totals, dTotals, sizeof totals, hipMemcpyDeviceToHost, stream));
	CVX_ST_HIP(hipStreamSynchronize(stream));
	if (totals[0] == 0) { return CVX_OK; } // no triangle with area
	if (totals[0] >= ((unsigned long long)1 << 31)) { return Fail(ctx, CVX_ERR_CAPACITY, "the triangles' boxes hold %llu columns", totals[0]); }
	cvxstamp::Pairs P{ dSetup, dPairStart, triangles, (uint32_t)totals[0] };

	// 2, 3. hits per pair, the cap, the voxel list's offsets
	uint32_t *dHits = nullptr, *dOffsets = nullptr;
	CVX_ST_ALLOC(dHits, (size_t)P.count);
	CVX_ST_ALLOC(dOffsets, (size_t)P.count);
	CVX_ST_CHUNKS((size_t)P.count);
	hipLaunchKernelGGL(cvxstamp::count_kernel, dim3(Grid(P.count)), dim3(kThreads), 0, stream, P, dHits, dOffsets);
	cvxi::ExclusiveScan(stream, dOffsets, (int)P.count, dChunks, dTotals + 1);
	hipLaunchKernelGGL(cvxstamp::cap_kernel, dim3(Grid(P.count)), dim3(kThreads), 0, stream, P, dHits, dOffsets);
	cvxi::ExclusiveScan(stream, dHits, (int)P.count, dChunks, dTotals + 2);
	CVX_ST_HIP(hipGetLastError());
	CVX_ST_HIP(hipMemcpyAsync(totals, dTotals, sizeof totals, hipMemcpyDeviceToHost, stream));
	CVX_ST_HIP(hipStreamSynchronize(stream));
	const unsigned long long kept = totals[2];
	if (kept == 0) { return CVX_OK; }
	if (kept >= ((unsigned long long)1 << 31) - chunk) { return Fail(ctx, CVX_ERR_CAPACITY, "the mesh gives %llu voxels", kept); }
	const uint32_t n = (uint32_t)kept;

	// 4. the voxel list
	const int yBits = std::max(1, BitWidth((uint64_t)dimY - 1));
	const uint64_t columns = (uint64_t)dimX * (uint64_t)dimZ;
	const int keyBits = BitWidth(columns) + yBits;
	const unsigned long long sentinel = (unsigned long long)columns << yBits; // the column past the last one
	const uint32_t tiles = (uint32_t)((n + cvxstamp::kRadixTile - 1) / cvxstamp::kRadixTile);
	unsigned long long *dKeys[2] = { nullptr, nullptr };
	uint32_t *dColours[2] = { nullptr, nullptr }, *dDigits = nullptr;
	CVX_ST_ALLOC(dKeys[0], (size_t)n);
	CVX_ST_ALLOC(dKeys[1], (size_t)n);
	CVX_ST_ALLOC(dColours[0], (size_t)n);
	CVX_ST_ALLOC(dColours[1], (size_t)n);
	CVX_ST_ALLOC(dDigits, std::max<size_t>((size_t)tiles * cvxstamp::kRadixDigits, n));
	const size_t scanMax = std::max<size_t>((size_t)tiles * cvxstamp::kRadixDigits, n);
	CVX_ST_CHUNKS(scanMax);
	cvxstamp::EmitArgs E{ M, P, dHits, n, yBits, sentinel, dKeys[0], dColours[0] };
	hipLaunchKernelGGL(cvxstamp::emit_kernel, dim3(Grid(P.count)), dim3(kThreads), 0, stream, E);
	// 5. sort
	int cur = 0;
	for (int shift = 0; shift < keyBits; shift += cvxstamp::kRadixBits) {
		hipLaunchKernelGGL(cvxstamp::radix_count_kernel, dim3(tiles), dim3(cvxstamp::kRadixThreads), 0, stream, dKeys[cur], n, shift, dDigits);
		cvxi::ExclusiveScan(stream, dDigits, (int)(tiles * cvxstamp::kRadixDigits), dChunks, dTotals + 8);
		hipLaunchKernelGGL(cvxstamp::radix_scatter_kernel, dim3(tiles), dim3(cvxstamp::kRadixThreads), 0, stream, dKeys[cur], dColours[cur], n, shift,
		                   dDigits, dKeys[cur ^ 1], dColours[cur ^ 1]);
		cur ^= 1;
	}
	// 6. merge the duplicates, the box
	uint32_t *dHeads = dDigits; // (n entries; the digit counts are done with)
	hipLaunchKernelGGL(cvxstamp::head_kernel, dim3(Grid(n)), dim3(kThreads), 0, stream, dKeys[cur], n, sentinel, dHeads);
	cvxi::ExclusiveScan(stream, dHeads, (int)n, dChunks, dTotals + 3);
	uint32_t *dColumn = dHits, *dY = dOffsets, *dArgb = dColours[cur ^ 1]; // (n >= the voxels; the pairs' arrays are done with, so are the spare colours)
	if ((size_t)n > (size_t)P.count) {
		CVX_ST_ALLOC(dColumn, (size_t)n);
		CVX_ST_ALLOC(dY, (size_t)n);
	}
	int *dBox = reinterpret_cast<int *>(dTotals + 6);
	const int boxInit[4] = { INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX };
	CVX_ST_HIP(hipMemcpyAsync(dBox, boxInit, sizeof boxInit, hipMemcpyHostToDevice, stream));
	cvxstamp::MergeArgs G{ dKeys[cur], dColours[cur], n, dHeads, sentinel, yBits, dimY, dimZ, dColumn, dY, dArgb, dBox };
	hipLaunchKernelGGL(cvxstamp::merge_kernel, dim3(Grid(n)), dim3(kThreads), 0, stream, G);
	CVX_ST_HIP(hipGetLastError());
	CVX_ST_HIP(hipMemcpyAsync(totals, dTotals, sizeof totals, hipMemcpyDeviceToHost, stream));
	CVX_ST_HIP(hipStreamSynchronize(stream));
	const uint32_t voxels = (uint32_t)totals[3];
	if (voxels == 0) { return CVX_OK; } // every hit transparent
	int box[4];
	std::memcpy(box, &totals[6], sizeof box);

	// 7. the rectangle: the voxels' XZ box rounded out to 2^levelCount, clipped
	cvxi::EditRectangle R;
	rc = cvxi::RoundEditRectangle(ctx, box[0], (int64_t)-box[2] + 1, box[1], (int64_t)-box[3] + 1, levelCount, "a stamp over", &R);
	if (rc != CVX_OK) { return rc; }
#undef CVX_ST_HIP
#undef CVX_ST_ALLOC
#undef CVX_ST_CHUNKS
	const DevWorldLevel &L = ctx->hostWorld.level[0];
	cvxstamp::ColumnArgs A{};
	A.arena = ctx->arena;
	A.recordsOff = L.recordsOff;
	A.runsOff = L.runsOff;
	A.elementsOff = L.elementsOff;
	A.rowShift = L.rowShift;
	A.colorShift = L.colorShift;
	A.dimY = dimY;
	A.dimZ = dimZ;
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	A.op = op;
	A.column = dColumn;
	A.y = dY;
	A.argb = dArgb;
	A.voxels = voxels;
	// ... and its columns through cvx_world_edit's machinery (cvxi::ColumnEdit): the elements and the flag are dTotals[4] and [5]
	const cvxi::ColumnEditTotals back{ dTotals, totals, sizeof totals, 4 * sizeof(unsigned long long), 5 * sizeof(unsigned long long) };
	cvxi::ColumnEditCall edit{ call, CVX_ERR_CAPACITY, "a stamped column", "the stamped columns" };
	edit.totals = &back;
	edit.done = D.Event(1);
	rc = cvxi::ColumnEdit(
		ctx, R, levelCount, edit,
		[&](const cvxi::ColumnEditJob &J) {
			A.counts = J.counts;
			A.overLimit = J.overLimit;
			hipLaunchKernelGGL(cvxstamp::column_count_kernel, dim3(Grid((size_t)R.n)), dim3(kThreads), 0, stream, A);
			return hipSuccess;
		},
		[&](const cvxi::ColumnEditJob &J) {
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxstamp::column_write_kernel, dim3(Grid((size_t)R.n)), dim3(kThreads), 0, stream, A);
			return hipSuccess;
		},
		nullptr);
	if (rc == CVX_OK && outDeviceMs) { *outDeviceMs = D.Ms(); }
	return rc;
}

} // extern "C"
