// cvx_spread.hip -- libcpuvox_gpu.so, travel-distance fields through the air or the solid of boxes of the device-resident world
// (cvx_world_spread[_device]).  See include/cpuvox_gpu_spread.h for the contract and cvx_spread.h for the rules.
//
//   1. init    a WAVE per column and chunk of 64 y, sixteen chunks after one another: one search of the column's runs for the chunk, then every
//              lane walks the few runs that meet it (cvxb::SpreadChunkVoxel); a ballot is the chunk's passable word, its popcount goes to the
//              wave's count and the workgroup makes one atomic; every lane stores 0xFFFF, 128 contiguous bytes per wave
//   2. seeds   a thread per seed: a 32-bit compare-and-swap on the word that holds the 16-bit value keeps the smallest start; the seed's tile and
//              the six around it become active (a seed on a tile's face concerns the neighbour although nothing in its own tile may fall)
//   3. relax   the hot path, a workgroup per tile of 8 x 64 x 8 voxels, launched over all tiles: the workgroup of a tile that is not active leaves
//              at once.  An active one loads the tile and a one-voxel halo into LDS (13 200 bytes), a wave's lanes the 64 y of a column.  For the
//              relaxation a thread owns 16 consecutive y of one column and keeps them in registers: a sweep reads the run's predecessors beside it
//              (x and z) and at its two ends from LDS, relaxes up the run and down it again (cvxb::SpreadLower) and writes what fell to LDS, so a
//              value crosses a tile's 64 y in four sweeps, not 64; sweep after sweep until __syncthreads_or says that one changed nothing, at most
//              kSpreadSweeps.  It writes back what fell, a wave's lanes again a column's 64 y, and marks, in the OTHER
//              flag array, the neighbour tiles through whose face a lowered voxel can step -- and itself if the sweeps ran out.  Values only ever
//              fall and every value is a path's length, so neither the order of the tiles nor a halo read while a neighbour writes it shows
//              in the fixpoint.  The host launches until a launch lowers nothing.  After launch L every voxel with D <= L is final (its
//              predecessor was final a launch earlier; either the same tile swept on from it, or its tile marked this one, which then made at
//              least one sweep against the halo of the launch before): more than maxSteps + 2 launches is a bug and ends the call.
//   4. finish  eight elements per thread, 256 consecutive ones per workgroup and trip: the int32 field; the reached count and the largest distance are
//              reduced per wave, then per workgroup.
// Nothing writes the arena.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cvx_context.h"
#include "cvx_spread.h"

using cvxi::Fail;

namespace cvxspread {

using cvxb::kSpreadSideY;
using cvxb::kSpreadSideZ;
using cvxb::kSpreadStrideX;
using cvxb::kSpreadStrideZ;
using cvxb::kSpreadTileCells;
using cvxb::kSpreadTileX;
using cvxb::kSpreadTileY;
using cvxb::kSpreadTileZ;
using cvxb::kSpreadUnreached;
using cvxi::WaveReduce;

constexpr unsigned kThreads = 256;
constexpr int kWaves = kThreads / CVX_WAVE;
constexpr int kColumnsPerWave = kSpreadTileX * kSpreadTileZ / kWaves; // 16: the columns of a tile a wave loads and stores
constexpr int kRunsPerColumn = kThreads / (kSpreadTileX * kSpreadTileZ), kRun = kSpreadTileY / kRunsPerColumn; // a thread relaxes 16 y of a column
static_assert(kRunsPerColumn * kSpreadTileX * kSpreadTileZ == (int)kThreads && kRun * kRunsPerColumn == kSpreadTileY && kRun <= 16, "a run per thread");
static_assert(kSpreadTileY == CVX_WAVE && kSpreadTileX * kSpreadTileZ % kWaves == 0, "a wave per column of the tile, a column's 64 y its lanes");
static_assert(kSpreadTileCells * 2 <= 160 * 1024 / 12, "twelve workgroups per CU");

struct Totals {
	unsigned long long passable, reached, visits;
	unsigned int largest, seedsUsed, changed, pad_;
};

struct Args {
	cvxb::CopyWorld W;
	cvxb::SpreadGrid G;
	uint16_t *dist;
	uint64_t *bits;
	Totals *totals;
	int32_t *out;
};

// (a wave takes kInitWords chunks and a thread kFinishElements elements, and a workgroup makes one atomic of each kind: one atomic per wave
// and chunk on the same address measured 3.1 ms for the 262 144 chunks of a 512 x 64 x 512 box, the rest of the kernel 0.2 ms)
constexpr int kInitWords = 16, kFinishElements = 8;

__global__ __launch_bounds__(kThreads) void spread_init_kernel(Args A, uint64_t words)
{
	__shared__ unsigned int waveCount[kWaves];
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CVX_WAVE)), lane = (int)(threadIdx.x % CVX_WAVE);
	const uint64_t first = ((uint64_t)blockIdx.x * kWaves + (uint64_t)wave) * kInitWords;
	const uint32_t chunks = (uint32_t)A.G.TilesY();
	unsigned int count = 0u;
	for (int n = 0; n < kInitWords && first + n < words; n++) { // (the same trips for the whole wave)
		const uint64_t w = first + n, column = w / chunks;
		const int64_t chunk = (int64_t)(w - column * chunks);
		const int64_t bx = (int64_t)(column / (uint32_t)A.G.box.size[2]), bz = (int64_t)(column - (uint64_t)bx * (uint32_t)A.G.box.size[2]);
		const int64_t x = A.G.box.min[0] + bx, z = A.G.box.min[2] + bz;
		const bool inWorld = x >= 0 && x < A.W.dimX && z >= 0 && z < A.W.dimZ;
		const cvxb::ArenaColumn col = inWorld ? cvxb::CopyColumnAt(A.W, x, z) : cvxb::ArenaColumn{ 0u, 0u, 0u, 0u, A.W.runs };
		const int64_t yLo = (int64_t)A.G.box.min[1] + chunk * 64, by = chunk * 64 + lane;
		const bool inBox = by < A.G.box.size[1];
		const uint32_t firstRun = cvxb::SpreadChunkFirst(col, yLo + 64);
		const bool passable = inBox && cvxb::SpreadChunkVoxel(col, firstRun, inWorld, A.W.dimY, A.G.medium, yLo, yLo + lane);
		const uint64_t word = __ballot(passable);
		if (inBox) { A.dist[column * (uint64_t)A.G.box.size[1] + (uint64_t)by] = (uint16_t)kSpreadUnreached; }
		if (lane == 0) { A.bits[w] = word; }
		count += (unsigned int)__popcll(word);
	}
	if (lane == 0) { waveCount[wave] = count; }
	__syncthreads();
	if (threadIdx.x == 0u) {
		unsigned long long total = 0ull;
		for (int k = 0; k < kWaves; k++) { total += waveCount[k]; }
		if (total) { atomicAdd(&A.totals->passable, total); }
	}
}

__global__ __launch_bounds__(kThreads) void spread_seeds_kernel(Args A, const cvx_spread_seed *seeds, int count, uint8_t *active)
{
	const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
	bool used = false;
	if (k < count) {
		const cvx_spread_seed seed = seeds[k];
		const int64_t bx = (int64_t)seed.voxel[0] - A.G.box.min[0], by = (int64_t)seed.voxel[1] - A.G.box.min[1], bz = (int64_t)seed.voxel[2] - A.G.box.min[2];
		if (A.G.Holds(bx, by, bz) && A.G.Bit(A.bits, bx, by, bz)) {
			used = true;
			// the 16-bit minimum through the aligned word that holds it (the array starts on a word and ends on one)
			const uint64_t i = A.G.Index(bx, by, bz);
			unsigned int *word = reinterpret_cast<unsigned int *>(A.dist) + (i >> 1);
			const unsigned shift = (unsigned)(i & 1u) * 16u;
			unsigned int seen = *word;
			while (((seen >> shift) & 0xFFFFu) > (unsigned)seed.start) {
				const unsigned int want = (seen & ~(0xFFFFu << shift)) | ((unsigned)seed.start << shift);
				const unsigned int was = atomicCAS(word, seen, want);
				if (was == seen) { break; }
				seen = was;
			}
			const int tx = (int)(bx / kSpreadTileX), ty = (int)(by / kSpreadTileY), tz = (int)(bz / kSpreadTileZ);
			active[A.G.Tile(tx, ty, tz)] = 1;
			for (int f = 0; f < 6; f++) {
				const int64_t t = cvxb::SpreadNeighbourTile(A.G, tx, ty, tz, f);
				if (t >= 0) { active[t] = 1; }
			}
		}
	}
	const uint64_t usedLanes = __ballot(used);
	if ((threadIdx.x % CVX_WAVE) == 0u && usedLanes) { atomicAdd(&A.totals->seedsUsed, (unsigned int)__popcll(usedLanes)); }
}

__global__ __launch_bounds__(kThreads) void spread_relax_kernel(Args A, uint8_t *active, uint8_t *next)
{
	__shared__ uint16_t tile[kSpreadTileCells];
	__shared__ int fellFaces; // the workgroup's SpreadFell bits (__syncthreads_or gives a truth value, not the bits)
	const uint32_t t = blockIdx.x;
	if (active[t] == 0) { return; } // (the whole workgroup: nothing but its thread 0, at the end, writes this flag during the launch)
	const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CVX_WAVE)), lane = (int)(threadIdx.x % CVX_WAVE);
	const cvxb::SpreadGrid &G = A.G;
	const int tilesY = G.TilesY(), tilesZ = G.TilesZ();
	const int ty = (int)(t % (uint32_t)tilesY), tz = (int)((t / (uint32_t)tilesY) % (uint32_t)tilesZ), tx = (int)(t / ((uint32_t)tilesY * (uint32_t)tilesZ));
	const int64_t bx0 = (int64_t)tx * kSpreadTileX, by0 = (int64_t)ty * kSpreadTileY, bz0 = (int64_t)tz * kSpreadTileZ;
	const int64_t sizeX = G.box.size[0], sizeY = G.box.size[1], sizeZ = G.box.size[2];
	// the tile and its halo: a wave per column, lane l the y by0 - 1 + l, lanes 0 and 1 also by0 + 63 and by0 + 64
#pragma unroll 5
	for (int c = wave; c < cvxb::kSpreadSideX * kSpreadSideZ; c += kWaves) { // (25 columns a wave, five loads in flight)
		const int sx = c / kSpreadSideZ, sz = c - sx * kSpreadSideZ;
		const int64_t bx = bx0 + sx - 1, bz = bz0 + sz - 1;
		const bool inside = bx >= 0 && bx < sizeX && bz >= 0 && bz < sizeZ;
		const uint16_t *column = A.dist + (inside ? G.Column(bx, bz) * (uint64_t)sizeY : 0u);
		const int64_t by = by0 - 1 + lane;
		tile[c * kSpreadSideY + lane] = inside && by >= 0 && by < sizeY ? column[by] : (uint16_t)kSpreadUnreached;
		if (lane < 2) {
			const int64_t high = by0 + 63 + lane;
			tile[c * kSpreadSideY + 64 + lane] = inside && high < sizeY ? column[high] : (uint16_t)kSpreadUnreached;
		}
	}
	if (threadIdx.x == 0u) { fellFaces = 0; }
	// the relaxation's mapping: a thread owns kRun consecutive y of one column, four threads a column, and keeps them in registers
	const int own = (int)(threadIdx.x / kRunsPerColumn), run = (int)(threadIdx.x % kRunsPerColumn);
	const int base = cvxb::SpreadCell(own / kSpreadTileZ, run * kRun, own % kSpreadTileZ);
	uint32_t passable = 0u; // bit k: voxel k of the run
	{
		const int64_t bx = bx0 + own / kSpreadTileZ, bz = bz0 + own % kSpreadTileZ;
		if (bx < sizeX && bz < sizeZ) { passable = (uint32_t)(A.bits[G.Column(bx, bz) * (uint64_t)tilesY + (uint64_t)ty] >> (run * kRun)) & ((1u << kRun) - 1u); }
	}
	__syncthreads();
	uint32_t v[kRun];
#pragma unroll
	for (int k = 0; k < kRun; k++) { v[k] = tile[base + k]; }
	const int stepFaces = G.stepFaces;
	const bool up = (stepFaces & 8) != 0, down = (stepFaces & 4) != 0; // a step +Y comes from y - 1, a step -Y from y + 1
	const uint32_t maxSteps = G.maxSteps;
	int more = 1;
	for (int sweep = 0; sweep < cvxb::kSpreadSweeps && more; sweep++) { // (the same trip count for every thread: the decision is the workgroup's)
		// the run's predecessors beside it, from LDS: other threads' voxels and the halo
		uint32_t beside[kRun];
#pragma unroll
		for (int k = 0; k < kRun; k++) {
			uint32_t least = kSpreadUnreached;
			for (int f = 0; f < 6; f++) {
				if (f != 2 && f != 3 && ((stepFaces >> f) & 1)) {
					const uint32_t d = tile[base + k + cvxb::SpreadPredecessor(f)];
					least = d < least ? d : least;
				}
			}
			beside[k] = least;
		}
		const uint32_t below = tile[base - 1], above = tile[base + kRun];
		// up the run, then down it, in registers: a value travels the whole run in one sweep, either way
		uint32_t lowered = 0u;
#pragma unroll
		for (int i = 0; i < 2 * kRun - 1; i++) {
			const int k = i < kRun ? i : 2 * kRun - 2 - i;
			if ((passable >> k) & 1u) {
				uint32_t least = beside[k];
				if (up) {
					const uint32_t d = k > 0 ? v[k > 0 ? k - 1 : 0] : below;
					least = d < least ? d : least;
				}
				if (down) {
					const uint32_t d = k < kRun - 1 ? v[k < kRun - 1 ? k + 1 : 0] : above;
					least = d < least ? d : least;
				}
				const uint32_t lower = cvxb::SpreadLower(v[k], least, maxSteps);
				if (lower < v[k]) {
					v[k] = lower;
					lowered |= 1u << k;
				}
			}
		}
#pragma unroll
		for (int k = 0; k < kRun; k++) {
			if ((lowered >> k) & 1u) { tile[base + k] = (uint16_t)v[k]; }
		}
		more = __syncthreads_or(lowered != 0u ? 1 : 0);
	}
	// what fell, back with a column's 64 y in a wave's lanes: nothing else writes the tile's voxels during the launch, so the array still holds
	// what they were
	int fell = 0;
	if (by0 + lane < sizeY) {
#pragma unroll 4
		for (int j = 0; j < kColumnsPerWave; j++) {
			const int ci = wave * kColumnsPerWave + j, lx = ci / kSpreadTileZ, lz = ci % kSpreadTileZ;
			if (bx0 + lx < sizeX && bz0 + lz < sizeZ) {
				const uint64_t at = G.Index(bx0 + lx, by0 + lane, bz0 + lz);
				const uint16_t now = tile[cvxb::SpreadCell(lx, lane, lz)];
				if (now < A.dist[at]) {
					A.dist[at] = now;
					fell |= cvxb::SpreadFell(lx, lane, lz, stepFaces) | 64;
				}
			}
		}
	}
	if (fell) { atomicOr(&fellFaces, fell); }
	__syncthreads();
	if (threadIdx.x == 0u) {
		fell = fellFaces;
		active[t] = 0; // both arrays are clear of this launch's flags when it ends: they swap
		atomicAdd(&A.totals->visits, 1ull);
		if (fell) {
			for (int f = 0; f < 6; f++) {
				const int64_t n = (fell >> f) & 1 ? cvxb::SpreadNeighbourTile(G, tx, ty, tz, f) : -1;
				if (n >= 0) { next[n] = 1; }
			}
			if (more) { next[t] = 1; } // the sweeps ran out before the tile settled
			atomicOr(&A.totals->changed, 1u);
		}
	}
}

__global__ __launch_bounds__(kThreads) void spread_finish_kernel(Args A, uint32_t n)
{
	__shared__ unsigned long long waveReached[kWaves];
	__shared__ uint32_t waveLargest[kWaves];
	unsigned long long reached = 0ull;
	uint32_t largest = 0u;
	const uint32_t sizeY = (uint32_t)A.G.box.size[1], chunks = (uint32_t)A.G.TilesY();
	for (int e = 0; e < kFinishElements; e++) {
		const uint32_t i = (blockIdx.x * kFinishElements + (uint32_t)e) * kThreads + threadIdx.x; // (n < 2^31: no overflow)
		if (i < n) {
			const uint32_t column = i / sizeY, y = i - column * sizeY;
			const bool passable = ((A.bits[(uint64_t)column * chunks + (y >> 6)] >> (y & 63u)) & 1ull) != 0ull;
			const uint32_t working = A.dist[i];
			A.out[i] = cvxb::SpreadResult(passable, working);
			if (passable && working != kSpreadUnreached) {
				reached++;
				largest = working > largest ? working : largest;
			}
		}
	}
	reached = WaveReduce<unsigned long long>(reached, [](unsigned long long a, unsigned long long b) { return a + b; });
	largest = WaveReduce<uint32_t>(largest, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
	if ((threadIdx.x % CVX_WAVE) == 0u) {
		waveReached[threadIdx.x / CVX_WAVE] = reached;
		waveLargest[threadIdx.x / CVX_WAVE] = largest;
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		for (int k = 1; k < kWaves; k++) {
			reached += waveReached[k];
			largest = waveLargest[k] > largest ? waveLargest[k] : largest;
		}
		if (reached) {
			atomicAdd(&A.totals->reached, reached);
			atomicMax(&A.totals->largest, largest);
		}
	}
}

} // namespace cvxspread

namespace {

using cvxi::Grid;
using cvxspread::kThreads;

size_t Align(uint64_t bytes) { return (size_t)((bytes + 255) & ~(uint64_t)255); }

int Spread(cvx_context *ctx, const char *call, const cvx_spread_params *params, const cvx_spread_seed *seeds, int seedCount, int32_t *out, bool device,
           cvx_spread_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	char message[160];
	if (cvxb::SpreadCheck(params, seeds, seedCount, out, message, sizeof message) != 0) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, message); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	cvxspread::Args A{};
	A.G = cvxb::SpreadGridOf(*params);
	const uint64_t n = A.G.Elements(), words = A.G.Words();
	const int64_t tiles = A.G.Tiles();
	// the scratch: totals | seeds | two flag arrays | passable words | working distances | the field of the host-array call
	const size_t seedsAt = Align(sizeof(cvxspread::Totals)), flagsAt = seedsAt + Align((uint64_t)seedCount * sizeof(cvx_spread_seed));
	const size_t bitsAt = flagsAt + 2 * Align((uint64_t)tiles), distAt = bitsAt + Align(words * 8), outAt = distAt + Align(n * 2);
	const size_t bytes = outAt + (device ? 0 : (size_t)n * 4);
	int rc = cvxi::PrepareWorld(ctx);
	if (rc != CVX_OK) { return rc; }

	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	cvxspread::Totals host{};
	int64_t launches = 0;
	hipError_t e = D.Allocate(&scratch, bytes);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = hipMemsetAsync(scratch, 0, bitsAt, ctx->stream); } // the totals and both flag arrays
	if (e == hipSuccess) { e = hipMemcpyAsync(scratch + seedsAt, seeds, (size_t)seedCount * sizeof(cvx_spread_seed), hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.totals = reinterpret_cast<cvxspread::Totals *>(scratch);
		A.bits = reinterpret_cast<uint64_t *>(scratch + bitsAt);
		A.dist = reinterpret_cast<uint16_t *>(scratch + distAt);
		A.out = device ? out : reinterpret_cast<int32_t *>(scratch + outAt);
		uint8_t *flags[2] = { scratch + flagsAt, scratch + flagsAt + Align((uint64_t)tiles) };
		hipLaunchKernelGGL(cvxspread::spread_init_kernel, dim3(Grid(words, cvxspread::kWaves * cvxspread::kInitWords)), dim3(kThreads), 0, ctx->stream, A, words);
		hipLaunchKernelGGL(cvxspread::spread_seeds_kernel, dim3(Grid((uint64_t)seedCount, kThreads)), dim3(kThreads), 0, ctx->stream, A,
		                   reinterpret_cast<const cvx_spread_seed *>(scratch + seedsAt), seedCount, flags[0]);
		e = hipGetLastError();
		const int64_t bound = (int64_t)A.G.maxSteps + 2;
		if (e == hipSuccess) {
			launches = cvxi::LaunchUntilUnchanged(
				ctx, &A.totals->changed, bound,
				[&](const int64_t &k) {
					hipLaunchKernelGGL(cvxspread::spread_relax_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, ctx->stream, A, flags[k & 1], flags[(k & 1) ^ 1]);
					return hipSuccess;
				},
				&e);
			if (launches < 0) { return Fail(ctx, CVX_ERR_HIP, "%s: the relaxation did not settle in maxSteps + 2 = %lld launches", call, (long long)bound); }
		}
	}
	if (e == hipSuccess) {
		hipLaunchKernelGGL(cvxspread::spread_finish_kernel, dim3(Grid(n, kThreads * cvxspread::kFinishElements)), dim3(kThreads), 0, ctx->stream, A, (uint32_t)n);
		e = hipGetLastError();
	}
	if (e == hipSuccess) { e = hipMemcpyAsync(&host, A.totals, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess && !device) { e = hipMemcpyAsync(out, A.out, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	if (summary) {
		cvx_spread_summary S{};
		S.passable = (int64_t)host.passable;
		S.reached = (int64_t)host.reached;
		S.largestDistance = host.reached ? (int32_t)host.largest : -1;
		S.seedsUsed = (int32_t)host.seedsUsed;
		S.launches = (int32_t)launches;
		S.tileVisits = (int64_t)host.visits;
		*summary = S;
	}
	return CVX_OK;
}

} // namespace

extern "C" {

int cvx_world_spread(cvx_context *ctx, const cvx_spread_params *params, const cvx_spread_seed *seeds, int seedCount, int32_t *out, cvx_spread_summary *summary,
                     float *outDeviceMs)
{
	return Spread(ctx, "cvx_world_spread", params, seeds, seedCount, out, false, summary, outDeviceMs);
}

int cvx_world_spread_device(cvx_context *ctx, const cvx_spread_params *params, const cvx_spread_seed *seeds, int seedCount, int32_t *outDevice,
                            cvx_spread_summary *summary, float *outDeviceMs)
{
	return Spread(ctx, "cvx_world_spread_device", params, seeds, seedCount, outDevice, true, summary, outDeviceMs);
}

} // extern "C"
