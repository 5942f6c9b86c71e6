// cvx_light.hip -- libcpuvox_gpu.so, sky occlusion and sun shadows baked into the device-resident world (cvx_world_light).  See
// include/cpuvox_gpu.h for the contract, cvx_light.h for the rules and DESIGN.md sections 3 and 4.
//
// The mechanics are cvxi::ColumnEdit's (cvx_edit.hip): its count launcher counts the elements of every column of the rounded rectangle, its write
// launcher writes the sub-world blob in the builder's encoding (cvxb::LightColumn: the colours verbatim) and then shades the blob's colours in place.
// Nothing in the arena is written before that last step, and the blob has one colour per voxel, so runs that share colour slots are shaded once.
//
// The shade kernel (light_brick_kernel): a workgroup of 256 threads owns a tile of 16 x 16 columns of the clipped box and walks the y range its
// columns have solid voxels in, 32 voxels (a slab) at a time:
//   1. expand   the occupancy of the tile plus a halo of skyRange columns, y = slab .. slab + 63, into LDS: ONE 64-bit word per column (bit b =
//               voxel slab + b), rows padded to an odd number of words.  The sky term of a voxel of the slab reaches at most skyRange <= 32 voxels
//               sideways and upwards: all of it is in the brick.
//   2. compact  every thread counts the solid voxels of its column inside the slab and the box (a popcount), a block-wide exclusive scan (wave
//               shuffles, then the four wave totals) numbers them, and the voxels are written to a list in LDS, 2048 at a time
//   3. shade    a LANE PER SOLID VOXEL: the 17 sky directions are word reads and bit tests in LDS; the sun's face neighbours and shadow walk
//               read LDS while they are inside the brick and the arena's records (cvxb::ArenaOcc) beyond it; the voxel's colour in the blob (the
//               column's colour base + the solid voxels above it: a popcount of its word + the count above the slab) is read, shaded, written.
// -DCVX_LIGHT_RECORDS builds the straightforward variant instead (make variant NAME=lightrec DEFS=-DCVX_LIGHT_RECORDS): no brick kernel, the
// write kernel shades every voxel as it emits it, every occupancy test a record fetch and a run search.  It is the A/B partner of
// tools/light_bench.py and a second implementation for tests/test_gpu_world_light.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "cvx_context.h"
#include "cvx_lamps.h"

using cvxi::Fail;

namespace cvxlight {

struct LightArgs {
	cvxb::CopyWorld W;
	cvxb::PiecesBox B;             // the clipped box
	cvx_light_params P;
	int x0, z0, sizeZ, n;          // the rectangle
	uint32_t *counts;              // per column: elements (-> offset after the scan)
	unsigned int *overLimit;
	uint32_t *headers;             // the sub-world blob, n headers of 3 words
	uint32_t *elements;
	int tilesZ, brickSide, brickStride; // brick kernel: tiles per row of the box, columns per side of the brick, words per row
	const cvx_lamp *lamps;         // cvx_world_light_lamps: the call's lamps on the device (lampCount 0: none, the kernels of cvx_world_light run)
	int lampCount;
};

template <class Recolour>
__device__ __forceinline__ void WriteColumn(const LightArgs &A, int i, int cx, int cz, const Recolour &recolour)
{
	const uint32_t off = A.counts[i];
	uint32_t *e = A.elements + off;
	uint32_t *h = A.headers + 3 * (size_t)i;
	const cvxb::BrushResult r = cvxb::LightColumn(A.W, cx, cz, nullptr, nullptr, cvxb::LightKeep{});
	if (r.runCount == 0u) { cvxb::BlobEmitEmpty(h); return; }
	cvxb::LightColumn(A.W, cx, cz, e + 1, e + r.runCount + 2u, recolour);
	cvxb::BlobEmitHeader(h, e, off, r);
}

__global__ __launch_bounds__(256) void light_count_kernel(LightArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const cvxb::BrushResult r = cvxb::LightColumn(A.W, A.x0 + i / A.sizeZ, A.z0 + i % A.sizeZ, nullptr, nullptr, cvxb::LightKeep{});
	if (r.overLimit) { atomicOr(A.overLimit, 1u); }
	A.counts[i] = cvxb::BlobElements(r);
}

__global__ __launch_bounds__(256) void light_write_kernel(LightArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= A.n) { return; }
	const int cx = A.x0 + i / A.sizeZ, cz = A.z0 + i % A.sizeZ;
#ifdef CVX_LIGHT_RECORDS
	if (A.lampCount > 0) {
		WriteColumn(A, i, cx, cz, cvxb::LightLampsFromRecords{ cvxb::ArenaOcc{ A.W }, A.B, A.P, cx, cz, A.lamps, A.lampCount });
	} else {
		WriteColumn(A, i, cx, cz, cvxb::LightFromRecords{ cvxb::ArenaOcc{ A.W }, A.B, A.P, cx, cz });
	}
#else
	WriteColumn(A, i, cx, cz, cvxb::LightKeep{});
#endif
}

#ifndef CVX_LIGHT_RECORDS

constexpr int kTile = 16;            // columns per side of a workgroup's tile
constexpr int kSlab = 32;            // voxels of y shaded per pass; the brick holds kSlab + 32 = 64 of them
constexpr int kThreads = kTile * kTile;
constexpr int kList = 2048;          // voxels compacted per round
constexpr int kLampList = 256;       // lamps a tile-slab's cull keeps in LDS per round (tests/test_gpu_world_lamps.py reads this constant)

// occupancy inside the brick, no checks: the sky directions of a voxel of the slab never leave it
struct BrickNear {
	const unsigned long long *brick;
	int stride, ox, oz, oy;
	__device__ __forceinline__ bool operator()(int x, int y, int z) const { return (brick[(x - ox) * stride + (z - oz)] >> (y - oy)) & 1ull; }
};

// occupancy anywhere: the brick where it reaches, the records beyond
struct BrickAny {
	BrickNear near;
	int side;
	cvxb::ArenaOcc far;
	__device__ __forceinline__ bool operator()(int x, int y, int z) const
	{
		if ((unsigned)(x - near.ox) < (unsigned)side && (unsigned)(z - near.oz) < (unsigned)side && (unsigned)(y - near.oy) < 64u) { return near(x, y, z); }
		return far(x, y, z);
	}
};

// bits lo .. hi - 1 (0 <= lo < hi <= 64)
__device__ __forceinline__ unsigned long long BitSpan(int lo, int hi) { return (~0ull >> (64 - (hi - lo))) << lo; }

// The lamps of the call that reach the range lo .. hi (inclusive voxels): a lamp reaches it when its cube [L - (r - 1), L + (r - 1)] meets it (a
// voxel with d2 < r2 has every |D_i| <= r - 1).  Block-wide: every thread tests a contiguous share of the lamps and counts, an exclusive scan
// numbers the survivors, and those numbered first .. first + kLampList - 1 are written to `out` (x, y, z, radius << 8 | level).  Returns the
// number of survivors.  A lamp of level 0 contributes nothing anywhere and is dropped here.
__device__ __forceinline__ bool LampReaches(const cvx_lamp &l, const int *lo, const int *hi)
{
	const int r = l.radius - 1;
	return l.level > 0 && l.pos[0] + r >= lo[0] && l.pos[0] - r <= hi[0] && l.pos[1] + r >= lo[1] && l.pos[1] - r <= hi[1] && l.pos[2] + r >= lo[2] && l.pos[2] - r <= hi[2];
}

__device__ __forceinline__ int CullLamps(const LightArgs &A, const int *lo, const int *hi, int first, int4 *out, uint32_t *waveSum)
{
	const int tid = threadIdx.x;
	const int share = (A.lampCount + kThreads - 1) / kThreads;
	const int from = min(tid * share, A.lampCount), to = min(from + share, A.lampCount);
	uint32_t before = 0u;
	for (int l = from; l < to; l++) { before += LampReaches(A.lamps[l], lo, hi) ? 1u : 0u; }
	const uint32_t cnt = before;
	for (int d = 1; d < CVX_WAVE; d <<= 1) {
		const uint32_t up = __shfl_up(before, d);
		if ((tid & (CVX_WAVE - 1)) >= d) { before += up; }
	}
	if ((tid & (CVX_WAVE - 1)) == CVX_WAVE - 1) { waveSum[tid / CVX_WAVE] = before; }
	__syncthreads(); // (also: every lane has finished with the list of the round before)
	uint32_t total = 0u;
	before -= cnt;
	for (int w = 0; w < kThreads / CVX_WAVE; w++) {
		if (w < tid / CVX_WAVE) { before += waveSum[w]; }
		total += waveSum[w];
	}
	if (cnt != 0u) {
		uint32_t at = before - (uint32_t)first; // (wraps below `first`: the unsigned comparison drops those too)
		for (int l = from; l < to; l++) {
			const cvx_lamp lamp = A.lamps[l];
			if (!LampReaches(lamp, lo, hi)) { continue; }
			if (at < (uint32_t)kLampList) { out[at] = make_int4(lamp.pos[0], lamp.pos[1], lamp.pos[2], (lamp.radius << 8) | lamp.level); }
			at++;
		}
	}
	__syncthreads();
	return (int)total;
}

// kLamps false: cvx_world_light's kernel.  true: after the slab's brick is expanded the workgroup culls the call's lamps against the slab's part of
// the tile and the box (CullLamps), and every voxel lane adds the terms of the survivors to its shade before the one min.  More than kLampList
// survivors are taken kLampList at a time, the partial sum carried in the lane's register: the voxels are shaded 256 at a time (one per lane)
// and the list is rebuilt per round for each 256 -- the rare case pays, the common one (one round) culls once per slab.
template <bool kLamps>
__global__ __launch_bounds__(kThreads) void light_brick_kernel(LightArgs A)
{
	extern __shared__ unsigned long long brick[];   // brickSide rows of brickStride words
	__shared__ uint16_t list[kList];                // tile column << 5 | bit
	__shared__ uint32_t colourAt[kThreads];         // per tile column: the element of its first solid voxel at or below the slab's top
	__shared__ uint32_t waveSum[kThreads / CVX_WAVE];
	__shared__ int tileLo, tileHi;
	__shared__ int4 lampList[kLamps ? kLampList : 1];
	__shared__ uint32_t lampWaveSum[kThreads / CVX_WAVE];

	const int tid = threadIdx.x;
	const int halo = A.P.skyRange, side = A.brickSide, stride = A.brickStride;
	const int tx0 = A.B.x0 + (int)(blockIdx.x / A.tilesZ) * kTile, tz0 = A.B.z0 + (int)(blockIdx.x % A.tilesZ) * kTile;
	const int cx = tx0 + tid / kTile, cz = tz0 + tid % kTile;
	const bool mine = cx < A.B.x1 && cz < A.B.z1;
	if (tid == 0) {
		tileLo = INT_MAX;
		tileHi = INT_MIN;
	}
	__syncthreads();
	cvxb::ArenaColumn own{ 0u, 0u, 0u, 0u, A.W.runs };
	uint32_t colourBase = 0u; // the element of the column's first colour in the blob
	if (mine) {
		own = cvxb::CopyColumnAt(A.W, cx, cz);
		if (own.Count() != 0u) {
			atomicMin(&tileLo, (int)own.WorldMin());
			atomicMax(&tileHi, (int)own.WorldMax());
			const uint32_t *h = A.headers + 3 * ((size_t)(cx - A.x0) * A.sizeZ + (size_t)(cz - A.z0));
			colourBase = h[0] + (h[1] & 0xFFFFu) + 2u;
		}
	}
	__syncthreads();
	const int yLo = max(A.B.y0, tileLo), yHi = min(A.B.y1, tileHi);
	const BrickNear near{ brick, stride, tx0 - halo, tz0 - halo, 0 };
	const cvxb::LightDims dims{ A.W.dimX, A.W.dimY, A.W.dimZ };

	for (int ys = yLo; ys < yHi; ys += kSlab) {
		// 1. expand
		for (int c = tid; c < side * side; c += kThreads) {
			const int bx = c / side, bz = c % side;
			const int wx = near.ox + bx, wz = near.oz + bz;
			unsigned long long bits = 0ull;
			if (wx >= 0 && wx < A.W.dimX && wz >= 0 && wz < A.W.dimZ) {
				const cvxb::ArenaColumn col = cvxb::CopyColumnAt(A.W, wx, wz);
				const uint32_t count = col.Count();
				if (count != 0u && (int)col.WorldMax() > ys && (int)col.WorldMin() < ys + 64) {
					for (uint32_t k = count > 3u ? cvxb::RunAtOrBelow(col, ys + 63) : 0u; k < count; k++) {
						const cvxb::SolidRun run = col.Run(k);
						if ((int)run.top <= ys) { break; }
						const int lo = max((int)run.bottom, ys) - ys, hi = min((int)run.top, ys + 64) - ys;
						if (lo < hi) { bits |= BitSpan(lo, hi); }
					}
				}
			}
			brick[bx * stride + bz] = bits;
		}
		__syncthreads();
		// 2. compact: this column's solid voxels inside the slab and the box
		const uint32_t word = (uint32_t)brick[(tid / kTile + halo) * stride + (tid % kTile + halo)];
		const int top = min(yHi - ys, kSlab);
		const uint32_t m = mine ? word & (uint32_t)BitSpan(0, top) : 0u;
		uint32_t before = __popc(m);
		const uint32_t cnt = before;
		for (int d = 1; d < CVX_WAVE; d <<= 1) {
			const uint32_t up = __shfl_up(before, d);
			if ((tid & (CVX_WAVE - 1)) >= d) { before += up; }
		}
		if ((tid & (CVX_WAVE - 1)) == CVX_WAVE - 1) { waveSum[tid / CVX_WAVE] = before; }
		if (m != 0u) { // the solid voxels of the column at or above the slab's last voxel come before the slab's in its colours
			uint32_t above = 0u;
			for (uint32_t k = 0; k < own.Count(); k++) {
				const cvxb::SolidRun run = own.Run(k);
				if ((int)run.top <= ys + kSlab) { break; }
				above += run.top - (uint32_t)max((int)run.bottom, ys + kSlab);
			}
			colourAt[tid] = colourBase + above;
		}
		__syncthreads();
		uint32_t total = 0u;
		before -= cnt;
		for (int w = 0; w < kThreads / CVX_WAVE; w++) {
			if (w < tid / CVX_WAVE) { before += waveSum[w]; }
			total += waveSum[w];
		}
		int lampLo[3] = { 0, 0, 0 }, lampHi[3] = { 0, 0, 0 }, survivors = 0;
		if constexpr (kLamps) { // the lamps that reach this slab's part of the tile and the box
			lampLo[0] = tx0, lampLo[1] = ys, lampLo[2] = tz0;
			lampHi[0] = min(tx0 + kTile, A.B.x1) - 1, lampHi[1] = ys + top - 1, lampHi[2] = min(tz0 + kTile, A.B.z1) - 1;
			survivors = total != 0u ? CullLamps(A, lampLo, lampHi, 0, lampList, lampWaveSum) : 0;
		}
		// 3. shade, kList voxels per round
		BrickNear slabNear = near;
		slabNear.oy = ys;
		const BrickAny any{ slabNear, side, cvxb::ArenaOcc{ A.W } };
		for (uint32_t base = 0u; base < total; base += kList) {
			uint32_t at = before;
			for (uint32_t rest = m; rest != 0u; rest &= rest - 1u, at++) {
				if (at - base < (uint32_t)kList) { list[at - base] = (uint16_t)((tid << 5) | (__ffs(rest) - 1)); }
			}
			__syncthreads();
			const uint32_t here = min(total - base, (uint32_t)kList);
			if constexpr (!kLamps) {
				for (uint32_t j = tid; j < here; j += kThreads) {
					const int entry = list[j], t = entry >> 5, b = entry & 31;
					const int x = tx0 + t / kTile, z = tz0 + t % kTile, y = ys + b;
					const int shade = cvxb::VoxelShade(slabNear, any, dims, A.P, x, y, z);
					const uint32_t w32 = (uint32_t)brick[(t / kTile + halo) * stride + (t % kTile + halo)];
					uint32_t *c = A.elements + colourAt[t] + __popc((w32 >> 1) >> b);
					*c = cvxb::ApplyShade(*c, shade, A.P.target);
				}
			} else {
				for (uint32_t j0 = 0u; j0 < here; j0 += kThreads) { // (uniform: CullLamps synchronises the workgroup)
					const uint32_t j = j0 + tid;
					const bool live = j < here;
					const int entry = live ? list[j] : 0, t = entry >> 5, b = entry & 31;
					const int x = tx0 + t / kTile, z = tz0 + t % kTile, y = ys + b;
					int shade = live ? cvxb::VoxelShade(slabNear, any, dims, A.P, x, y, z) : 255;
					for (int first = 0; first < survivors; first += kLampList) {
						if (survivors > kLampList) { (void)CullLamps(A, lampLo, lampHi, first, lampList, lampWaveSum); }
						const int n = min(survivors - first, kLampList);
						for (int l = 0; l < n && shade < 255; l++) {
							const int4 lamp = lampList[l];
							shade += cvxb::LampVoxelTerm(any, x, y, z, lamp.x, lamp.y, lamp.z, lamp.w >> 8, lamp.w & 255);
						}
					}
					if (live) {
						const uint32_t w32 = (uint32_t)brick[(t / kTile + halo) * stride + (t % kTile + halo)];
						uint32_t *c = A.elements + colourAt[t] + __popc((w32 >> 1) >> b);
						*c = cvxb::ApplyShade(*c, min(shade, 255), A.P.target);
					}
				}
			}
			__syncthreads();
		}
		__syncthreads();
	}
}

#endif // !CVX_LIGHT_RECORDS

} // namespace cvxlight

using cvxi::Grid;

// cvx_world_light (lamps NULL, lampCount 0) and cvx_world_light_lamps
static int Light(cvx_context *ctx, const cvx_light_params *params, const cvx_lamp *lamps, int lampCount, int levelCount, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!params) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "params is NULL"); }
	if (const char *what = cvxb::LightParamsError(*params)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "cvx_light_params: bad %s", what); }
	if (const char *what = cvxb::LampParamsError(lamps, lampCount)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "cvx_lamp: bad %s (lampCount %d)", what, lampCount); }
	if (levelCount < 0 || levelCount >= CVX_LOD_LEVELS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "levelCount %d outside 0 .. %d", levelCount, CVX_LOD_LEVELS - 1); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int dimX = ctx->hostWorld.dimX, dimY = ctx->hostWorld.dimY, dimZ = ctx->hostWorld.dimZ;
	if (outDeviceMs) { *outDeviceMs = 0.f; }
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(params->boxMin, params->boxMax, dimX, dimY, dimZ, &B)) { return CVX_OK; }
	cvxi::EditRectangle R;
	int rc = cvxi::RoundEditRectangle(ctx, B.x0, B.x1, B.z0, B.z1, levelCount, "lighting", &R);
	if (rc != CVX_OK) { return rc; }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	const size_t lampBytes = (size_t)lampCount * sizeof(cvx_lamp);
	cvxlight::LightArgs A{};
	A.W = cvxi::WorldOf(ctx);
	A.B = B;
	A.P = *params;
	A.x0 = R.x0;
	A.z0 = R.z0;
	A.sizeZ = R.sizeZ;
	A.n = R.n;
	A.lampCount = lampCount;
	cvxi::ColumnEditCall call{ "light", CVX_ERR_HIP, "a re-emitted column", "the lit columns" };
	call.extraScratchBytes = lampBytes;
	return cvxi::ColumnEdit(
		ctx, R, levelCount, call,
		[&](const cvxi::ColumnEditJob &J) {
			A.counts = J.counts;
			A.overLimit = J.overLimit;
			A.lamps = reinterpret_cast<const cvx_lamp *>(J.extra);
			const hipError_t e = lampCount > 0 ? hipMemcpyAsync(J.extra, lamps, lampBytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
			if (e == hipSuccess) { hipLaunchKernelGGL(cvxlight::light_count_kernel, dim3(Grid((size_t)R.n)), dim3(256), 0, ctx->stream, A); }
			return e;
		},
		[&](const cvxi::ColumnEditJob &J) { // the sub-world blob, then its colours shaded in place
			A.headers = J.headers;
			A.elements = J.elements;
			hipLaunchKernelGGL(cvxlight::light_write_kernel, dim3(Grid((size_t)R.n)), dim3(256), 0, ctx->stream, A);
#ifndef CVX_LIGHT_RECORDS
			const int tilesX = (B.SizeX() + cvxlight::kTile - 1) / cvxlight::kTile;
			A.tilesZ = (B.SizeZ() + cvxlight::kTile - 1) / cvxlight::kTile;
			A.brickSide = cvxlight::kTile + 2 * params->skyRange;
			A.brickStride = A.brickSide | 1;
			const size_t lds = (size_t)A.brickSide * A.brickStride * 8;
			if (lampCount > 0) {
				hipLaunchKernelGGL(cvxlight::light_brick_kernel<true>, dim3((unsigned)(tilesX * A.tilesZ)), dim3(cvxlight::kThreads), lds, ctx->stream, A);
			} else {
				hipLaunchKernelGGL(cvxlight::light_brick_kernel<false>, dim3((unsigned)(tilesX * A.tilesZ)), dim3(cvxlight::kThreads), lds, ctx->stream, A);
			}
#endif
			return hipSuccess;
		},
		outDeviceMs);
}

extern "C" int cvx_world_light(cvx_context *ctx, const cvx_light_params *params, int levelCount, float *outDeviceMs)
{
	return Light(ctx, params, nullptr, 0, levelCount, outDeviceMs);
}

extern "C" int cvx_world_light_lamps(cvx_context *ctx, const cvx_light_params *params, const cvx_lamp *lamps, int lampCount, int levelCount, float *outDeviceMs)
{
	return Light(ctx, params, lamps, lampCount, levelCount, outDeviceMs);
}
