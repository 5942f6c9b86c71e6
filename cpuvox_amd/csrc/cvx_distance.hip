// cvx_distance.hip -- libcpuvox_gpu.so, exact squared-distance fields of boxes of the device-resident world (cvx_world_distance[_device]).
// See include/cpuvox_gpu.h for the contract and cvx_distance.h for the rules.
//
// Three kernels per transform, a thread per element of what each writes; consecutive lanes are consecutive y of a column and go on into the
// next column (z, then x) where the box is lower than a wave, as in dense_read_kernel, so every store is contiguous whatever the box's height:
//   1. along Y  (the footprint grown by R on all four sides): a binary search of the column's runs gives the nearest solid (or air) voxel
//               above and below; its square, capped just above R^2, goes to a 16-bit array.  No voxel is scanned and Y needs no halo.
//   2. along Z  min over |d| <= R of g(z + d) + d^2, outward from d = 0 until d^2 >= the best so far.  The neighbour column at distance d is
//               d * sizeY elements away for every lane: each load of the scan is as contiguous as the store.
//   3. along X  the same over the columns d * sizeZ * sizeY away; values above R^2 become CVX_DISTANCE_FAR and the mode is applied.
// CVX_DISTANCE_SIGNED runs the transform to solid, then the transform to air over the same scratch; its last kernel only touches the elements
// the first left 0 (the solid voxels).  Nothing writes the arena.
#include <hip/hip_runtime.h>

#include "cvx_context.h"
#include "cvx_distance.h"

using cvxi::Fail;

namespace cvxdistance {

constexpr unsigned kThreads = 256;

struct Args {
	cvxb::CopyWorld W;
	cvxb::DistanceGrid G;
	uint16_t *fromY, *fromZ;
	int32_t *out;
};

__device__ __forceinline__ uint64_t Element() { return (uint64_t)blockIdx.x * kThreads + threadIdx.x; }

__global__ __launch_bounds__(kThreads) void distance_y_kernel(Args A, bool toAir)
{
	const uint64_t i = Element();
	if (i >= A.G.ElementsY()) { return; }
	A.fromY[i] = cvxb::DistancePassY(A.W, A.G, i, toAir);
}

__global__ __launch_bounds__(kThreads) void distance_z_kernel(Args A)
{
	const uint64_t i = Element();
	if (i >= A.G.ElementsZ()) { return; }
	A.fromZ[i] = cvxb::DistancePassZ(A.G, A.fromY, i);
}

__global__ __launch_bounds__(kThreads) void distance_x_kernel(Args A, bool signedSecond)
{
	const uint64_t i = Element();
	if (i >= A.G.Elements()) { return; }
	const int32_t previous = signedSecond ? A.out[i] : 0;
	if (signedSecond && previous != 0) { return; }
	A.out[i] = cvxb::DistancePassX(A.G, A.fromZ, i, signedSecond, previous);
}

} // namespace cvxdistance

namespace {

using cvxdistance::kThreads;
using cvxi::Grid;

int Distance(cvx_context *ctx, const char *call, const int32_t boxMin[3], const int32_t boxMax[3], int maxDistance, int mode, int solidOutside, int32_t *out,
             bool device, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	cvxdistance::Args A{};
	int64_t n = 0;
	char bad[cvxb::kBoxMessage];
	if (cvxb::DenseBoxCheck(boxMin, boxMax, &A.G.box, &n, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: %s", call, bad); }
	if (!out) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: out is NULL", call); }
	if (maxDistance < 1 || maxDistance > 255) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: maxDistance %d outside 1 .. 255", call, maxDistance); }
	if (mode < CVX_DISTANCE_TO_SOLID || mode > CVX_DISTANCE_SIGNED) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: bad mode %d", call, mode); }
	if (solidOutside & ~0x3F) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s: solidOutside 0x%x has bits above 0x3F", call, solidOutside); }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	A.G.R = maxDistance;
	A.G.solidOutside = solidOutside;
	// the scratch: 2 bytes per element of the two intermediate arrays (at most 511^2 * 2^31 elements: no overflow); the grids stay below 2^31 blocks
	const uint64_t elementsY = A.G.ElementsY(), elementsZ = A.G.ElementsZ();
	const size_t bytesY = (size_t)((elementsY * 2 + 15) & ~(uint64_t)15), bytesZ = (size_t)((elementsZ * 2 + 15) & ~(uint64_t)15);
	const size_t bytesOut = device ? 0 : (size_t)n * 4;
	if (elementsY >= (uint64_t)1 << 38) {
		return Fail(ctx, CVX_ERR_CAPACITY, "%s: %llu bytes of device memory for the scratch", call, (unsigned long long)(bytesY + bytesZ + bytesOut));
	}
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }

	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	hipError_t e = D.Allocate(&scratch, bytesY + bytesZ + bytesOut);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.fromY = reinterpret_cast<uint16_t *>(scratch);
		A.fromZ = reinterpret_cast<uint16_t *>(scratch + bytesY);
		A.out = device ? out : reinterpret_cast<int32_t *>(scratch + bytesY + bytesZ);
		for (int pass = 0; pass < (mode == CVX_DISTANCE_SIGNED ? 2 : 1); pass++) {
			const bool toAir = mode == CVX_DISTANCE_TO_AIR || pass == 1;
			hipLaunchKernelGGL(cvxdistance::distance_y_kernel, dim3(Grid(elementsY)), dim3(kThreads), 0, ctx->stream, A, toAir);
			hipLaunchKernelGGL(cvxdistance::distance_z_kernel, dim3(Grid(elementsZ)), dim3(kThreads), 0, ctx->stream, A);
			hipLaunchKernelGGL(cvxdistance::distance_x_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, A, pass == 1);
		}
		e = hipGetLastError();
	}
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess && !device) { e = hipMemcpyAsync(out, A.out, bytesOut, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

} // namespace

extern "C" {

int cvx_world_distance(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int maxDistance, int mode, int solidOutside, int32_t *out,
                       float *outDeviceMs)
{
	return Distance(ctx, "cvx_world_distance", boxMin, boxMax, maxDistance, mode, solidOutside, out, false, outDeviceMs);
}

int cvx_world_distance_device(cvx_context *ctx, const int32_t boxMin[3], const int32_t boxMax[3], int maxDistance, int mode, int solidOutside,
                              int32_t *outDevice, float *outDeviceMs)
{
	return Distance(ctx, "cvx_world_distance_device", boxMin, boxMax, maxDistance, mode, solidOutside, outDevice, true, outDeviceMs);
}

} // extern "C"
