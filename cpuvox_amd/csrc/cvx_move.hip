// cvx_move.hip -- libcpuvox_gpu.so, moving boxes through the device-resident world with collision and sliding (cvx_world_move,
// cvx_world_move_device).  See include/cpuvox_gpu.h for the contract, cvx_move.h for the rule and DESIGN.md section 3.
//
// move_kernel<G>: G consecutive lanes of a wave own one body (64 / G bodies per wave).  The legs of a body run one after the other; inside a leg
// the group's lanes take the leg's columns G at a time -- one 16-byte record load per lane and trip, scattered by column as in pick_kernel, then a
// binary search of the column's runs -- and reduce the nearest blocker with log2 G butterfly shuffles that never leave the group.  Every branch
// around a shuffle depends on reduced values only, so the lanes of a group stay together while the groups of a wave diverge freely.  G = 1 is
// the pick's thread-per-body shape without any shuffle.  Nothing is written but the results.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cvx_context.h"
#include "cvx_move.h"

using cvxi::Fail;

namespace cvxmove {

template <int G>
struct LaneGroup {
	int lane;
	__device__ __forceinline__ int Lane() const { return lane; }
	__device__ __forceinline__ int Size() const { return G; }
	// Min / Max: callers must reach these with the WHOLE group active (every branch around them depends on body fields and reduced values only):
	// a shuffle reads the lanes of its group, and a lane that is not there gives nothing
	__device__ __forceinline__ int32_t Min(int32_t v) const
	{
#pragma unroll
		for (int m = G / 2; m > 0; m >>= 1) {
			const int32_t o = __shfl_xor(v, m, G);
			v = o < v ? o : v;
		}
		return v;
	}
	__device__ __forceinline__ int32_t Max(int32_t v) const
	{
#pragma unroll
		for (int m = G / 2; m > 0; m >>= 1) {
			const int32_t o = __shfl_xor(v, m, G);
			v = o > v ? o : v;
		}
		return v;
	}
};

constexpr int kThreads = 256;

template <int G>
__global__ __launch_bounds__(kThreads) void move_kernel(cvxb::CopyWorld W, int repeat, int bodyCount, const cvx_move_body *bodies, cvx_move_result *results)
{
	const size_t thread = (size_t)blockIdx.x * kThreads + threadIdx.x;
	const size_t i = thread / G; // the same for the G lanes of a group: they leave together
	if (i >= (size_t)bodyCount) { return; }
	const cvx_move_body body = bodies[i];
	const LaneGroup<G> group{ (int)(threadIdx.x % G) };
	const cvx_move_result r = cvxb::MoveBodyValid(body) ? cvxb::MoveBody(W, repeat != 0, body, group) : cvxb::MoveInvalid(body);
	if (group.lane == 0) { results[i] = r; }
}

} // namespace cvxmove

namespace {

template <int G>
void Launch(hipStream_t stream, const cvx_context *ctx, int bodyCount, const cvx_move_body *bodies, cvx_move_result *results)
{
	const size_t threads = (size_t)bodyCount * G;
	const unsigned grid = (unsigned)((threads + cvxmove::kThreads - 1) / cvxmove::kThreads);
	hipLaunchKernelGGL(cvxmove::move_kernel<G>, dim3(grid), dim3(cvxmove::kThreads), 0, stream, cvxi::WorldOf(ctx), ctx->worldRepeat, bodyCount, bodies, results);
}

} // namespace

extern "C" {

int cvx_world_move_device(cvx_context *ctx, int bodyCount, const cvx_move_body *bodiesDevice, cvx_move_result *resultsDevice, int lanesPerBody, void *hipStream)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (bodyCount < 1 || !bodiesDevice || !resultsDevice) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad bodies / results (bodyCount %d)", bodyCount); }
	if (lanesPerBody != 0 && lanesPerBody != 1 && lanesPerBody != 4 && lanesPerBody != 16 && lanesPerBody != 64) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "lanesPerBody %d is not 0, 1, 4, 16 or 64", lanesPerBody);
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	int rc = cvxi::PrepareWorld(ctx);
	if (rc == CVX_OK && ctx->worldRepeat) { rc = cvxi::ValidateRepeat(ctx); }
	if (rc != CVX_OK) { return rc; }
	hipStream_t stream = hipStream ? static_cast<hipStream_t>(hipStream) : ctx->stream;
	switch (lanesPerBody) {
	case 1: Launch<1>(stream, ctx, bodyCount, bodiesDevice, resultsDevice); break;
	case 4: Launch<4>(stream, ctx, bodyCount, bodiesDevice, resultsDevice); break;
	case 64: Launch<64>(stream, ctx, bodyCount, bodiesDevice, resultsDevice); break;
	default: Launch<16>(stream, ctx, bodyCount, bodiesDevice, resultsDevice); break;
	}
	CVX_HIP(ctx, hipGetLastError());
	return CVX_OK;
}

int cvx_world_move(cvx_context *ctx, int bodyCount, const cvx_move_body *bodies, cvx_move_result *results)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (bodyCount < 1 || !bodies || !results) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad bodies / results (bodyCount %d)", bodyCount); }
	int64_t region = 0;
	for (int i = 0; i < bodyCount; i++) {
		if (!cvxb::MoveBodyValid(bodies[i])) {
			return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "body %d: size outside 1 .. %d, |delta| above %d, stepUp outside 0 .. %d, |pos| above 2^28 or unknown flags", i,
			            cvxb::kMoveMaxSize, cvxb::kMoveMaxDelta, cvxb::kMoveMaxStepUp);
		}
		region = std::max(region, cvxb::MoveLegRegion(bodies[i]));
	}
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	const size_t bodiesBytes = ((size_t)bodyCount * sizeof(cvx_move_body) + 255) & ~(size_t)255, resultsBytes = (size_t)bodyCount * sizeof(cvx_move_result);
	if (ctx->pickScratchBytes < bodiesBytes + resultsBytes) { // the pick's scratch: grown on demand, kept
		cvxi::FreeBrushState(ctx);
		CVX_HIP(ctx, hipMalloc(&ctx->pickScratch, bodiesBytes + resultsBytes));
		ctx->pickScratchBytes = bodiesBytes + resultsBytes;
	}
	cvx_move_body *dBodies = static_cast<cvx_move_body *>(ctx->pickScratch);
	cvx_move_result *dResults = reinterpret_cast<cvx_move_result *>(static_cast<uint8_t *>(ctx->pickScratch) + bodiesBytes);
	CVX_HIP(ctx, hipMemcpyAsync(dBodies, bodies, (size_t)bodyCount * sizeof(cvx_move_body), hipMemcpyHostToDevice, ctx->stream));
	const int rc = cvx_world_move_device(ctx, bodyCount, dBodies, dResults, cvxb::MoveLanesFor(region), nullptr);
	if (rc != CVX_OK) { return rc; }
	CVX_HIP(ctx, hipMemcpyAsync(results, dResults, resultsBytes, hipMemcpyDeviceToHost, ctx->stream));
	CVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return CVX_OK;
}

} // extern "C"
