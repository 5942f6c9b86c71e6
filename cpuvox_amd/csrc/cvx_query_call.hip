// cvx_query_call.hip -- the host drivers of the calls that read the world into a caller's arrays or capped list (cvxi::ReadArrays, cvxi::FinishList,
// cvx_context.h): the dense, height-map and model reads; the surface quads, the surface rectangles and a snapshot's changes.  No kernel lives here: the
// callers' launchers enqueue theirs.
#include <algorithm>
#include <cstring>

#include "cvx_context.h"

namespace cvxi {

int ReadArrays(cvx_context *ctx, const char *call, void *const to[3], const size_t bytes[3], bool device, void *hipStream, Launcher<ReadArraysJob> launch,
               float *outDeviceMs)
{
	ReadArraysJob J{};
	if (device) {
		for (int k = 0; k < 3; k++) { J.array[k] = to[k]; }
		J.stream = hipStream ? static_cast<hipStream_t>(hipStream) : ctx->stream;
		(void)launch(J);
		CVX_HIP(ctx, hipGetLastError());
		return CVX_OK;
	}
	DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	size_t at[3], total = 0;
	for (int k = 0; k < 3; k++) {
		at[k] = total;
		total += to[k] ? bytes[k] : 0;
	}
	hipError_t e = D.Allocate(&scratch, total);
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) {
		for (int k = 0; k < 3; k++) { J.array[k] = to[k] ? scratch + at[k] : nullptr; }
		J.stream = ctx->stream;
		e = launch(J);
		if (e == hipSuccess) { e = hipGetLastError(); }
	}
	if (e == hipSuccess) { e = D.End(); }
	for (int k = 0; k < 3; k++) {
		if (e == hipSuccess && to[k]) { e = hipMemcpyAsync(to[k], J.array[k], bytes[k], hipMemcpyDeviceToHost, ctx->stream); }
	}
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (outDeviceMs) { *outDeviceMs = D.Ms(); }
	return CVX_OK;
}

int FinishList(cvx_context *ctx, DeviceCall &D, const ListCall &list, Launcher<ListJob> launchWrite)
{
	const size_t wanted = (size_t)std::min<unsigned long long>(list.found, (unsigned long long)list.capacity), bytes = wanted * list.itemBytes;
	void *back = nullptr;
	uint8_t *staged = nullptr;
	hipError_t e = hipSuccess;
	if (wanted) {
		if (!list.device) {
			back = D.Host(bytes);
			e = D.Allocate(&staged, bytes);
		}
		if (e == hipSuccess) { e = launchWrite(ListJob{ list.device ? list.list : staged, (uint32_t)wanted }); }
		if (e == hipSuccess) { e = hipGetLastError(); }
		if (e == hipSuccess && !list.device) { e = hipMemcpyAsync(back, staged, bytes, hipMemcpyDeviceToHost, ctx->stream); }
	}
	if (e == hipSuccess) { e = D.End(); }
	if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	if (back) { std::memcpy(list.list, back, bytes); }
	return CVX_OK;
}

} // namespace cvxi
