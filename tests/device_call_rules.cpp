// Host build of cvxi::DeviceCall (cpuvox_amd/csrc/cvx_context.h) for tests/test_device_call_cpu.py: the owner of a world call's device scratch
// and event pair, run over counting stand-ins for the runtime.  No device and no library: the program defines the two symbols the header
// leaves to cvx_gpu.hip (tests/counting_device_api.h).  Prints one line per failed expectation; the exit status is their number.
#include <string>
#include <type_traits>

#include "counting_device_api.h"

int main()
{
	static_assert(!std::is_copy_constructible_v<cvxi::DeviceCall> && !std::is_copy_assignable_v<cvxi::DeviceCall>, "one owner");
	uint8_t *a = nullptr, *b = nullptr;
	uint32_t *c = nullptr;

	// the success path: two blocks before the first event, one behind it
	g = Counts{};
	{
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(D.Ms() == 0.f, "no time before Begin");
		Expect(D.Allocate(&a, 100) == hipSuccess && D.Allocate(&b, 200) == hipSuccess && a && b && a != b, "two blocks");
		Expect(D.Begin() == hipSuccess && g.created == 2 && g.recorded == 1 && g.lastRecorded == D.Event(0), "Begin creates the pair and records the first event");
		Expect(D.Allocate(&c, 300) == hipSuccess && c, "a block behind Begin");
		Expect(D.End() == hipSuccess && g.recorded == 2 && g.lastRecorded == D.Event(1), "End records the second event");
		Expect(D.Ms() == 1.5f, "the elapsed time");
		Expect(g.freed == 0 && g.destroyed == 0, "nothing goes before the destructor");
	}
	Expect(g.allocated == 3 && g.freed == 3 && g.created == 2 && g.destroyed == 2, "success: three blocks and two events, each released once");
	ExpectAllReleased("success");

	// an early failure after one allocation: the second allocation runs out of memory
	g = Counts{};
	g.failAt = 4096;
	g_message = 0;
	{
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(D.Allocate(&a, 100) == hipSuccess, "the first block");
		const hipError_t e = D.Allocate(&b, 4096);
		Expect(e == hipErrorOutOfMemory && b == nullptr, "the second allocation fails");
		Expect(D.Fail(e) == CVX_ERR_CAPACITY && g.cleared == 1 && g_message == 1, "out of memory: CVX_ERR_CAPACITY, the thread's error cleared");
		Expect(std::string(g_text).find("call") != std::string::npos && std::string(g_text).find("4096") != std::string::npos, "the message names the call and the bytes");
	}
	Expect(g.allocated == 1 && g.freed == 1 && g.created == 0 && g.destroyed == 0, "early failure: the one block released once, no event");
	ExpectAllReleased("early failure");

	// a failure after Begin and before any allocation
	g = Counts{};
	{
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(D.Begin() == hipSuccess, "Begin");
		Expect(D.Fail(hipErrorInvalidValue) == CVX_ERR_HIP && g.cleared == 0, "anything else: CVX_ERR_HIP, nothing cleared");
		Expect(D.Fail(hipErrorOutOfMemory, CVX_ERR_HIP) == CVX_ERR_HIP && g.cleared == 1, "out of memory under a caller's code: cleared all the same");
	}
	Expect(g.allocated == 0 && g.freed == 0 && g.created == 2 && g.destroyed == 2, "failure after Begin: both events released once");
	ExpectAllReleased("failure after Begin");

	// a kept block is the caller's
	g = Counts{};
	{
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(D.Allocate(&a, 100) == hipSuccess && D.Allocate(&b, 200) == hipSuccess, "two blocks");
		Expect(D.Keep(a) == a, "Keep returns the block");
	}
	Expect(g.freed == 1 && g.blocks.size() == 1 && g.blocks.count(a) == 1 && g.badFree == 0, "the kept block is not released, the other is");

	// an adopted start event is the caller's
	g = Counts{};
	{
		hipEvent_t start = nullptr;
		(void)EventCreate(&start);
		{
			cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
			Expect(D.Begin(start) == hipSuccess && g.created == 2 && g.recorded == 0 && D.Event(0) == start, "Begin(start) creates the second event only and records nothing");
			Expect(D.End() == hipSuccess && g.lastRecorded == D.Event(1) && D.Event(1) != start, "End records the adopter's own event");
		}
		Expect(g.destroyed == 1 && g.events.size() == 1 && g.events.count(start) == 1 && g.badDestroy == 0, "the adopted event is not destroyed, the adopter's is");
	}

	// more blocks than the array holds: refused, nothing lost
	g = Counts{};
	{
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		for (int i = 0; i < cvxi::DeviceCall::kBlocks; i++) { Expect(D.Allocate(&a, 8) == hipSuccess, "a block within the array"); }
		Expect(D.Allocate(&a, 8) != hipSuccess && a == nullptr && g.allocated == cvxi::DeviceCall::kBlocks, "one block too many is refused before it is allocated");
	}
	Expect(g.freed == cvxi::DeviceCall::kBlocks, "every block of the full array released");
	ExpectAllReleased("full array");

	std::printf("%d failed\n", g_failures);
	return g_failures;
}
