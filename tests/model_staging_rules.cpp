// Host build of cvxi::ModelStaging (cpuvox_amd/csrc/cvx_model_call.h) for tests/test_model_staging_cpu.py: the plan of the one device block that
// holds a call's host model arrays, and who owns it, run over the counting stand-ins of tests/counting_device_api.h.  No device and no library:
// the copies (Enqueue) are never called.  Prints one line per failed expectation; the exit status is their number.
#include <string>

#include "counting_device_api.h"
#include "cvx_model_call.h"

namespace {

uint32_t g_argb[3 * 5 * 7];
uint8_t g_solid[3 * 5 * 7];

cvx_model Model(int sx, int sy, int sz, bool argb, bool solid) { return cvx_model{ { sx, sy, sz }, 0, argb ? g_argb : nullptr, solid ? g_solid : nullptr }; }
size_t Rounded(size_t bytes) { return (bytes + 15) / 16 * 16; }

// The plan of `models` against the rules: every array of every model in the issue's order, at multiples of 16, one behind the other.
void ExpectPlan(const cvxi::ModelStaging &S, const cvx_model *models, int count)
{
	size_t u = 0, at = 0;
	for (int k = 0; k < count; k++) {
		const size_t n = (size_t)models[k].size[0] * (size_t)models[k].size[1] * (size_t)models[k].size[2];
		const void *from[2] = { models[k].argb, models[k].solid };
		const size_t bytes[2] = { n * 4, n };
		for (int which = 0; which < 2; which++) {
			if (!from[which]) { continue; }
			Expect(u < S.uploads.size(), "a region per array");
			if (u >= S.uploads.size()) { return; }
			const cvxi::ModelStaging::Upload &r = S.uploads[u++];
			Expect(r.at % 16 == 0, "every offset is a multiple of 16");
			Expect(r.at == at && r.bytes == bytes[which] && r.from == from[which], "argb then solid per model, in model order, no gap and no overlap");
			at += Rounded(bytes[which]);
		}
	}
	Expect(u == S.uploads.size(), "no region without an array");
	Expect(S.layout.bytes == at, "the total is the sum of the rounded sizes");
}

// The descriptors after Allocate: into the block exactly where the caller's were not NULL, sizes untouched.
void ExpectPatched(const cvxi::ModelStaging &S, const cvx_model *models, int count)
{
	size_t u = 0;
	for (int k = 0; k < count; k++) {
		const cvx_model &d = S.descriptors[k];
		Expect(d.size[0] == models[k].size[0] && d.size[1] == models[k].size[1] && d.size[2] == models[k].size[2], "sizes are untouched");
		Expect(models[k].argb ? reinterpret_cast<const uint8_t *>(d.argb) == S.block + S.uploads[u++].at : d.argb == nullptr, "argb points into the block or stays NULL");
		Expect(models[k].solid ? d.solid == S.block + S.uploads[u++].at : d.solid == nullptr, "solid points into the block or stays NULL");
	}
}

bool SameDescriptors(const cvxi::ModelStaging &S, const cvx_model *models, int count)
{
	bool same = (int)S.descriptors.size() == count;
	for (int k = 0; k < count && same; k++) {
		same = S.descriptors[k].argb == models[k].argb && S.descriptors[k].solid == models[k].solid && S.descriptors[k].size[0] == models[k].size[0] &&
		       S.descriptors[k].size[1] == models[k].size[1] && S.descriptors[k].size[2] == models[k].size[2];
	}
	return same;
}

} // namespace

int main()
{
	const cvx_model three[3] = { Model(1, 1, 1, true, false), Model(17, 1, 1, false, true), Model(3, 5, 7, true, true) };
	const cvx_model one[1] = { Model(1, 1, 1, false, true) };

	// host arrays: three models, four arrays
	g = Counts{};
	{
		cvxi::ModelStaging S(three, 3, false);
		ExpectPlan(S, three, 3);
		Expect(S.uploads.size() == 4 && S.layout.bytes == 16 + 32 + 432 + 112, "16 + 32 + 432 + 112 bytes");
		Expect(SameDescriptors(S, three, 3) && g.allocated == 0, "the plan allocates and patches nothing");
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(S.Allocate(D) == hipSuccess && g.allocated == 1 && S.block != nullptr, "one block");
		ExpectPatched(S, three, 3);
		Expect(g.freed == 0, "nothing goes before the DeviceCall's destructor");
	}
	Expect(g.allocated == 1 && g.freed == 1, "host arrays: the one block released once");
	ExpectAllReleased("host arrays");

	// the same models on the device: nothing to stage
	g = Counts{};
	{
		cvxi::ModelStaging S(three, 3, true);
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(S.uploads.empty() && S.layout.bytes == 0, "device arrays: no region");
		Expect(S.Allocate(D) == hipSuccess && g.allocated == 0 && S.block == nullptr, "device arrays: nothing is allocated");
		Expect(SameDescriptors(S, three, 3), "device arrays: the descriptors are the caller's");
	}
	Expect(g.allocated == 0 && g.freed == 0, "device arrays: nothing to release");
	ExpectAllReleased("device arrays");

	// the smallest call, and a region of the caller's behind the arrays
	g = Counts{};
	{
		cvxi::ModelStaging S(one, 1, false);
		ExpectPlan(S, one, 1);
		Expect(S.uploads.size() == 1 && S.layout.bytes == 16, "a 1-voxel solid-only model: 16 bytes");
		Expect(S.Add(40, g_argb) == 16 && S.Add(8, nullptr) == 64 && S.layout.bytes == 80, "added regions follow the arrays at multiples of 16");
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		Expect(S.Allocate(D) == hipSuccess && g.allocated == 1, "one block");
		ExpectPatched(S, one, 1);
	}
	Expect(g.allocated == 1 && g.freed == 1, "one model: the one block released once");
	ExpectAllReleased("one model");

	// the block's allocation fails: the error comes back, DeviceCall::Fail reports the plan's total
	g = Counts{};
	g_message = 0;
	{
		cvxi::ModelStaging S(three, 3, false);
		g.failAt = S.layout.bytes;
		cvxi::DeviceCall D(nullptr, "call", nullptr, kApi);
		const hipError_t e = S.Allocate(D);
		Expect(e == hipErrorOutOfMemory && S.block == nullptr && SameDescriptors(S, three, 3), "the failed allocation is returned and nothing is patched");
		Expect(D.Fail(e) == CVX_ERR_CAPACITY && g_message == 1 && std::string(g_text).find(std::to_string(S.layout.bytes)) != std::string::npos, "Fail reports the block's bytes");
	}
	Expect(g.allocated == 0 && g.freed == 0, "failed allocation: nothing to release");
	ExpectAllReleased("failed allocation");

	std::printf("%d failed\n", g_failures);
	return g_failures;
}
