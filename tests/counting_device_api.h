// Counting stand-ins for the runtime calls of cvxi::DeviceApi (cpuvox_amd/csrc/cvx_context.h) and the two symbols that header leaves to
// cvx_gpu.hip, for the host programs that run cvxi::DeviceCall and its users with no device and no library (tests/device_call_rules.cpp,
// tests/model_staging_rules.cpp).  Expect prints one line per failed expectation and counts them in g_failures.
#pragma once

#include <cstdarg>
#include <cstdio>
#include <set>

#include "cvx_context.h"

namespace {

struct Counts {
	std::set<void *> blocks;      // allocated and not yet freed
	std::set<hipEvent_t> events;  // created and not yet destroyed
	int allocated = 0, freed = 0, created = 0, destroyed = 0, recorded = 0, badFree = 0, badDestroy = 0, cleared = 0;
	size_t failAt = 0;            // an allocation of this many bytes runs out of memory
	hipEvent_t lastRecorded = nullptr;
} g;
char g_slots[64];
int g_message = 0;
char g_text[512];

hipError_t Malloc(void **p, size_t bytes)
{
	if (bytes == g.failAt) { return hipErrorOutOfMemory; }
	*p = &g_slots[g.allocated++];
	g.blocks.insert(*p);
	return hipSuccess;
}
hipError_t Free(void *p)
{
	g.freed++;
	g.badFree += g.blocks.erase(p) ? 0 : 1;
	return hipSuccess;
}
hipError_t EventCreate(hipEvent_t *e)
{
	*e = reinterpret_cast<hipEvent_t>(&g_slots[32 + g.created++]);
	g.events.insert(*e);
	return hipSuccess;
}
hipError_t EventRecord(hipEvent_t e, hipStream_t)
{
	g.recorded++;
	g.lastRecorded = e;
	return hipSuccess;
}
hipError_t EventDestroy(hipEvent_t e)
{
	g.destroyed++;
	g.badDestroy += g.events.erase(e) ? 0 : 1;
	return hipSuccess;
}
hipError_t EventElapsedTime(float *ms, hipEvent_t, hipEvent_t)
{
	*ms = 1.5f;
	return hipSuccess;
}
hipError_t GetLastError()
{
	g.cleared++;
	return hipSuccess;
}
const char *GetErrorString(hipError_t) { return "an error"; }

const cvxi::DeviceApi kApi = { Malloc, Free, EventCreate, EventRecord, EventDestroy, EventElapsedTime, GetLastError, GetErrorString };

int g_failures = 0;
void Expect(bool ok, const char *what)
{
	if (!ok) {
		std::printf("FAILED: %s\n", what);
		g_failures++;
	}
}
// everything the stand-ins handed out has come back, each once
void ExpectAllReleased(const char *what)
{
	Expect(g.blocks.empty() && g.events.empty() && g.badFree == 0 && g.badDestroy == 0, what);
}

} // namespace

namespace cvxi {
int Fail(cvx_context *, int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	std::vsnprintf(g_text, sizeof g_text, fmt, ap);
	va_end(ap);
	g_message++;
	return code;
}
const DeviceApi &HipApi() { return kApi; }
} // namespace cvxi
