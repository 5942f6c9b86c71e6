// cvx_edit.h -- in-place edits of the device-resident world (cvx_world_set_columns / cvx_world_edit, cvx_edit.hip).
//
// The record rule of cvx_world_upload (cvx_world.hip, shapeOf / codeOf and the record words) restated for ONE column so that it compiles for the
// device AND the host: the edit kernels build the records of the replaced columns with it, and tests/test_world_edit_cpu.py compiles it for the
// host and compares it with what cvx_world_upload writes.  The words are the upload's apart from where the colours (record.x's colorsBase) and
// the run-list block (a listed column's record.z) are placed: the caller fills those in.
#pragma once

#include <stdint.h>

#include "cvx_device.h"

#if defined(__HIPCC__)
#define CVX_HD __host__ __device__
#else
#define CVX_HD
#endif

namespace cvxe {

struct ColumnWords {
	uint32_t x, y, z, w;   // record (cvx_device.h) with colorsBase = 0 and, for a listed column, z = 0
	uint32_t c0, c1;       // counts entry
	uint32_t colours;      // colours the column's runs address (max ColorsIndex + length; what ValidateColumn reports)
	uint32_t solid;        // solid runs
	uint32_t code;         // 1 .. 3: the record holds the runs; 0: listed (or the empty column, x == y == 0)
};

// header: the reference's 12-byte RLEColumn (World.cs:161-169) as three words; elements: the blob's pool.  The column must have passed
// ValidateColumn (cvx_world.hip) for the height dimY >> lod.
CVX_HD inline ColumnWords BuildColumnWords(const uint32_t *header, const uint32_t *elements, int lod, int dimY)
{
	ColumnWords c{};
	const uint32_t off = header[0];
	const uint32_t runCount = header[1] & 0xFFFFu;
	const uint32_t worldMin = header[1] >> 16, worldMax = header[2] & 0xFFFFu;
	if (runCount == 0u) {
		return c;
	}
	uint32_t bottom[3] = { 0u, 0u, 0u }, top[3] = { 0u, 0u, 0u }, position[3] = { 0u, 0u, 0u };
	bool derived = true;
	uint32_t start = 0, sum = 0, colours = 0;
	for (uint32_t r = 0; r < runCount; r++) { // top-down
		const uint32_t raw = elements[off + 1u + r];
		const uint32_t length = raw >> 16;
		if ((int16_t)(raw & 0xFFFFu) >= 0) {
			const uint32_t topY = (uint32_t)dimY - (start << lod), bottomY = topY - (length << lod);
			if (c.solid < 3u) { bottom[c.solid] = bottomY; top[c.solid] = topY; position[c.solid] = r + 1u; }
			if ((raw & 0xFFFFu) != sum) { derived = false; }
			sum += length;
			const uint32_t end = (raw & 0xFFFFu) + length;
			colours = end > colours ? end : colours;
			c.solid++;
		}
		start += length;
	}
	c.code = (c.solid >= 1u && c.solid <= 3u && derived && worldMax == top[0] && worldMin == bottom[c.solid - 1u]) ? c.solid : 0u;
	const uint32_t bounds = worldMin | (worldMax << 16);
	c.x = c.code << 30;
	c.y = bounds;
	if (c.code == 0u) {
		c.z = 0u;
		c.w = c.solid;
	} else {
		c.w = (c.code >= 2u) ? (bottom[0] | ((top[1] - 1u) << 16)) : bounds;
		c.z = (c.code == 3u) ? (bottom[1] | ((top[2] - 1u) << 16)) : worldMin;
	}
	c.c0 = runCount | (position[0] << 16);
	c.c1 = position[1] | (position[2] << 16);
	c.colours = colours;
	return c;
}

// Entry r of a listed column's run-list block (cvx_device.h): every solid run, top-down.  `out` receives `solid` entries.
CVX_HD inline void BuildListedRuns(const uint32_t *header, const uint32_t *elements, int lod, int dimY, uint32_t *out /* 2 words per solid run */)
{
	const uint32_t off = header[0];
	const uint32_t runCount = header[1] & 0xFFFFu;
	uint32_t start = 0, k = 0;
	for (uint32_t r = 0; r < runCount; r++) {
		const uint32_t raw = elements[off + 1u + r];
		const uint32_t length = raw >> 16;
		if ((int16_t)(raw & 0xFFFFu) >= 0) {
			const uint32_t topY = (uint32_t)dimY - (start << lod), bottomY = topY - (length << lod);
			out[2u * k] = bottomY | ((topY - 1u) << 16);
			out[2u * k + 1u] = (raw & 0xFFFFu) | ((r + 1u) << 16);
			k++;
		}
		start += length;
	}
}

// The colours a column of the arena holds, read back from its record (and its run-list block): the number cvx_world_upload sized its place with.
CVX_HD inline uint32_t RecordColours(uint32_t x, uint32_t y, uint32_t z, uint32_t w, const uint32_t *runs /* the level's run list, 2 words per entry */, int lod)
{
	if (x == 0u) {
		return 0u;
	}
	const uint32_t code = x >> 30;
	const uint32_t worldMin = y & 0xFFFFu, worldMax = y >> 16;
	if (code == 1u) {
		return (worldMax - worldMin) >> lod;
	}
	if (code >= 2u) {
		uint32_t n = (worldMax - (w & 0xFFFFu)) + ((w >> 16) + 1u - (z & 0xFFFFu));
		if (code == 3u) { n += (z >> 16) + 1u - worldMin; }
		return n >> lod;
	}
	uint32_t colours = 0;
	for (uint32_t k = 0; k < w; k++) {
		const uint32_t w0 = runs[2u * (z + k)], w1 = runs[2u * (z + k) + 1u];
		const uint32_t end = (w1 & 0xFFFFu) + (((w0 >> 16) + 1u - (w0 & 0xFFFFu)) >> lod);
		colours = end > colours ? end : colours;
	}
	return colours;
}

// Run-list entries a column occupies: a block of its solid runs, rounded up to an even count (16-byte aligned blocks)
CVX_HD inline uint32_t RecordRunEntries(uint32_t x, uint32_t w)
{
	return (x != 0u && (x >> 30) == 0u) ? ((w + 1u) & ~1u) : 0u;
}

} // namespace cvxe
