// cvx_spread.h -- the rules of cvx_world_spread (cvx_spread.hip): travel-distance fields through the air or the solid of a box of the
// device-resident world.
//
// Written once for the device AND the host (tests/test_world_spread_cpu.py compiles it with g++ through tests/spread_rules.cpp and compares it
// with the dense model of tests/spreadmodel.py):
//   SpreadCheck        the argument check, in the order of include/cpuvox_gpu_spread.h (host only: it writes the message)
//   SpreadGrid         the box, the medium, the step mask, the cut; where a voxel lies in the working arrays and in the tile grid
//   SpreadPassable     the contract's Passable(v), from the records (cvxb::ArenaOcc)
//   SpreadChunkVoxel   the same for the init kernel: one voxel of a 64-voxel chunk of a column, from the column's runs that meet the chunk
//                      (one search per chunk and column, a walk of those runs per voxel)
//   SpreadLower / SpreadRelax   the relaxation of one voxel against its up to six predecessors, by value and inside a tile-plus-halo array
//   SpreadFell         which neighbour tiles a lowered voxel concerns
//   SpreadResult       the int32 result of a voxel
//   SpreadTileHost     a workgroup of spread_relax_kernel on the host, a voxel at a time: the specification of the kernel
// Working values are 16 bits: 0 .. 65534 a distance (maxSteps <= CVX_SPREAD_MAX_STEPS is what makes this fit), 0xFFFF unreached.  Every value
// is taken, so blocked is a bit of its own: one passable bit per voxel, 64 voxels of a column per word.  A blocked voxel keeps 0xFFFF for
// good and is never relaxed; as a predecessor it reads as unreached, so the relaxation needs the bit of the voxel it lowers alone.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "cpuvox_gpu_spread.h"
#include "cvx_dense.h"
#include "cvx_light.h"

namespace cvxb {

// the tile a workgroup relaxes: a wave's lanes are the 64 y of a column (y is the arrays' fastest axis), 8 x 8 columns
constexpr int kSpreadTileX = CVX_SPREAD_TILE_X, kSpreadTileY = CVX_SPREAD_TILE_Y, kSpreadTileZ = CVX_SPREAD_TILE_Z;
// ... with its one-voxel halo, laid out like the arrays: (x, z, y), y fastest
constexpr int kSpreadSideX = kSpreadTileX + 2, kSpreadSideY = kSpreadTileY + 2, kSpreadSideZ = kSpreadTileZ + 2;
constexpr int kSpreadStrideZ = kSpreadSideY, kSpreadStrideX = kSpreadSideZ * kSpreadSideY;
constexpr int kSpreadTileCells = kSpreadSideX * kSpreadSideZ * kSpreadSideY; // 6600 values, 13 200 bytes
constexpr int kSpreadSweeps = 64;                                            // sweeps of a tile per launch
constexpr uint32_t kSpreadUnreached = 0xFFFFu;
static_assert(kSpreadTileY == 64, "a passable word is a tile's column");

// The argument check of both calls.  0, or CVX_ERR_INVALID_ARGUMENT with the reason in `message`.
inline int SpreadCheck(const cvx_spread_params *params, const cvx_spread_seed *seeds, int seedCount, const void *out, char *message, size_t size)
{
	if (!params || !seeds || !out) {
		snprintf(message, size, "%s is NULL", !params ? "params" : (!seeds ? "seeds" : "out"));
		return CVX_ERR_INVALID_ARGUMENT;
	}
	const cvx_spread_params &P = *params;
	if (BoxCheck(P.boxMin, P.boxMax, kBoxWithin | kBoxVoxels, message, size)) { return CVX_ERR_INVALID_ARGUMENT; }
	if (P.medium != CVX_SPREAD_AIR && P.medium != CVX_SPREAD_SOLID) {
		snprintf(message, size, "bad medium %d", P.medium);
		return CVX_ERR_INVALID_ARGUMENT;
	}
	if (P.stepFaces == 0) {
		snprintf(message, size, "stepFaces is zero");
		return CVX_ERR_INVALID_ARGUMENT;
	}
	if (P.stepFaces & ~0x3F) {
		snprintf(message, size, "stepFaces 0x%x has bits above 0x3F", P.stepFaces);
		return CVX_ERR_INVALID_ARGUMENT;
	}
	if (P.maxSteps < 1 || P.maxSteps > CVX_SPREAD_MAX_STEPS) {
		snprintf(message, size, "maxSteps %d outside 1 .. %d", P.maxSteps, CVX_SPREAD_MAX_STEPS);
		return CVX_ERR_INVALID_ARGUMENT;
	}
	if (seedCount < 1 || seedCount > CVX_SPREAD_MAX_SEEDS) {
		snprintf(message, size, "seedCount %d outside 1 .. %d", seedCount, CVX_SPREAD_MAX_SEEDS);
		return CVX_ERR_INVALID_ARGUMENT;
	}
	for (int k = 0; k < seedCount; k++) {
		if (seeds[k].start < 0 || seeds[k].start > P.maxSteps) {
			snprintf(message, size, "seed %d: start %d outside 0 .. maxSteps %d", k, seeds[k].start, P.maxSteps);
			return CVX_ERR_INVALID_ARGUMENT;
		}
	}
	return 0;
}

// The checked arguments.  Working arrays, both over the box alone:
//   dist  one 16-bit value per voxel in the result's layout, ((x * size.z + z) * size.y + y), box-relative
//   bits  one word per column and chunk of 64 y: word (x * size.z + z) * TilesY() + (y >> 6), bit y & 63: the voxel is passable
// and one flag per tile, tile (tx, ty, tz) at (tx * TilesZ() + tz) * TilesY() + ty.
struct SpreadGrid {
	DenseBox box;
	int medium, stepFaces;
	uint32_t maxSteps;

	CVX_HD int TilesX() const { return (box.size[0] + kSpreadTileX - 1) / kSpreadTileX; }
	CVX_HD int TilesY() const { return (box.size[1] + kSpreadTileY - 1) / kSpreadTileY; }
	CVX_HD int TilesZ() const { return (box.size[2] + kSpreadTileZ - 1) / kSpreadTileZ; }
	CVX_HD int64_t Tiles() const { return (int64_t)TilesX() * TilesZ() * TilesY(); } // (at most the voxels: below 2^31)
	CVX_HD uint64_t Columns() const { return (uint64_t)box.size[0] * (uint64_t)box.size[2]; }
	CVX_HD uint64_t Elements() const { return Columns() * (uint64_t)box.size[1]; }
	CVX_HD uint64_t Words() const { return Columns() * (uint64_t)TilesY(); }
	CVX_HD bool Holds(int64_t bx, int64_t by, int64_t bz) const { return bx >= 0 && bx < box.size[0] && by >= 0 && by < box.size[1] && bz >= 0 && bz < box.size[2]; }
	CVX_HD uint64_t Column(int64_t bx, int64_t bz) const { return (uint64_t)bx * (uint64_t)box.size[2] + (uint64_t)bz; }
	CVX_HD uint64_t Index(int64_t bx, int64_t by, int64_t bz) const { return Column(bx, bz) * (uint64_t)box.size[1] + (uint64_t)by; }
	CVX_HD uint64_t Word(int64_t bx, int64_t by, int64_t bz) const { return Column(bx, bz) * (uint64_t)TilesY() + (uint64_t)(by >> 6); }
	CVX_HD int64_t Tile(int64_t tx, int64_t ty, int64_t tz) const { return (tx * TilesZ() + tz) * TilesY() + ty; }
	CVX_HD bool Bit(const uint64_t *bits, int64_t bx, int64_t by, int64_t bz) const { return ((bits[Word(bx, by, bz)] >> (by & 63)) & 1ull) != 0ull; }
};

inline SpreadGrid SpreadGridOf(const cvx_spread_params &P)
{
	SpreadGrid G{};
	for (int a = 0; a < 3; a++) {
		G.box.min[a] = P.boxMin[a];
		G.box.size[a] = (int32_t)((int64_t)P.boxMax[a] - P.boxMin[a]);
	}
	G.medium = P.medium;
	G.stepFaces = P.stepFaces;
	G.maxSteps = (uint32_t)P.maxSteps;
	return G;
}

// Passable(v) for the world voxel (x, y, z): in the box, in the world, and of the medium.
CVX_HD inline bool SpreadPassable(const CopyWorld &W, const SpreadGrid &G, int64_t x, int64_t y, int64_t z)
{
	if (!G.Holds(x - G.box.min[0], y - G.box.min[1], z - G.box.min[2])) { return false; }
	if (x < 0 || x >= W.dimX || y < 0 || y >= W.dimY || z < 0 || z >= W.dimZ) { return false; }
	return ArenaOcc{ W }(x, y, z) == (G.medium == CVX_SPREAD_SOLID);
}

// The init kernel's access.  A chunk is the world heights [yLo, yHi) of column (x, z), at most 64 of them; SpreadChunkFirst is the first run
// (0 = the top one) that can meet it -- one search per chunk --, SpreadChunkVoxel whether height y of the chunk is passable: the runs from
// `first` on are walked until one lies wholly below the chunk.  (x, z) outside the world: no column, nothing passable.
CVX_HD inline uint32_t SpreadChunkFirst(const ArenaColumn &col, int64_t yHi) { return RunAtOrBelow(col, yHi - 1); }

CVX_HD inline bool SpreadChunkVoxel(const ArenaColumn &col, uint32_t first, bool inWorld, int64_t dimY, int medium, int64_t yLo, int64_t y)
{
	if (!inWorld || y < 0 || y >= dimY) { return false; }
	bool solid = false;
	const uint32_t count = col.Count();
	for (uint32_t k = first; k < count; k++) {
		const SolidRun run = col.Run(k);
		if ((int64_t)run.top <= yLo) { break; } // this run and every later one lie below the chunk
		solid = solid || ((int64_t)run.bottom <= y && y < (int64_t)run.top);
	}
	return solid == (medium == CVX_SPREAD_SOLID);
}

// The step of face f goes from v - dir(f) to v: where the predecessor of the voxel at `at` of a tile-plus-halo array lies.
CVX_HD inline int SpreadPredecessor(int f)
{
	return f == 0 ? kSpreadStrideX : (f == 1 ? -kSpreadStrideX : (f == 2 ? 1 : (f == 3 ? -1 : (f == 4 ? kSpreadStrideZ : -kSpreadStrideZ))));
}

// A passable voxel with the value `own` whose smallest predecessor holds `least`: the value it takes.  The values are unsigned 16 bits widened
// to 32: 0xFFFF + 1 is above every maxSteps, so unreached and blocked predecessors drop out.
CVX_HD inline uint32_t SpreadLower(uint32_t own, uint32_t least, uint32_t maxSteps)
{
	const uint32_t through = least + 1u;
	return through < own && through <= maxSteps ? through : own;
}

// The relaxation of the passable voxel at `at`: the value it takes, its own or 1 + its smallest predecessor's if that is smaller and within
// the cut.
CVX_HD inline uint32_t SpreadRelax(const uint16_t *tile, int at, int stepFaces, uint32_t maxSteps)
{
	uint32_t least = kSpreadUnreached;
	for (int f = 0; f < 6; f++) {
		if ((stepFaces >> f) & 1) {
			const uint32_t d = tile[at + SpreadPredecessor(f)];
			least = d < least ? d : least;
		}
	}
	return SpreadLower(tile[at], least, maxSteps);
}

// The interior voxel (lx, ly, lz) of a tile, 0 <= l < kSpreadTile, in the tile-plus-halo array.
CVX_HD inline int SpreadCell(int lx, int ly, int lz) { return (lx + 1) * kSpreadStrideX + (lz + 1) * kSpreadStrideZ + ly + 1; }

// A lowered voxel at (lx, ly, lz) of its tile: the faces f (bits) through which a step leaves the tile from it -- the neighbour tiles whose
// halo changed and that can use it.
CVX_HD inline int SpreadFell(int lx, int ly, int lz, int stepFaces)
{
	return ((lx == 0 ? 1 : 0) | (lx == kSpreadTileX - 1 ? 2 : 0) | (ly == 0 ? 4 : 0) | (ly == kSpreadTileY - 1 ? 8 : 0) | (lz == 0 ? 16 : 0) |
	        (lz == kSpreadTileZ - 1 ? 32 : 0)) & stepFaces;
}

// Tile (tx, ty, tz)'s neighbour through face f; -1: the box ends there.
CVX_HD inline int64_t SpreadNeighbourTile(const SpreadGrid &G, int tx, int ty, int tz, int f)
{
	const int nx = tx + (f == 0 ? -1 : (f == 1 ? 1 : 0)), ny = ty + (f == 2 ? -1 : (f == 3 ? 1 : 0)), nz = tz + (f == 4 ? -1 : (f == 5 ? 1 : 0));
	if (nx < 0 || nx >= G.TilesX() || ny < 0 || ny >= G.TilesY() || nz < 0 || nz >= G.TilesZ()) { return -1; }
	return G.Tile(nx, ny, nz);
}

CVX_HD inline int32_t SpreadResult(bool passable, uint32_t working)
{
	return !passable ? CVX_SPREAD_BLOCKED : (working == kSpreadUnreached ? CVX_SPREAD_UNREACHED : (int32_t)working);
}

// ---- the host's walk of the call, the kernels' steps one element at a time --------------------------------------------------------------------

// init: dist and bits of the whole box; returns the passable count.
inline int64_t SpreadInitHost(const CopyWorld &W, const SpreadGrid &G, uint16_t *dist, uint64_t *bits)
{
	int64_t passable = 0;
	for (int64_t bx = 0; bx < G.box.size[0]; bx++) {
		for (int64_t bz = 0; bz < G.box.size[2]; bz++) {
			const int64_t x = G.box.min[0] + bx, z = G.box.min[2] + bz;
			const bool inWorld = x >= 0 && x < W.dimX && z >= 0 && z < W.dimZ;
			const ArenaColumn col = inWorld ? CopyColumnAt(W, x, z) : ArenaColumn{ 0u, 0u, 0u, 0u, W.runs };
			for (int64_t chunk = 0; chunk < G.TilesY(); chunk++) {
				const int64_t yLo = (int64_t)G.box.min[1] + chunk * 64;
				const uint32_t first = SpreadChunkFirst(col, yLo + 64);
				uint64_t word = 0;
				for (int64_t lane = 0; lane < 64 && chunk * 64 + lane < G.box.size[1]; lane++) {
					dist[G.Index(bx, chunk * 64 + lane, bz)] = (uint16_t)kSpreadUnreached;
					if (SpreadChunkVoxel(col, first, inWorld, W.dimY, G.medium, yLo, yLo + lane)) { word |= 1ull << lane; }
				}
				bits[G.Word(bx, chunk * 64, bz)] = word;
				passable += __builtin_popcountll(word);
			}
		}
	}
	return passable;
}

// seeds: the seed's value into dist (the smallest wins), its tile and the six around it active; false: the seed is ignored.
inline bool SpreadSeedHost(const SpreadGrid &G, const cvx_spread_seed &seed, uint16_t *dist, const uint64_t *bits, uint8_t *active)
{
	const int64_t bx = (int64_t)seed.voxel[0] - G.box.min[0], by = (int64_t)seed.voxel[1] - G.box.min[1], bz = (int64_t)seed.voxel[2] - G.box.min[2];
	if (!G.Holds(bx, by, bz) || !G.Bit(bits, bx, by, bz)) { return false; }
	uint16_t &d = dist[G.Index(bx, by, bz)];
	d = (uint32_t)seed.start < d ? (uint16_t)seed.start : d;
	const int tx = (int)(bx / kSpreadTileX), ty = (int)(by / kSpreadTileY), tz = (int)(bz / kSpreadTileZ);
	active[G.Tile(tx, ty, tz)] = 1;
	for (int f = 0; f < 6; f++) {
		const int64_t t = SpreadNeighbourTile(G, tx, ty, tz, f);
		if (t >= 0) { active[t] = 1; }
	}
	return true;
}

// relax: one workgroup of spread_relax_kernel on tile t, which must be active -- the tile and its halo into a local array, sweeps until one
// changes nothing (at most kSpreadSweeps), what fell written back, the neighbours it concerns (and the tile itself, if the sweeps ran out)
// marked in `next`.  Returns whether anything fell.
inline bool SpreadTileHost(const SpreadGrid &G, uint16_t *dist, const uint64_t *bits, int64_t t, uint8_t *next)
{
	const int ty = (int)(t % G.TilesY()), tz = (int)((t / G.TilesY()) % G.TilesZ()), tx = (int)(t / ((int64_t)G.TilesY() * G.TilesZ()));
	static thread_local uint16_t tile[kSpreadTileCells], before[kSpreadTileCells];
	for (int sx = 0; sx < kSpreadSideX; sx++) {
		for (int sz = 0; sz < kSpreadSideZ; sz++) {
			for (int sy = 0; sy < kSpreadSideY; sy++) {
				const int64_t bx = (int64_t)tx * kSpreadTileX + sx - 1, by = (int64_t)ty * kSpreadTileY + sy - 1, bz = (int64_t)tz * kSpreadTileZ + sz - 1;
				const int at = sx * kSpreadStrideX + sz * kSpreadStrideZ + sy;
				before[at] = tile[at] = G.Holds(bx, by, bz) ? dist[G.Index(bx, by, bz)] : (uint16_t)kSpreadUnreached;
			}
		}
	}
	bool more = true;
	for (int sweep = 0; sweep < kSpreadSweeps && more; sweep++) {
		more = false;
		for (int lx = 0; lx < kSpreadTileX; lx++) {
			for (int lz = 0; lz < kSpreadTileZ; lz++) {
				for (int ly = 0; ly < kSpreadTileY; ly++) {
					const int64_t bx = (int64_t)tx * kSpreadTileX + lx, by = (int64_t)ty * kSpreadTileY + ly, bz = (int64_t)tz * kSpreadTileZ + lz;
					if (!G.Holds(bx, by, bz) || !G.Bit(bits, bx, by, bz)) { continue; }
					const int at = SpreadCell(lx, ly, lz);
					const uint32_t v = SpreadRelax(tile, at, G.stepFaces, G.maxSteps);
					if (v < tile[at]) {
						tile[at] = (uint16_t)v;
						more = true;
					}
				}
			}
		}
	}
	int fell = 0;
	bool any = false;
	for (int lx = 0; lx < kSpreadTileX; lx++) {
		for (int lz = 0; lz < kSpreadTileZ; lz++) {
			for (int ly = 0; ly < kSpreadTileY; ly++) {
				const int at = SpreadCell(lx, ly, lz);
				if (tile[at] < before[at]) {
					dist[G.Index((int64_t)tx * kSpreadTileX + lx, (int64_t)ty * kSpreadTileY + ly, (int64_t)tz * kSpreadTileZ + lz)] = tile[at];
					fell |= SpreadFell(lx, ly, lz, G.stepFaces);
					any = true;
				}
			}
		}
	}
	for (int f = 0; f < 6; f++) {
		const int64_t n = (fell >> f) & 1 ? SpreadNeighbourTile(G, tx, ty, tz, f) : -1;
		if (n >= 0) { next[n] = 1; }
	}
	if (more) { next[t] = 1; } // the sweeps ran out before the tile settled
	return any;
}

} // namespace cvxb
