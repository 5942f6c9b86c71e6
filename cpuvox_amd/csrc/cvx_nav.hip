// cvx_nav.hip -- libcpuvox_gpu.so, walking-distance fields over the device-resident world (cvx_world_nav_build, cvx_nav_field_goals,
// cvx_nav_query, cvx_nav_query_device, cvx_nav_field_destroy).  See include/cpuvox_gpu.h for the contract and cvx_nav.h for the rules.
//
// A node is a maximal air interval of a CELL column (the union of the solid runs of its w x w arena columns) that is high enough for the body
// and whose floor lies in the box's y range; a step joins nodes of face-neighbouring cell columns (cvxb::NavStep).  The field keeps, on the
// device, the node offset of every cell column and per node its interval, its distance and its packed `next`; nothing of it points into the
// arena, which is what makes it a snapshot.
//   1. count  (a thread per cell column): its nodes; cvxi::ExclusiveScan gives the node offsets; ONE copy brings the total to the host
//   2. nodes  (a thread per cell column): the [lo, hi) of every node, top-down.  How the arena is read: the walk of cvx_nav.h keeps no state per
//             arena column, so a thread re-reads the 16-byte records of its w x w arena columns and binary-searches their runs on every move.
//             Neighbouring cell columns share w (w - 1) arena columns; consecutive threads are consecutive in z, so a wave's record loads of
//             one (i, k) are one contiguous row segment, and the shared columns come from L1 / L2.  Nothing is staged in LDS here.
//   3. solve  dist = "unreached", goals = 0, then relaxation dist(a) = min(dist(a), 1 + min over steps a -> b of dist(b)); distances only ever
//             fall, and the fixpoint -- the shortest step count -- is unique, so no schedule shows in the result.  nav_relax_kernel: a workgroup
//             of 256 threads per tile of 16 x 16 cell columns, a thread per column, with a one-column halo.  The tile's node intervals and
//             distances (18 x 18 columns, at most kTileNodes nodes: 18 KiB + 1.5 KiB of offsets, under the 20 KiB that leave eight workgroups
//             = 32 waves on a CU of 160 KiB LDS) are staged in LDS and relaxed there for at most kSweeps sweeps or until the tile stops
//             changing; the interior goes back to global memory.  A tile with more nodes relaxes in global memory with the same code on
//             another view.  Steps are re-derived from the intervals every sweep; no edge list is stored.  The host launches until a launch
//             changes nothing (cvx_settle.hip's loop); after launch L every node at distance <= L is final, so more than nodes + 2 launches is
//             a defect and ends in an error return.
//   4. next   (a thread per cell column): `next` of every node from the final distances; reached nodes and the largest distance
//   5. query  (a thread per position): resolve in the column's node list, copy the node's record out
// cvx_nav_field_goals runs 3 and 4 on the field's tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "cvx_context.h"
#include "cvx_nav.h"

using cvxi::Fail;

namespace cvxnav {

using cvxi::Grid;
using cvxi::kThreads;
using cvxi::WaveReduce;

constexpr int kTile = 16;              // interior cell columns of a tile per axis: kTile * kTile = the workgroup's threads
constexpr int kSide = kTile + 2;       // ... with the halo
constexpr int kRowStarts = kSide + 1;  // node offsets of a tile row: one per column and the row's end
constexpr int kTileNodes = 1536;       // LDS budget of the tile path, nodes (halo included)
constexpr int kSweeps = 64;            // sweeps of a tile per launch
static_assert(kTile * kTile == (int)kThreads, "a thread per interior column");
static_assert(kTileNodes * 12 + (kSide * kRowStarts + 2 * kSide + 1) * 4 <= 20 * 1024, "eight workgroups per CU");

struct Totals {
	unsigned long long nodes;   // the count scan's total
	unsigned long long reached;
	unsigned long long several; // cell columns with two or more nodes
	unsigned int goalsResolved;
	unsigned int largest;
	unsigned int changed;       // a relax launch lowered a distance
	unsigned int pad;
};

struct NavTables {
	cvxb::NavGrid G;
	cvxb::NavRule R;
	int n;             // cell columns
	uint32_t nodes;
	uint32_t maxSteps; // 0: no bound
	uint32_t *offsets; // n + 1: the first node of every cell column
	uint32_t *lohi;    // per node: lo, hi
	uint32_t *dist;    // per node
	uint32_t *next;    // per node: packed (cvxb::NavPackNext)
	Totals *totals;
};

struct NavArgs { // the passes that read the arena
	cvxb::CopyWorld W;
	NavTables T;
};

// a node list in global memory
struct FieldNodes {
	const uint32_t *lohi;
	__device__ uint32_t Lo(uint32_t i) const { return lohi[2 * (size_t)i]; }
	__device__ uint32_t Hi(uint32_t i) const { return lohi[2 * (size_t)i + 1]; }
};

__global__ __launch_bounds__(256) void nav_count_kernel(NavArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > A.T.n) { return; }
	if (i == A.T.n) { // (the scan then leaves the node total behind the last column's offset)
		A.T.offsets[i] = 0u;
		return;
	}
	const cvxb::NavGrid &G = A.T.G;
	A.T.offsets[i] = cvxb::NavNodeCount(A.W, G, G.x0 + i / G.sizeZ, G.z0 + i % G.sizeZ, A.T.R);
}

__global__ __launch_bounds__(256) void nav_nodes_kernel(NavArgs A)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t count = 0u;
	if (i < A.T.n) {
		const uint32_t first = A.T.offsets[i];
		count = A.T.offsets[i + 1] - first;
		const cvxb::NavGrid &G = A.T.G;
		const int64_t x = G.x0 + i / G.sizeZ, z = G.z0 + i % G.sizeZ;
		cvxb::NavWalk walk = cvxb::NavWalkFrom(A.W);
		for (uint32_t j = first; j < first + count; j++) { // (bounded by the count of step 1 whatever the walk gives)
			uint32_t lo = 0u, hi = 0u;
			(void)cvxb::NavNextNode(A.W, G, x, z, A.T.R, &walk, &lo, &hi);
			A.T.lohi[2 * (size_t)j] = lo;
			A.T.lohi[2 * (size_t)j + 1] = hi;
		}
	}
	const unsigned long long several = WaveReduce<unsigned long long>(count >= 2u ? 1ull : 0ull, [](unsigned long long a, unsigned long long b) { return a + b; });
	if ((threadIdx.x & 63u) == 0u && several) { atomicAdd(&A.T.totals->several, several); }
}

__global__ __launch_bounds__(256) void nav_init_kernel(NavTables T)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < T.nodes) { T.dist[i] = cvxb::kNavUnreached; }
}

// the node position (px, py, pz) resolves to: T.nodes when none
__device__ inline uint32_t ResolveNode(const NavTables &T, int64_t px, int64_t py, int64_t pz)
{
	if (!T.G.Holds(px, pz)) { return T.nodes; }
	const int64_t c = T.G.Column(px, pz);
	const uint32_t first = T.offsets[c], end = T.offsets[c + 1];
	const uint32_t i = cvxb::NavResolve(FieldNodes{ T.lohi }, first, end, py);
	return i < end ? i : T.nodes;
}

__global__ __launch_bounds__(256) void nav_goals_kernel(NavTables T, const int32_t *goals, int goalCount)
{
	const int g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= goalCount) { return; }
	const uint32_t i = ResolveNode(T, goals[3 * g], goals[3 * g + 1], goals[3 * g + 2]);
	if (i >= T.nodes) { return; }
	T.dist[i] = 0u; // (several goals on one node store the same value)
	atomicAdd(&T.totals->goalsResolved, 1u);
}

// The tile in LDS: the node lists of 18 x 18 columns, row after row; `at` = the thread's own column in `start`.
struct TileView {
	const uint32_t *lo, *hi;
	uint32_t *dist;
	const uint32_t *start;
	int at;
	__device__ uint32_t Lo(uint32_t i) const { return lo[i]; }
	__device__ uint32_t Hi(uint32_t i) const { return hi[i]; }
	__device__ uint32_t Dist(uint32_t i) const { return __hip_atomic_load(dist + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
	__device__ void SetDist(uint32_t i, uint32_t d) const { __hip_atomic_store(dist + i, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
	__device__ void Range(int k, uint32_t *first, uint32_t *end) const
	{
		const int c = at + cvxb::NavDirX(k) * kRowStarts + cvxb::NavDirZ(k);
		*first = start[c];
		*end = start[c + 1];
	}
};

// The same in global memory: (x, z) = the thread's own cell column.
struct FieldView {
	const uint32_t *lohi;
	uint32_t *dist;
	const uint32_t *offsets;
	cvxb::NavGrid G;
	int64_t x, z;
	__device__ uint32_t Lo(uint32_t i) const { return lohi[2 * (size_t)i]; }
	__device__ uint32_t Hi(uint32_t i) const { return lohi[2 * (size_t)i + 1]; }
	__device__ uint32_t Dist(uint32_t i) const { return cvxi::Load(dist + i); }
	__device__ void SetDist(uint32_t i, uint32_t d) const { __hip_atomic_store(dist + i, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	__device__ void Range(int k, uint32_t *first, uint32_t *end) const
	{
		const int64_t nx = x + cvxb::NavDirX(k), nz = z + cvxb::NavDirZ(k);
		*first = *end = 0u;
		if (!G.Holds(nx, nz)) { return; }
		const int64_t c = G.Column(nx, nz);
		*first = offsets[c];
		*end = offsets[c + 1];
	}
};

// One sweep over the nodes [first, end) of the thread's column: true when a distance fell.  A distance read while its owner lowers it is the old
// or the new value, both upper bounds of the true one: the order of the threads does not show in the fixpoint.
template <typename View> __device__ inline bool RelaxColumn(const View &V, const cvxb::NavRule &R, uint32_t maxSteps, uint32_t first, uint32_t end)
{
	bool changed = false;
	for (uint32_t a = first; a < end; a++) {
		const uint32_t best = V.Dist(a);
		if (best == 0u) { continue; }
		const uint32_t lo = V.Lo(a), hi = V.Hi(a);
		uint32_t low = best;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			uint32_t nFirst, nEnd;
			V.Range(k, &nFirst, &nEnd);
			cvxb::NavForEachStep(V, lo, hi, nFirst, nEnd, R, [&](uint32_t b) {
				const uint32_t d = V.Dist(b);
				if (d != cvxb::kNavUnreached && d + 1u < low) { low = d + 1u; }
				return false;
			});
		}
		if (low < best && (maxSteps == 0u || low <= maxSteps)) {
			V.SetDist(a, low);
			changed = true;
		}
	}
	return changed;
}

template <typename View> __device__ inline bool RelaxSweeps(const View &V, const cvxb::NavRule &R, uint32_t maxSteps, uint32_t first, uint32_t end)
{
	bool mine = false;
	for (int sweep = 0; sweep < kSweeps; sweep++) { // (the same trip count for every thread: the decision is the workgroup's)
		const bool changed = RelaxColumn(V, R, maxSteps, first, end);
		mine = mine || changed;
		if (!__syncthreads_or(changed ? 1 : 0)) { break; }
	}
	return mine;
}

__global__ __launch_bounds__(256) void nav_relax_kernel(NavTables T, int tilesZ)
{
	__shared__ uint32_t sLo[kTileNodes], sHi[kTileNodes], sDist[kTileNodes];
	__shared__ uint32_t sStart[kSide * kRowStarts]; // row r, column k: the local index of its first node; [r][kSide]: the row's end
	__shared__ uint32_t sRowBase[kSide + 1];        // the local index of a row's first node
	__shared__ uint32_t sRowGlobal[kSide];          // ... and its global one: a row's nodes are consecutive in both
	const int tid = (int)threadIdx.x;
	const int sizeX = T.G.sizeX, sizeZ = T.G.sizeZ;
	const int cx0 = (int)(blockIdx.x / (unsigned)tilesZ) * kTile, cz0 = (int)(blockIdx.x % (unsigned)tilesZ) * kTile; // grid-relative
	const int zA = cz0 > 0 ? cz0 - 1 : 0, zB = cz0 + kTile + 1 < sizeZ ? cz0 + kTile + 1 : sizeZ;
	if (tid < kSide) {
		const int gx = cx0 - 1 + tid;
		uint32_t first = 0u, length = 0u;
		if (gx >= 0 && gx < sizeX) {
			first = T.offsets[(int64_t)gx * sizeZ + zA];
			length = T.offsets[(int64_t)gx * sizeZ + zB] - first;
		}
		sRowGlobal[tid] = first;
		sRowBase[tid + 1] = length;
	}
	__syncthreads();
	if (tid == 0) {
		sRowBase[0] = 0u;
		for (int r = 0; r < kSide; r++) { sRowBase[r + 1] += sRowBase[r]; }
	}
	__syncthreads();
	const uint32_t total = sRowBase[kSide];
	const int ix = tid / kTile, iz = tid % kTile, gx = cx0 + ix, gz = cz0 + iz;
	bool mine;
	if (total <= (uint32_t)kTileNodes) {
		for (int t = tid; t < kSide * kRowStarts; t += (int)kThreads) {
			const int r = t / kRowStarts, k = t % kRowStarts, x = cx0 - 1 + r;
			int z = cz0 - 1 + k;
			z = z < zA ? zA : (z > zB ? zB : z);
			sStart[t] = sRowBase[r] + (x >= 0 && x < sizeX ? T.offsets[(int64_t)x * sizeZ + z] - sRowGlobal[r] : 0u);
		}
		for (uint32_t j = (uint32_t)tid; j < total; j += kThreads) {
			int r = 0;
			while (r + 1 < kSide && sRowBase[r + 1] <= j) { r++; }
			const uint32_t g = sRowGlobal[r] + (j - sRowBase[r]);
			sLo[j] = T.lohi[2 * (size_t)g];
			sHi[j] = T.lohi[2 * (size_t)g + 1];
			sDist[j] = cvxi::Load(T.dist + g);
		}
		__syncthreads();
		const TileView V{ sLo, sHi, sDist, sStart, (ix + 1) * kRowStarts + iz + 1 };
		const uint32_t first = sStart[V.at], end = sStart[V.at + 1]; // (a column outside the grid has none)
		mine = RelaxSweeps(V, T.R, T.maxSteps, first, end);
		if (mine) {
			for (uint32_t a = first; a < end; a++) {
				__hip_atomic_store(T.dist + sRowGlobal[ix + 1] + (a - sRowBase[ix + 1]), sDist[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
	} else { // the tile's nodes do not fit: the same relaxation on the tables in global memory
		const bool live = gx < sizeX && gz < sizeZ;
		const int64_t c = live ? (int64_t)gx * sizeZ + gz : 0;
		const uint32_t first = live ? T.offsets[c] : 0u, end = live ? T.offsets[c + 1] : 0u;
		const FieldView V{ T.lohi, T.dist, T.offsets, T.G, (int64_t)T.G.x0 + gx, (int64_t)T.G.z0 + gz };
		mine = RelaxSweeps(V, T.R, T.maxSteps, first, end);
	}
	if (__syncthreads_or(mine ? 1 : 0) && tid == 0) { atomicOr(&T.totals->changed, 1u); }
}

__global__ __launch_bounds__(256) void nav_next_kernel(NavTables T)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long reached = 0ull;
	uint32_t largest = 0u;
	if (i < T.n) {
		const int64_t x = T.G.x0 + i / T.G.sizeZ, z = T.G.z0 + i % T.G.sizeZ;
		const FieldNodes N{ T.lohi };
		const uint32_t end = T.offsets[i + 1];
		for (uint32_t a = T.offsets[i]; a < end; a++) {
			const uint32_t d = T.dist[a];
			uint32_t next = cvxb::kNavNoNext;
			if (d == 0u) {
				next = cvxb::kNavAtGoal;
			} else if (d != cvxb::kNavUnreached) {
				next = cvxb::NavChooseNext(N, T.G, x, z, N.Lo(a), N.Hi(a), d, T.R,
				                           [&](int64_t c, uint32_t *first, uint32_t *last) { *first = T.offsets[c]; *last = T.offsets[c + 1]; },
				                           [&](uint32_t b) { return T.dist[b]; });
			}
			T.next[a] = next;
			if (d != cvxb::kNavUnreached) {
				reached++;
				largest = d > largest ? d : largest;
			}
		}
	}
	reached = WaveReduce<unsigned long long>(reached, [](unsigned long long a, unsigned long long b) { return a + b; });
	largest = WaveReduce<uint32_t>(largest, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
	if ((threadIdx.x & 63u) == 0u && reached) {
		atomicAdd(&T.totals->reached, reached);
		atomicMax(&T.totals->largest, largest);
	}
}

__global__ __launch_bounds__(256) void nav_query_kernel(NavTables T, int count, const int32_t *cells, cvx_nav_step *steps)
{
	const int q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= count) { return; }
	const int64_t px = cells[3 * (size_t)q], py = cells[3 * (size_t)q + 1], pz = cells[3 * (size_t)q + 2];
	const uint32_t i = ResolveNode(T, px, py, pz);
	const bool found = i < T.nodes;
	steps[q] = cvxb::NavStepRecord(found, px, found ? T.lohi[2 * (size_t)i] : 0u, pz, found ? T.dist[i] : cvxb::kNavUnreached, found ? T.next[i] : cvxb::kNavNoNext);
}

} // namespace cvxnav

struct cvx_nav_field {
	cvx_context *ctx = nullptr;
	cvxnav::NavTables T{};
	uint8_t *columnMem = nullptr, *nodeMem = nullptr; // totals and offsets; lohi, dist and next
	int64_t several = 0;
};

namespace cvxnav {

static int CheckGoals(cvx_context *ctx, const int32_t *goals, int goalCount, int maxSteps)
{
	if (!goals) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "goals is NULL"); }
	if (goalCount < 1 || goalCount > CVX_NAV_MAX_GOALS) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "goalCount %d outside 1 .. %d", goalCount, CVX_NAV_MAX_GOALS); }
	if (maxSteps < 0) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "maxSteps %d is negative", maxSteps); }
	return CVX_OK;
}

// Steps 3 and 4 on the field's tables, in the caller's DeviceCall: where the caller has begun it in front of its own passes, the time covers those too.
static int Solve(cvx_context *ctx, const char *call, cvxi::DeviceCall &D, cvx_nav_field *F, const int32_t *goals, int goalCount, int maxSteps, cvx_nav_summary *summary,
                 float *outDeviceMs)
{
	cvx_nav_summary S{};
	S.nodes = (int64_t)F->T.nodes;
	S.columnsWithSeveralNodes = F->several;
	float ms = 0.f;
	if (F->T.nodes) {
		NavTables &T = F->T;
		T.maxSteps = (uint32_t)maxSteps;
		int32_t *dGoals = nullptr;
		Totals host{};
		host.nodes = T.nodes;
		host.several = (unsigned long long)F->several;
		hipError_t e = D.Event(0) ? hipSuccess : D.Begin();
		if (e == hipSuccess) { e = D.Allocate(&dGoals, (size_t)goalCount * 12); }
		if (e == hipSuccess) { e = hipMemcpyAsync(dGoals, goals, (size_t)goalCount * 12, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) { e = hipMemcpyAsync(T.totals, &host, sizeof host, hipMemcpyHostToDevice, ctx->stream); }
		if (e == hipSuccess) {
			hipLaunchKernelGGL(nav_init_kernel, dim3(Grid(T.nodes)), dim3(kThreads), 0, ctx->stream, T);
			hipLaunchKernelGGL(nav_goals_kernel, dim3(Grid((size_t)goalCount)), dim3(kThreads), 0, ctx->stream, T, dGoals, goalCount);
			e = hipGetLastError();
		}
		const int tilesX = (T.G.sizeX + kTile - 1) / kTile, tilesZ = (T.G.sizeZ + kTile - 1) / kTile;
		const int64_t bound = (int64_t)T.nodes + 2;
		int64_t launches = 0;
		if (e == hipSuccess) {
			launches = cvxi::LaunchUntilUnchanged(
				ctx, &T.totals->changed, bound,
				[&](const int64_t &) {
					hipLaunchKernelGGL(nav_relax_kernel, dim3((unsigned)((int64_t)tilesX * tilesZ)), dim3(kThreads), 0, ctx->stream, T, tilesZ);
					return hipSuccess;
				},
				&e);
			if (launches < 0) { return Fail(ctx, CVX_ERR_HIP, "%s: the relaxation of %u nodes did not settle in %lld launches", call, T.nodes, (long long)bound); }
		}
		if (e == hipSuccess) {
			hipLaunchKernelGGL(nav_next_kernel, dim3(Grid((size_t)T.n)), dim3(kThreads), 0, ctx->stream, T);
			e = hipGetLastError();
		}
		if (e == hipSuccess) { e = hipMemcpyAsync(&host, T.totals, sizeof host, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = D.End(); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return D.Fail(e); }
		ms = D.Ms();
		S.reached = (int64_t)host.reached;
		S.goalsResolved = (int32_t)host.goalsResolved;
		S.largestDistance = (int32_t)host.largest;
		S.launches = (int32_t)std::min<int64_t>(launches, INT32_MAX);
	}
	if (summary) { *summary = S; }
	if (outDeviceMs) { *outDeviceMs = ms; }
	return CVX_OK;
}

} // namespace cvxnav

extern "C" {

void cvx_nav_field_destroy(cvx_nav_field *field)
{
	if (!field) { return; }
	if (field->columnMem || field->nodeMem) { (void)hipSetDevice(field->ctx->device); }
	if (field->columnMem) { (void)hipFree(field->columnMem); }
	if (field->nodeMem) { (void)hipFree(field->nodeMem); }
	delete field;
}

int cvx_world_nav_build(cvx_context *ctx, const cvx_nav_params *params, const int32_t *goals, int goalCount, cvx_nav_field **outField, cvx_nav_summary *summary,
                        float *outDeviceMs)
{
	using namespace cvxnav;
	static const char *const call = "cvx_world_nav_build";
	if (outField) { *outField = nullptr; }
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!params || !outField) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "params or outField is NULL"); }
	const cvx_nav_params P = *params;
	char bad[cvxb::kBoxMessage];
	if (cvxb::BoxCheck(P.boxMin, P.boxMax, 0, bad, sizeof bad)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "%s", bad); }
	const cvxb::NavRule R{ P.width, P.height, P.stepUp, P.maxDrop };
	if (!cvxb::NavRuleValid(R)) {
		return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "width %d outside 1 .. %d, height %d outside 1 .. %d, stepUp %d outside 0 .. height or maxDrop %d outside 0 .. %d", P.width,
		            cvxb::kNavMaxWidth, P.height, cvxb::kNavMaxHeight, P.stepUp, P.maxDrop, cvxb::kNavMaxDrop);
	}
	int rc = CheckGoals(ctx, goals, goalCount, P.maxSteps);
	if (rc != CVX_OK) { return rc; }
	if (const int refused = cvxi::RequireWorld(ctx)) { return refused; }
	const int dim[3] = { ctx->hostWorld.dimX, ctx->hostWorld.dimY, ctx->hostWorld.dimZ };
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(P.boxMin, P.boxMax, dim[0], dim[1], dim[2], &B)) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "the box lies outside the world"); }
	NavArgs A{};
	A.T.G = cvxb::NavGridOf(B, R.w);
	A.T.R = R;
	if (A.T.G.Columns() >= ((int64_t)1 << 31) - 1) { return Fail(ctx, CVX_ERR_CAPACITY, "a field of %lld cell columns", (long long)A.T.G.Columns()); }
	if (const int refused = cvxi::PrepareWorld(ctx)) { return refused; }
	cvx_nav_field *F = new (std::nothrow) cvx_nav_field();
	if (!F) { return Fail(ctx, CVX_ERR_CAPACITY, "out of host memory"); }
	F->ctx = ctx;
	const int n = (int)A.T.G.Columns();
	A.T.n = n;
	F->T = A.T;
	cvxi::DeviceCall D(ctx, call);
	if (n == 0) { // a box narrower than the body: the empty field
		*outField = F;
		return Solve(ctx, call, D, F, goals, goalCount, P.maxSteps, summary, outDeviceMs);
	}

	uint8_t *columnMem = nullptr, *nodeMem = nullptr, *scanMem = nullptr;
	auto fail = [&](int code) {
		cvx_nav_field_destroy(F);
		return code;
	};
	// 1. the nodes of every cell column, their offsets, the total
	const size_t offsetsAt = (sizeof(Totals) + 15) & ~(size_t)15;
	const size_t chunks = ((size_t)n + 1 + cvxi::ScanChunk() - 1) / cvxi::ScanChunk();
	Totals host{};
	hipError_t e = D.Allocate(&columnMem, offsetsAt + ((size_t)n + 1) * 4);
	if (e == hipSuccess) { e = D.Allocate(&scanMem, chunks * 8); } // (a few KiB, held to the end of the call with the rest)
	if (e == hipSuccess) { e = D.Begin(); }
	if (e == hipSuccess) { e = hipMemcpyAsync(columnMem, &host, sizeof host, hipMemcpyHostToDevice, ctx->stream); }
	if (e == hipSuccess) {
		A.W = cvxi::WorldOf(ctx);
		A.T.totals = reinterpret_cast<Totals *>(columnMem);
		A.T.offsets = reinterpret_cast<uint32_t *>(columnMem + offsetsAt);
		hipLaunchKernelGGL(nav_count_kernel, dim3(Grid((size_t)n + 1)), dim3(kThreads), 0, ctx->stream, A);
		cvxi::ExclusiveScan(ctx->stream, A.T.offsets, n + 1, reinterpret_cast<unsigned long long *>(scanMem), &A.T.totals->nodes);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host.nodes, &A.T.totals->nodes, sizeof host.nodes, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
	}
	if (e != hipSuccess) { return fail(D.Fail(e)); }
	if (host.nodes >= ((unsigned long long)1 << 31) - 1) { return fail(Fail(ctx, CVX_ERR_CAPACITY, "the field holds %llu nodes", host.nodes)); }
	// 2. the node table
	const size_t nodes = (size_t)host.nodes;
	A.T.nodes = (uint32_t)nodes;
	if (nodes) {
		e = D.Allocate(&nodeMem, nodes * 16);
		if (e != hipSuccess) { return fail(D.Fail(e)); }
		A.T.lohi = reinterpret_cast<uint32_t *>(nodeMem);
		A.T.dist = reinterpret_cast<uint32_t *>(nodeMem + nodes * 8);
		A.T.next = reinterpret_cast<uint32_t *>(nodeMem + nodes * 12);
		hipLaunchKernelGGL(nav_nodes_kernel, dim3(Grid((size_t)n)), dim3(kThreads), 0, ctx->stream, A);
		e = hipGetLastError();
		if (e == hipSuccess) { e = hipMemcpyAsync(&host.several, &A.T.totals->several, sizeof host.several, hipMemcpyDeviceToHost, ctx->stream); }
		if (e == hipSuccess) { e = hipStreamSynchronize(ctx->stream); }
		if (e != hipSuccess) { return fail(D.Fail(e)); }
	}
	F->T = A.T;
	F->several = (int64_t)host.several;
	// 3, 4. the distances and the next cells
	rc = Solve(ctx, call, D, F, goals, goalCount, P.maxSteps, summary, outDeviceMs);
	if (rc != CVX_OK) { return fail(rc); }
	F->columnMem = D.Keep(columnMem);
	F->nodeMem = D.Keep(nodeMem);
	*outField = F;
	return CVX_OK;
}

int cvx_nav_field_goals(cvx_context *ctx, cvx_nav_field *field, const int32_t *goals, int goalCount, int maxSteps, cvx_nav_summary *summary, float *outDeviceMs)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!field || field->ctx != ctx) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, field ? "the field belongs to another context" : "field is NULL"); }
	const int rc = cvxnav::CheckGoals(ctx, goals, goalCount, maxSteps);
	if (rc != CVX_OK) { return rc; }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	static const char *const call = "cvx_nav_field_goals";
	cvxi::DeviceCall D(ctx, call);
	return cvxnav::Solve(ctx, call, D, field, goals, goalCount, maxSteps, summary, outDeviceMs);
}

int cvx_nav_query_device(cvx_context *ctx, const cvx_nav_field *field, int count, const int32_t *cellsDevice, cvx_nav_step *stepsDevice, void *hipStream)
{
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!field || field->ctx != ctx) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, field ? "the field belongs to another context" : "field is NULL"); }
	if (count < 0 || !cellsDevice || !stepsDevice) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad cells / steps (count %d)", count); }
	if (count == 0) { return CVX_OK; }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	hipStream_t stream = hipStream ? static_cast<hipStream_t>(hipStream) : ctx->stream;
	hipLaunchKernelGGL(cvxnav::nav_query_kernel, dim3(cvxnav::Grid((size_t)count)), dim3(cvxnav::kThreads), 0, stream, field->T, count, cellsDevice, stepsDevice);
	CVX_HIP(ctx, hipGetLastError());
	return CVX_OK;
}

int cvx_nav_query(cvx_context *ctx, const cvx_nav_field *field, int count, const int32_t *cells, cvx_nav_step *steps)
{
	static const char *const call = "cvx_nav_query";
	if (!ctx) { return CVX_ERR_INVALID_ARGUMENT; }
	if (!field || field->ctx != ctx) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, field ? "the field belongs to another context" : "field is NULL"); }
	if (count < 0 || !cells || !steps) { return Fail(ctx, CVX_ERR_INVALID_ARGUMENT, "bad cells / steps (count %d)", count); }
	if (count == 0) { return CVX_OK; }
	CVX_HIP(ctx, hipSetDevice(ctx->device));
	const size_t cellsBytes = ((size_t)count * 12 + 255) & ~(size_t)255, stepsBytes = (size_t)count * sizeof(cvx_nav_step);
	cvxi::DeviceCall D(ctx, call);
	uint8_t *scratch = nullptr;
	hipError_t e = D.Allocate(&scratch, cellsBytes + stepsBytes);
	if (e != hipSuccess) { return D.Fail(e); }
	int rc = CVX_OK;
	e = hipMemcpyAsync(scratch, cells, (size_t)count * 12, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) { rc = cvx_nav_query_device(ctx, field, count, reinterpret_cast<const int32_t *>(scratch), reinterpret_cast<cvx_nav_step *>(scratch + cellsBytes), nullptr); }
	if (e == hipSuccess && rc == CVX_OK) { e = hipMemcpyAsync(steps, scratch + cellsBytes, stepsBytes, hipMemcpyDeviceToHost, ctx->stream); }
	if (e == hipSuccess && rc == CVX_OK) { e = hipStreamSynchronize(ctx->stream); }
	if (e != hipSuccess) { return D.Fail(e); }
	return rc;
}

} // extern "C"
