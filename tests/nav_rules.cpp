// Host build of the rules of cvx_world_nav_build / cvx_nav_query (cpuvox_amd/csrc/cvx_nav.h) for tests/test_world_nav_cpu.py, driven
// sequentially: per-column node lists, Bellman-Ford to the fixpoint, the next choice, the query.
//   nav_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <x0> <y0> <z0> <x1> <y1> <z1> <width> <height> <stepUp> <maxDrop> <maxSteps> <goals in> <out>
//     Uploads the LOD-0 blob into a context that never touches a device, builds the field of the box for the goals (int32 triples) and writes
//     the summary (40 bytes, launches = the sweeps made) and the cvx_nav_step (32 bytes) of EVERY voxel position of the world, x-major, then y,
//     then z.  Prints the node count and the milliseconds of the build alone (tools/nav_bench.py: the host route).
//   nav_rules args
//     The argument checks of the five calls on a context without a device or world: one return code per call.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_nav.h"
#include "rules_world.h"
struct HostNodes {
	const uint32_t *lohi;
	uint32_t Lo(uint32_t i) const { return lohi[2 * (size_t)i]; }
	uint32_t Hi(uint32_t i) const { return lohi[2 * (size_t)i + 1]; }
};

struct Field {
	cvxb::NavGrid G;
	cvxb::NavRule R;
	std::vector<uint32_t> offsets, lohi, dist, next;
	cvx_nav_summary summary{};
};

static uint32_t Resolve(const Field &F, int64_t x, int64_t y, int64_t z)
{
	const uint32_t none = F.offsets.back();
	if (!F.G.Holds(x, z)) { return none; }
	const int64_t c = F.G.Column(x, z);
	const uint32_t first = F.offsets[(size_t)c], end = F.offsets[(size_t)c + 1];
	const uint32_t i = cvxb::NavResolve(HostNodes{ F.lohi.data() }, first, end, y);
	return i < end ? i : none;
}

static Field Build(const cvxb::CopyWorld &W, const cvxb::PiecesBox &B, const cvxb::NavRule &R, const int32_t *goals, int goalCount, int maxSteps)
{
	Field F;
	F.G = cvxb::NavGridOf(B, R.w);
	F.R = R;
	const cvxb::NavGrid &G = F.G;
	const int64_t n = G.Columns();
	F.offsets.assign((size_t)n + 1, 0u);
	for (int64_t c = 0; c < n; c++) {
		const uint32_t count = cvxb::NavNodeCount(W, G, G.x0 + c / G.sizeZ, G.z0 + c % G.sizeZ, R);
		F.offsets[(size_t)c + 1] = F.offsets[(size_t)c] + count;
		F.summary.columnsWithSeveralNodes += count >= 2u;
	}
	const uint32_t nodes = F.offsets[(size_t)n];
	F.lohi.assign(2 * (size_t)nodes + 2, 0u);
	for (int64_t c = 0; c < n; c++) {
		cvxb::NavWalk walk = cvxb::NavWalkFrom(W);
		for (uint32_t j = F.offsets[(size_t)c]; j < F.offsets[(size_t)c + 1]; j++) {
			if (!cvxb::NavNextNode(W, G, G.x0 + c / G.sizeZ, G.z0 + c % G.sizeZ, R, &walk, &F.lohi[2 * (size_t)j], &F.lohi[2 * (size_t)j + 1])) { std::exit(5); }
		}
	}
	const HostNodes N{ F.lohi.data() };
	F.dist.assign((size_t)nodes + 1, cvxb::kNavUnreached);
	F.next.assign((size_t)nodes + 1, cvxb::kNavNoNext);
	for (int g = 0; g < goalCount; g++) {
		const uint32_t i = Resolve(F, goals[3 * g], goals[3 * g + 1], goals[3 * g + 2]);
		if (i < nodes) {
			F.dist[i] = 0u;
			F.summary.goalsResolved++;
		}
	}
	auto range = [&](int64_t c, uint32_t *first, uint32_t *end) {
		*first = F.offsets[(size_t)c];
		*end = F.offsets[(size_t)c + 1];
	};
	for (bool changed = true; changed;) {
		changed = false;
		F.summary.launches++;
		for (int64_t c = 0; c < n; c++) {
			const int64_t x = G.x0 + c / G.sizeZ, z = G.z0 + c % G.sizeZ;
			for (uint32_t a = F.offsets[(size_t)c]; a < F.offsets[(size_t)c + 1]; a++) {
				uint32_t low = F.dist[a];
				for (int k = 0; k < 4; k++) {
					const int64_t nx = x + cvxb::NavDirX(k), nz = z + cvxb::NavDirZ(k);
					if (!G.Holds(nx, nz)) { continue; }
					uint32_t first, end;
					range(G.Column(nx, nz), &first, &end);
					cvxb::NavForEachStep(N, N.Lo(a), N.Hi(a), first, end, R, [&](uint32_t b) {
						if (F.dist[b] != cvxb::kNavUnreached && F.dist[b] + 1u < low) { low = F.dist[b] + 1u; }
						return false;
					});
				}
				if (low < F.dist[a] && (maxSteps == 0 || low <= (uint32_t)maxSteps)) {
					F.dist[a] = low;
					changed = true;
				}
			}
		}
	}
	for (int64_t c = 0; c < n; c++) {
		const int64_t x = G.x0 + c / G.sizeZ, z = G.z0 + c % G.sizeZ;
		for (uint32_t a = F.offsets[(size_t)c]; a < F.offsets[(size_t)c + 1]; a++) {
			const uint32_t d = F.dist[a];
			if (d == cvxb::kNavUnreached) { continue; }
			F.summary.reached++;
			if ((int32_t)d > F.summary.largestDistance) { F.summary.largestDistance = (int32_t)d; }
			F.next[a] = d == 0u ? cvxb::kNavAtGoal : cvxb::NavChooseNext(N, G, x, z, N.Lo(a), N.Hi(a), d, R, range, [&](uint32_t b) { return F.dist[b]; });
		}
	}
	F.summary.nodes = nodes;
	return F;
}

static int World(char **argv)
{
	const int dimX = std::atoi(argv[3]), dimY = std::atoi(argv[4]), dimZ = std::atoi(argv[5]), columnCount = std::atoi(argv[6]);
	int32_t boxMin[3], boxMax[3];
	for (int a = 0; a < 3; a++) {
		boxMin[a] = std::atoi(argv[7 + a]);
		boxMax[a] = std::atoi(argv[10 + a]);
	}
	const cvxb::NavRule R{ std::atoi(argv[13]), std::atoi(argv[14]), std::atoi(argv[15]), std::atoi(argv[16]) };
	const int maxSteps = std::atoi(argv[17]);
	if (!cvxb::NavRuleValid(R) || maxSteps < 0) { return 4; }
	const std::vector<uint8_t> goalBytes = ReadFile(argv[18]);
	const int32_t *goals = reinterpret_cast<const int32_t *>(goalBytes.data());
	const int goalCount = (int)(goalBytes.size() / 12);
	const BlobWorld blob = LoadBlobWorld(argv[2], dimX, dimY, dimZ, columnCount);
	const cvxb::CopyWorld &W = blob.W;
	cvxb::PiecesBox B;
	if (!cvxb::PiecesClipBox(boxMin, boxMax, dimX, dimY, dimZ, &B)) { return 4; }
	const auto t0 = std::chrono::steady_clock::now();
	const Field F = Build(W, B, R, goals, goalCount, maxSteps);
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	const uint32_t nodes = F.offsets.back();
	std::vector<cvx_nav_step> steps((size_t)dimX * dimY * dimZ);
	size_t at = 0;
	for (int x = 0; x < dimX; x++) {
		for (int y = 0; y < dimY; y++) {
			for (int z = 0; z < dimZ; z++) {
				const uint32_t i = Resolve(F, x, y, z);
				const bool found = i < nodes;
				steps[at++] = cvxb::NavStepRecord(found, x, found ? F.lohi[2 * (size_t)i] : 0u, z, found ? F.dist[i] : cvxb::kNavUnreached, found ? F.next[i] : cvxb::kNavNoNext);
			}
		}
	}
	FILE *f = std::fopen(argv[19], "wb");
	if (!f) { return 2; }
	std::fwrite(&F.summary, 1, sizeof F.summary, f);
	std::fwrite(steps.data(), sizeof(cvx_nav_step), steps.size(), f);
	std::fclose(f);
	std::printf("nodes %u ms %.3f\n", nodes, ms);
	return 0;
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_nav_field *field = reinterpret_cast<cvx_nav_field *>(ctx); // never dereferenced: every call below fails before it looks at a field
	cvx_nav_summary summary;
	cvx_nav_step steps[2];
	const int32_t goals[6] = { 1, 1, 1, 2, 2, 2 };
	auto params = [](int x1, int y1, int w, int h, int s, int m, int maxSteps) {
		cvx_nav_params p{};
		p.boxMax[0] = x1;
		p.boxMax[1] = y1;
		p.boxMax[2] = 8;
		p.width = w;
		p.height = h;
		p.stepUp = s;
		p.maxDrop = m;
		p.maxSteps = maxSteps;
		return p;
	};
	const cvx_nav_params good = params(8, 8, 2, 3, 1, 4, 0), emptyY = params(8, 0, 2, 3, 1, 4, 0), emptyX = params(-1, 8, 2, 3, 1, 4, 0), wide = params(8, 8, 9, 3, 1, 4, 0),
	                     narrow = params(8, 8, 0, 3, 1, 4, 0), tall = params(8, 8, 2, 65, 1, 4, 0), flat = params(8, 8, 2, 0, 0, 4, 0), climb = params(8, 8, 2, 3, 4, 4, 0),
	                     negativeClimb = params(8, 8, 2, 3, -1, 4, 0), drop = params(8, 8, 2, 3, 1, 4097, 0), negativeDrop = params(8, 8, 2, 3, 1, -1, 0),
	                     steps0 = params(8, 8, 2, 3, 1, 4, -1);
	cvx_nav_field *out = field;
	const int codes[] = {
		cvx_world_nav_build(nullptr, &good, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, nullptr, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &good, nullptr, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &good, goals, 2, nullptr, &summary, nullptr),
		cvx_world_nav_build(ctx, &emptyY, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &emptyX, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &wide, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &narrow, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &tall, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &flat, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &climb, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &negativeClimb, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &drop, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &negativeDrop, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &steps0, goals, 2, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &good, goals, 0, &out, &summary, nullptr),
		cvx_world_nav_build(ctx, &good, goals, CVX_NAV_MAX_GOALS + 1, &out, &summary, nullptr),
		cvx_nav_field_goals(nullptr, field, goals, 2, 0, &summary, nullptr),
		cvx_nav_field_goals(ctx, nullptr, goals, 2, 0, &summary, nullptr),
		cvx_nav_query(nullptr, field, 2, goals, steps),
		cvx_nav_query(ctx, nullptr, 2, goals, steps),
		cvx_nav_query_device(nullptr, field, 2, goals, steps, nullptr),
		cvx_nav_query_device(ctx, nullptr, 2, goals, steps, nullptr),
		cvx_world_nav_build(ctx, &good, goals, 2, &out, nullptr, nullptr), // valid: no world yet
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("%d\n", out == nullptr ? 0 : 1); // every failing build leaves *outField NULL
	cvx_nav_field_destroy(nullptr);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 20 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: nav_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <box: 6> <width> <height> <stepUp> <maxDrop> <maxSteps> <goals in> <out> | args\n");
	return 2;
}
