// Host build of the pair-sweep rules (cpuvox_amd/csrc/cvx_pair_sweep.h) for tests/test_model_sweep_cpu.py.  Its own main: it is also built
// stand-alone with -fsanitize=address,undefined (-DPAIR_SWEEP_RULES_NO_LIBRARY leaves `args` out: the rest calls nothing of the library, so nothing
// of it is linked).
//   pair_sweep_rules cases <cases in> <results out>
//     Each case, as int32 words: tests/pair_contacts_rules.cpp's call (the models, the instances, pairCount and the pairs), then three words of
//     motion per pair.  Every pair goes through cvxb::PairSweepPair, a pose at a time with cvxb::PairOf's own overlap, AND the whole call through
//     the kernel's walk (WaveFirst below: the jobs in order, the pair by the 64-probe search, cvxb::PairSweepJob with the 64 lanes run in turn,
//     the minimum); the two must agree, the jobs' prefix must be the count of the header's R_c one coordinate at a time, and the closed form's
//     offsets the merge loop's (exit code 3 otherwise).  Out per case: the sweeps (56 bytes each), the summary (32 bytes), the pair results of
//     the touching poses (144 bytes each).
//   pair_sweep_rules windows <motions in> <out>
//     Per motion (three words): every window of one axis -- the poses whose offset on that axis lies in [lo, hi], for all lo <= hi around the
//     motion's range, or for a motion with a long component a fixed choice of them -- and some windows of all three axes cut one after the other,
//     by cvxb::PairSweepAxisWindow and PairSweepTakenAt and by the merge loop; exit code 3 where they differ.  Out per motion, two int32 words:
//     the windows compared and how many of them held a pose.
//   pair_sweep_rules args
//     The argument checks of the two calls on a context without a device: per call a line "<return code> <the context's message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef PAIR_SWEEP_RULES_NO_LIBRARY
#include "cvx_context.h"
#endif
#include "cvx_pair_sweep.h"
#include "rules_io.h"

struct PairSweepCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	std::vector<int32_t> pairs, motions;

	const int32_t *Parse(const int32_t *p)
	{
		const int modelCount = *p++;
		argbWords.resize(modelCount);
		solidBytes.resize(modelCount);
		models.resize(modelCount);
		for (int k = 0; k < modelCount; k++) {
			cvx_model &M = models[k];
			for (int a = 0; a < 3; a++) { M.size[a] = *p++; }
			M.pad_ = 0;
			const int hasArgb = *p++, hasSolid = *p++;
			const size_t n = (size_t)M.size[0] * M.size[1] * M.size[2];
			if (hasArgb) {
				argbWords[k].resize(n);
				std::memcpy(argbWords[k].data(), p, n * 4);
				p += n;
			}
			if (hasSolid) {
				solidBytes[k].resize(n);
				for (size_t i = 0; i < n; i++) { solidBytes[k][i] = (uint8_t)(*p++ != 0 ? 1 : 0); }
			}
			M.argb = hasArgb ? argbWords[k].data() : nullptr;
			M.solid = hasSolid ? solidBytes[k].data() : nullptr;
		}
		const int instanceCount = *p++;
		instances.resize(instanceCount);
		std::memcpy(instances.data(), p, (size_t)instanceCount * sizeof(cvx_model_instance));
		p += (size_t)instanceCount * (sizeof(cvx_model_instance) / 4);
		const int pairCount = *p++;
		pairs.assign(p, p + 2 * (size_t)pairCount);
		p += 2 * (size_t)pairCount;
		motions.assign(p, p + 3 * (size_t)pairCount);
		return p + 3 * (size_t)pairCount;
	}
	int PairCount() const { return (int)(pairs.size() / 2); }
};

static void Append(std::vector<uint8_t> *out, const void *p, size_t bytes)
{
	out->insert(out->end(), static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes);
}

// |R_c| of the header, a coordinate at a time.
static int64_t Reach(int32_t aMin, int32_t aMax, int32_t bMin, int32_t bMax, int32_t v)
{
	int64_t count = 0;
	for (int64_t u = aMin; u < aMax; u++) {
		const int64_t lo = v < 0 ? u + v : u, hi = v < 0 ? u : u + v;
		count += hi >= bMin && lo <= (int64_t)bMax - 1 ? 1 : 0;
	}
	return count;
}

// cvx_pair_sweep.hip's kernel with the waves run one after the other and the lanes of a wave too: first[] of every pair.
static bool WaveFirst(const PairSweepCall &C, std::vector<uint32_t> *first, int64_t *jobsOut)
{
	const int n = C.PairCount();
	std::vector<uint32_t> prefix((size_t)n + 1);
	first->assign((size_t)n, cvxb::kSweepNone);
	const int64_t jobs = cvxb::PairSweepJobs(C.instances.data(), C.pairs.data(), C.motions.data(), n, prefix.data());
	if (jobs < 0) { return false; }
	for (int p = 0; p < n; p++) { // the prefix against the rule's own words
		const cvx_model_instance &A = C.instances[C.pairs[2 * p]], &B = C.instances[C.pairs[2 * p + 1]];
		const int32_t *v = C.motions.data() + 3 * (size_t)p;
		const int64_t x = Reach(A.boxMin[0], A.boxMax[0], B.boxMin[0], B.boxMax[0], v[0]), y = Reach(A.boxMin[1], A.boxMax[1], B.boxMin[1], B.boxMax[1], v[1]),
		              z = Reach(A.boxMin[2], A.boxMax[2], B.boxMin[2], B.boxMax[2], v[2]);
		if ((int64_t)prefix[p + 1] - prefix[p] != (y > 0 ? x * z : 0)) {
			std::fprintf(stderr, "pair %d: %lld jobs, the rule counts %lld\n", p, (long long)prefix[p + 1] - prefix[p], (long long)(y > 0 ? x * z : 0));
			return false;
		}
	}
	const cvxb::SameInEveryLane U;
	const cvxb::PairSweepLanesInTurn lanes;
	for (int64_t job = 0; job < jobs; job++) {
		int32_t p = 0, within = n; // the kernel's search: 64 probes a round
		while (within > 1) {
			uint64_t le = 0ull;
			for (int lane = 0; lane < 64; lane++) {
				const int32_t probe = cvxb::PairSearchProbe(p, within, lane);
				if (probe >= 0 && prefix[probe] <= (uint32_t)job) { le |= 1ull << lane; }
			}
			cvxb::PairSearchNarrow(&p, &within, le);
		}
		if (p != cvxb::ContactsPairInstance(prefix.data(), n, (uint32_t)job) || prefix[p + 1] <= (uint32_t)job) { return false; }
		const uint32_t best = cvxb::PairSweepJob(U, lanes, C.models.data(), C.instances.data(), C.pairs.data(), C.motions.data(), p, (uint32_t)job - prefix[p]);
		(*first)[p] = best < (*first)[p] ? best : (*first)[p];
	}
	*jobsOut = jobs;
	return true;
}

// Both forms of one call, compared; the call's bytes appended to `out`.
static bool BothForms(const PairSweepCall &C, std::vector<uint8_t> *out)
{
	const int n = C.PairCount();
	char message[200];
	if (!cvxb::PairSweepValidate(C.models.data(), (int)C.models.size(), C.instances.data(), (int)C.instances.size(), C.pairs.data(), C.motions.data(), n, message, message,
	                             sizeof message)) {
		std::fprintf(stderr, "the case is no valid call: %s\n", message);
		return false;
	}
	int64_t jobs = 0;
	std::vector<uint32_t> first;
	if (!WaveFirst(C, &first, &jobs)) { return false; }
	std::vector<cvxm_pair_sweep_result> sweeps((size_t)n);
	std::vector<cvxp_pair_result> results((size_t)n);
	cvxm_pair_sweeps_summary summary{ 0, 0, jobs, 0 };
	int64_t listed = 0;
	for (int p = 0; p < n; p++) {
		const int32_t *v = C.motions.data() + 3 * (size_t)p, a = C.pairs[2 * p], b = C.pairs[2 * p + 1];
		const int32_t hit = cvxb::PairSweepPair(C.models.data(), C.instances[a], C.instances[b], v);
		sweeps[p] = cvxb::PairSweepResultOf(v, first[p], a, b);
		const cvxs_sweep_result &s = sweeps[p].sweep;
		if (hit != s.hit) {
			std::fprintf(stderr, "pair %d: the wave's hit %d differs from the rule's %d\n", p, s.hit, hit);
			return false;
		}
		// `free` and `at` by the merge loop, not the closed form SweepResultOf uses
		int32_t at[3] = { v[0], v[1], v[2] }, before[3] = { v[0], v[1], v[2] };
		int axis = -1, unused = -1;
		if (hit >= 0 && (!cvxb::SweepOffset(v, hit, at, &axis) || !cvxb::SweepOffset(v, hit > 0 ? hit - 1 : 0, before, &unused))) { return false; }
		if (std::memcmp(at, s.at, sizeof at) != 0 || std::memcmp(before, s.free, sizeof before) != 0 || axis != s.axis) {
			std::fprintf(stderr, "pair %d: the closed form's offsets differ from the merge loop's\n", p);
			return false;
		}
		summary.hits += hit >= 0 ? 1 : 0;
		summary.startsSolid += hit == 0 ? 1 : 0;
		cvx_model_instance two[2] = { C.instances[a], C.instances[b] };
		if (!cvxb::SweepInstanceMoved(C.instances[a], s.at, &two[0])) { return false; }
		cvxb::PairOf(C.models.data(), two, p, 0, 1, &results[p], [](const cvxp_pair_point &) {});
		results[p].a = a;
		results[p].b = b;
		results[p].firstPoint = listed;
		listed += results[p].points;
	}
	Append(out, sweeps.data(), sweeps.size() * sizeof(cvxm_pair_sweep_result));
	Append(out, &summary, sizeof summary);
	Append(out, results.data(), results.size() * sizeof(cvxp_pair_result));
	return true;
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<uint8_t> out;
	while (p < end) {
		PairSweepCall C;
		p = C.Parse(p);
		if (!BothForms(C, &out)) { return 3; }
	}
	return WriteFile(outPath, out.data(), out.size());
}

// ---- windows --------------------------------------------------------------------------------------------------------------------------------------
struct Pose {
	int32_t taken[3];
};

// One comparison: the window of the poses j with lo[c] <= o_c(j) <= hi[c] on every axis c of `axes`, cut in that order.
static bool SameWindow(const int32_t v[3], const std::vector<Pose> &path, const int *axes, int axisCount, const int64_t lo[3], const int64_t hi[3], bool *any)
{
	const int64_t n = (int64_t)path.size() - 1;
	cvxb::PairSweepWindow W{ 0, n, 0, 0 };
	for (int i = 0; i < axisCount; i++) { cvxb::PairSweepAxisWindow(v, axes[i], lo[axes[i]], hi[axes[i]], &W); }
	int64_t j0 = -1, j1 = -2;
	for (int64_t j = 0; j <= n; j++) {
		bool inside = true;
		for (int i = 0; i < axisCount; i++) {
			const int64_t o = (int64_t)cvxb::SweepSign(v[axes[i]]) * path[(size_t)j].taken[axes[i]];
			inside = inside && o >= lo[axes[i]] && o <= hi[axes[i]];
		}
		if (!inside) { continue; }
		if (j0 >= 0 && j != j1 + 1) { return false; } // (an interval: every offset is monotone)
		j0 = j0 < 0 ? j : j0;
		j1 = j;
	}
	*any = j0 >= 0;
	if (j0 < 0) { return W.j0 > W.j1; }
	if (W.j0 != j0 || W.j1 != j1) { return false; }
	int32_t taken[3];
	cvxb::PairSweepTakenAt(v, W, taken);
	return std::memcmp(taken, path[(size_t)j0].taken, sizeof taken) == 0;
}

static int Windows(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	std::vector<int32_t> out;
	for (size_t at = 0; at + 3 <= words.size(); at += 3) {
		const int32_t *v = words.data() + at;
		std::vector<Pose> path;
		int32_t taken[3] = { 0, 0, 0 };
		do { path.push_back(Pose{ { taken[0], taken[1], taken[2] } }); } while (cvxb::SweepPathNext(v, taken) >= 0);
		if ((int64_t)path.size() != cvxb::SweepSteps(v) + 1) { return 3; }
		int32_t compared = 0, held = 0;
		uint32_t seed = 12345u + (uint32_t)(v[0] * 31 + v[1] * 17 + v[2]);
		const bool isLong = cvxb::SweepAbs(v[0]) > 64 || cvxb::SweepAbs(v[1]) > 64 || cvxb::SweepAbs(v[2]) > 64;
		std::vector<int64_t> bounds[3];
		for (int c = 0; c < 3; c++) {
			const int64_t n = cvxb::SweepAbs(v[c]);
			if (isLong) {
				for (const int64_t b : { -n - 1, -n, -n + 1, -n / 2, (int64_t)-1, (int64_t)0, (int64_t)1, n / 3, n - 1, n, n + 1 }) { bounds[c].push_back(b); }
			} else {
				for (int64_t b = -n - 1; b <= n + 1; b++) { bounds[c].push_back(b); }
			}
		}
		for (int c = 0; c < 3; c++) {
			for (const int64_t l : bounds[c]) {
				for (const int64_t h : bounds[c]) {
					if (l > h) { continue; }
					int64_t lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
					lo[c] = l;
					hi[c] = h;
					bool any = false;
					if (!SameWindow(v, path, &c, 1, lo, hi, &any)) {
						std::fprintf(stderr, "motion (%d, %d, %d): axis %d, [%lld, %lld]\n", v[0], v[1], v[2], c, (long long)l, (long long)h);
						return 3;
					}
					compared++;
					held += any ? 1 : 0;
				}
			}
		}
		const int orders[3][3] = { { 0, 2, 1 }, { 1, 0, 2 }, { 2, 1, 0 } }; // (the kernel's is the first)
		for (int k = 0; k < (isLong ? 12 : 48); k++) {
			int64_t lo[3], hi[3];
			for (int c = 0; c < 3; c++) {
				seed = seed * 1664525u + 1013904223u;
				const int64_t a = bounds[c][(seed >> 8) % bounds[c].size()];
				seed = seed * 1664525u + 1013904223u;
				const int64_t b = bounds[c][(seed >> 8) % bounds[c].size()];
				lo[c] = a < b ? a : b;
				hi[c] = a < b ? b : a;
			}
			bool any = false;
			if (!SameWindow(v, path, orders[k % 3], 3, lo, hi, &any)) {
				std::fprintf(stderr, "motion (%d, %d, %d): the three axes cut one after the other\n", v[0], v[1], v[2]);
				return 3;
			}
			compared++;
			held += any ? 1 : 0;
		}
		out.push_back(compared);
		out.push_back(held);
	}
	return WriteFile(outPath, out);
}

#ifndef PAIR_SWEEP_RULES_NO_LIBRARY
static int Args()
{
	cvx_context context;
	cvx_context *ctx = &context;
	uint32_t argb[8] = {};
	uint8_t solid[8] = {};
	const cvx_model good{ { 2, 2, 2 }, 0, argb, solid }, neither{ { 2, 2, 2 }, 0, nullptr, nullptr };
	cvx_model_instance I{};
	for (int a = 0; a < 3; a++) {
		I.toModel.m[a][a] = 65536;
		I.boxMax[a] = 2;
	}
	I.op = 77; // (not read)
	auto with = [&](auto change) {
		cvx_model_instance k = I;
		change(k);
		return k;
	};
	const cvx_model_instance two[2] = { I, I };
	const cvx_model_instance emptyBox[2] = { I, with([](cvx_model_instance &k) { k.boxMax[1] = 0; }) };
	const cvx_model_instance nearEdge[2] = { I, with([](cvx_model_instance &k) { k.boxMin[0] = (1 << 30) - 12; k.boxMax[0] = (1 << 30) - 10; }) };
	const cvx_model_instance nearT[2] = { with([](cvx_model_instance &k) { k.toModel.t[1] = -((int64_t)1 << 46) + 65536; }), I };
	const cvx_model_instance wideOne = with([](cvx_model_instance &k) { k.boxMin[0] = k.boxMin[2] = -(1 << 15); k.boxMax[0] = k.boxMax[2] = 1 << 15; }); // 2^32 columns
	const cvx_model_instance wide[2] = { wideOne, wideOne };
	const int32_t pair01[2] = { 0, 1 }, pair10[2] = { 1, 0 }, beyond[6] = { 0, 1, 1, 0, 1, 2 }, self[4] = { 1, 0, 1, 1 }, both[4] = { 0, 1, 1, 0 };
	std::vector<int32_t> many(2 * (size_t)(CVXP_MAX_PAIRS + 1)), manyStill(3 * (size_t)(CVXP_MAX_PAIRS + 1), 0);
	for (size_t k = 0; k < many.size(); k++) { many[k] = (int32_t)(k & 1); }
	const int32_t still[6] = { 0, 0, 0, 0, 0, 0 }, far[3] = { 0, CVXS_MAX_MOTION + 1, 0 }, farDown[6] = { 0, 0, 0, 0, 0, -CVXS_MAX_MOTION - 1 }, right[3] = { 11, 0, 0 },
	              up[3] = { 0, 2, 0 };
	cvxm_pair_sweep_result sweeps[3];
	cvxp_pair_result contacts[3];
	cvxm_pair_sweeps_summary summary;
	std::memset(sweeps, 0x5A, sizeof sweeps);
	std::memset(contacts, 0x5A, sizeof contacts);
	std::memset(&summary, 0x5A, sizeof summary);
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs, const int32_t *motions, int pairCount,
	                cvxm_pair_sweep_result *s, cvxp_pair_result *c) {
		line(cvxm_pair_sweep(ctx, models, modelCount, instances, instanceCount, pairs, motions, pairCount, s, c, &summary, nullptr));
		line(cvxm_pair_sweep_device(ctx, models, modelCount, instances, instanceCount, pairs, motions, pairCount, s, c, &summary, nullptr));
	};
	std::printf("%d\n", cvxm_pair_sweep(nullptr, &good, 1, two, 2, pair01, still, 1, sweeps, contacts, &summary, nullptr));
	std::printf("%d\n", cvxm_pair_sweep_device(nullptr, &good, 1, two, 2, pair01, still, 1, sweeps, contacts, &summary, nullptr));
	// cvxp_model_contacts' checks of models, instances and pairs (every one of them: tests/test_model_contacts_cpu.py, through the same function)
	call(nullptr, 1, two, 2, pair01, still, 1, sweeps, contacts);
	call(&good, 1, two, CVX_MODELS_MAX_INSTANCES + 1, pair01, still, 1, sweeps, contacts);
	call(&neither, 1, two, 2, pair01, still, 1, sweeps, contacts);
	call(&good, 1, emptyBox, 2, pair01, still, 1, sweeps, contacts);
	call(&good, 1, two, 2, nullptr, still, 1, sweeps, contacts);
	call(&good, 1, two, 2, pair01, still, 0, sweeps, contacts);
	call(&good, 1, two, 2, many.data(), manyStill.data(), CVXP_MAX_PAIRS + 1, sweeps, contacts);
	call(&good, 1, two, 2, beyond, still, 3, sweeps, contacts);
	call(&good, 1, two, 2, self, still, 2, sweeps, contacts);
	// its own
	call(&good, 1, two, 2, pair01, nullptr, 1, sweeps, contacts);
	call(&good, 1, two, 2, pair01, still, 1, nullptr, contacts);
	call(&good, 1, two, 2, pair01, far, 1, sweeps, contacts);
	call(&good, 1, two, 2, both, farDown, 2, sweeps, contacts);
	call(&good, 1, nearEdge, 2, pair10, right, 1, sweeps, contacts);
	call(&good, 1, nearT, 2, pair01, up, 1, sweeps, contacts);
	// too many jobs: rejected before any device call
	call(&good, 1, wide, 2, pair01, still, 1, sweeps, contacts);
	// every error left the host arrays alone
	for (size_t k = 0; k < sizeof sweeps; k++) { if (reinterpret_cast<const uint8_t *>(sweeps)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof contacts; k++) { if (reinterpret_cast<const uint8_t *>(contacts)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof summary; k++) { if (reinterpret_cast<const uint8_t *>(&summary)[k] != 0x5A) { return 1; } }
	// the same instance beside the edge is fine while it is body b: only I_a + v has to stay inside the limits (no device here: the checks alone)
	char message[200];
	std::printf("%d\n", cvxb::PairSweepValidate(&good, 1, nearEdge, 2, pair01, right, 1, sweeps, message, sizeof message) ? 1 : 0);
	return 0;
}
#endif

int main(int argc, char **argv)
{
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "windows") == 0) { return Windows(argv[2], argv[3]); }
#ifndef PAIR_SWEEP_RULES_NO_LIBRARY
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
#endif
	std::fprintf(stderr, "usage: pair_sweep_rules cases <in> <out> | windows <in> <out> | args\n");
	return 2;
}
