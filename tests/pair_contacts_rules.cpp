// Host build of the pair-contact rules (cpuvox_amd/csrc/cvx_pair_contacts.h) for tests/test_model_contacts_cpu.py.  Its own main: it is also
// built with -fsanitize=address,undefined as a stand-alone program.
//   pair_contacts_rules cases <cases in> <results out>
//     Each case, as int32 words: tests/models_rules.cpp's call (the models, then the instances), then pairCount and the pairs.  Every pair goes
//     through cvxb::PairOf, a voxel at a time, AND the whole call through the kernels' walk (WaveCall below: the jobs in order, the steps of 64
//     lanes, lane after lane, the job's sums added as the atomics add them, the finish); the two must agree byte for byte (exit code 3
//     otherwise).  Out per case: the results (144 bytes each), the summary (32 bytes), every point (32 bytes each).
//   pair_contacts_rules boxpairs <cases in> <out>
//     Each case: instanceCount, the instances, margin, capacity.  Out per case, as int32 words: the return code, found, then the
//     min(capacity, found) pairs cvxp_box_pairs wrote (behind them a guard word the call must leave alone: exit code 3 otherwise).
//   pair_contacts_rules args
//     The argument checks of the two calls on a context without a device, and of cvxp_box_pairs and cvxp_pair_response: per call a line
//     "<return code> <the context's message>", for the two helpers the return code alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_pair_contacts.h"
#include "rules_io.h"

struct PairsCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	std::vector<int32_t> pairs;

	const int32_t *ParseInstances(const int32_t *p)
	{
		const int instanceCount = *p++;
		instances.resize(instanceCount);
		if (instanceCount) { std::memcpy(instances.data(), p, (size_t)instanceCount * sizeof(cvx_model_instance)); }
		return p + (size_t)instanceCount * (sizeof(cvx_model_instance) / 4);
	}

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
		p = ParseInstances(p);
		const int pairCount = *p++;
		pairs.assign(p, p + 2 * (size_t)pairCount);
		return p + 2 * (size_t)pairCount;
	}
	int PairCount() const { return (int)(pairs.size() / 2); }
};

struct CallResult {
	std::vector<cvxp_pair_result> results;
	std::vector<cvxp_pair_point> points;
	cvxp_pairs_summary summary{};

	void Finish(int64_t jobs) // firstPoint and the summary (cvx_pair_contacts.hip's finish kernel; the box is already [min, max))
	{
		for (cvxp_pair_result &r : results) {
			r.firstPoint = summary.points;
			summary.touching += r.overlap > 0 ? 1 : 0;
			summary.overlap += r.overlap;
			summary.points += r.points;
		}
		summary.jobs = jobs;
	}
};

// The specification: pair after pair, a voxel at a time.  The jobs are counted by their definition: the columns of every X_p.
static CallResult ScalarCall(const PairsCall &C)
{
	CallResult out;
	out.results.resize((size_t)C.PairCount());
	int64_t jobs = 0;
	for (int p = 0; p < C.PairCount(); p++) {
		const int32_t a = C.pairs[2 * p], b = C.pairs[2 * p + 1];
		cvxb::PairOf(C.models.data(), C.instances.data(), p, a, b, &out.results[p], [&](const cvxp_pair_point &point) { out.points.push_back(point); });
		int32_t lo[3], hi[3];
		if (cvxb::PairBox(C.instances[a], C.instances[b], lo, hi)) { jobs += ((int64_t)hi[0] - lo[0]) * ((int64_t)hi[2] - lo[2]); }
	}
	out.Finish(jobs);
	return out;
}

static uint32_t ColourAt(const cvxb::ContactsColumnJob &J, int32_t y)
{
	const int64_t s[3] = { cvxb::ModelMapFinish(J.part[0], J.m1[0], y), cvxb::ModelMapFinish(J.part[1], J.m1[1], y), cvxb::ModelMapFinish(J.part[2], J.m1[2], y) };
	return cvxb::PairModelColour(J.M, s);
}

// cvx_pair_contacts.hip's count and write kernels with the waves run one after the other and the lanes of a wave too.
static CallResult WaveCall(const PairsCall &C)
{
	CallResult out;
	const int n = C.PairCount();
	out.results.resize((size_t)n);
	std::vector<uint32_t> prefix((size_t)n + 1);
	const int64_t jobs = cvxb::PairJobs(C.instances.data(), C.pairs.data(), n, prefix.data());
	if (jobs < 0) { std::exit(4); }
	for (int p = 0; p < n; p++) { cvxb::PairResultInit(C.instances[C.pairs[2 * p]], C.instances[C.pairs[2 * p + 1]], C.pairs[2 * p], C.pairs[2 * p + 1], &out.results[p]); }
	const cvxb::SameInEveryLane U;
	for (int64_t job = 0; job < jobs; job++) {
		int32_t p = 0, within = n; // the wave's search, lane after lane; it must find what the binary search finds
		while (within > 1) {
			uint64_t le = 0ull;
			for (int lane = 0; lane < 64; lane++) {
				const int32_t probe = cvxb::PairSearchProbe(p, within, lane);
				if (probe >= 0 && prefix[probe] <= (uint32_t)job) { le |= 1ull << lane; }
			}
			cvxb::PairSearchNarrow(&p, &within, le);
		}
		if (p != cvxb::ContactsPairInstance(prefix.data(), n, (uint32_t)job)) { std::exit(5); }
		const cvx_model_instance &Ia = C.instances[C.pairs[2 * p]], &Ib = C.instances[C.pairs[2 * p + 1]];
		int32_t lo[3], hi[3];
		if (!cvxb::PairBox(Ia, Ib, lo, hi)) { std::exit(5); } // (the search landed on a pair without jobs)
		const uint32_t sizeZ = (uint32_t)(hi[2] - lo[2]), column = (uint32_t)job - prefix[p];
		const int32_t cx = lo[0] + (int32_t)(column / sizeZ), cz = lo[2] + (int32_t)(column % sizeZ);
		if (cx >= hi[0]) { std::exit(5); }
		const cvxb::PairBodyJob Ja = cvxb::PairBodyJobOf(U, C.models.data(), Ia, cx, cz), Jb = cvxb::PairBodyJobOf(U, C.models.data(), Ib, cx, cz);
		cvxb::PairColumnSums S;
		uint64_t ySum = 0u;
		int32_t top, low;
		cvxb::PairStepRange(Ja, Jb, lo[1], hi[1], &top, &low);
		for (int32_t yTop = top; yTop >= low; yTop -= 64) {
			uint64_t inA = 0ull, inB = 0ull, points = 0ull, faceA[6] = { 0ull, 0ull, 0ull, 0ull, 0ull, 0ull }, faceB[6] = { 0ull, 0ull, 0ull, 0ull, 0ull, 0ull };
			for (int lane = 0; lane < 64; lane++) {
				if (cvxb::ContactsLaneVoxel(Ja.J, yTop - lane)) { inA |= 1ull << lane; }
				if (cvxb::ContactsLaneVoxel(Jb.J, yTop - lane)) { inB |= 1ull << lane; }
			}
			const uint64_t overlap = inA & inB;
			if (overlap == 0ull) { continue; }
			const bool aboveA = cvxb::ContactsLaneVoxel(Ja.J, yTop + 1), belowA = cvxb::ContactsLaneVoxel(Ja.J, yTop - 64);
			const bool aboveB = cvxb::ContactsLaneVoxel(Jb.J, yTop + 1), belowB = cvxb::ContactsLaneVoxel(Jb.J, yTop - 64);
			for (int lane = 0; lane < 64; lane++) {
				if (((overlap >> lane) & 1ull) == 0ull) { continue; }
				const int32_t y = yTop - lane;
				const int facesA = cvxb::PairLaneSideFaces(Ja, y) | cvxb::ContactsLaneEndFaces(inA, aboveA, belowA, lane);
				const int facesB = cvxb::PairLaneSideFaces(Jb, y) | cvxb::ContactsLaneEndFaces(inB, aboveB, belowB, lane);
				for (int f = 0; f < 6; f++) {
					faceA[f] |= (uint64_t)((facesA >> f) & 1) << lane;
					faceB[f] |= (uint64_t)((facesB >> f) & 1) << lane;
				}
				ySum += (uint64_t)(uint32_t)(y - lo[1]);
				if ((facesA | facesB) == 0) { continue; }
				points |= 1ull << lane;
				out.points.push_back(cvxp_pair_point{ { cx, y, cz }, p, facesA, facesB, ColourAt(Ja.J, y), ColourAt(Jb.J, y) }); // (jobs and lanes in order: the scan's offsets)
			}
			cvxb::PairStep(S, overlap, points, faceA, faceB, yTop);
		}
		cvxb::PairColumnDone(S, ySum, cx, cz, &out.results[p]);
	}
	for (cvxp_pair_result &r : out.results) { cvxb::PairResultFinish(&r); }
	out.Finish(jobs);
	return out;
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<uint8_t> out;
	while (p < end) {
		PairsCall C;
		p = C.Parse(p);
		const CallResult a = ScalarCall(C), b = WaveCall(C);
		const size_t resultsBytes = a.results.size() * sizeof(cvxp_pair_result), pointsBytes = a.points.size() * sizeof(cvxp_pair_point);
		if (a.points.size() != b.points.size() || (resultsBytes && std::memcmp(a.results.data(), b.results.data(), resultsBytes) != 0) ||
		    (pointsBytes && std::memcmp(a.points.data(), b.points.data(), pointsBytes) != 0) || std::memcmp(&a.summary, &b.summary, sizeof a.summary) != 0) {
			std::fprintf(stderr, "the wave's results differ from the rule's\n");
			return 3;
		}
		const uint8_t *r = reinterpret_cast<const uint8_t *>(a.results.data()), *s = reinterpret_cast<const uint8_t *>(&a.summary),
		              *q = reinterpret_cast<const uint8_t *>(a.points.data());
		if (resultsBytes) { out.insert(out.end(), r, r + resultsBytes); }
		out.insert(out.end(), s, s + sizeof a.summary);
		if (pointsBytes) { out.insert(out.end(), q, q + pointsBytes); }
	}
	return WriteFile(outPath, out.data(), out.size());
}

static int BoxPairsCases(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<int32_t> out;
	constexpr int32_t kGuard = 0x5A5A5A5A;
	while (p < end) {
		PairsCall C;
		p = C.ParseInstances(p);
		const int margin = *p++, capacity = *p++;
		std::vector<int32_t> pairs(2 * (size_t)capacity + 1, kGuard);
		int64_t found = -1;
		const int code = cvxp_box_pairs(C.instances.data(), (int)C.instances.size(), margin, capacity ? pairs.data() : nullptr, capacity, &found);
		const int64_t written = found < capacity ? found : capacity;
		if (code == CVX_OK && pairs[2 * (size_t)written] != kGuard) { return 3; }
		out.push_back(code);
		out.push_back((int32_t)found);
		if (code == CVX_OK) { out.insert(out.end(), pairs.begin(), pairs.begin() + 2 * written); }
	}
	return WriteFile(outPath, out);
}

static int Args()
{
	cvx_context context;
	cvx_context *ctx = &context;
	uint32_t argb[8] = {};
	uint8_t solid[8] = {};
	const cvx_model good{ { 2, 2, 2 }, 0, argb, solid }, neither{ { 2, 2, 2 }, 0, nullptr, nullptr }, flat{ { 2, 0, 2 }, 0, argb, solid };
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
	const cvx_model_instance badModel[2] = { I, with([](cvx_model_instance &k) { k.model = 1; }) };
	const cvx_model_instance emptyBox[2] = { I, with([](cvx_model_instance &k) { k.boxMax[1] = 0; }) };
	const cvx_model_instance farBox[2] = { with([](cvx_model_instance &k) { k.boxMax[2] = (1 << 30) + 1; }), I };
	const cvx_model_instance bigM[2] = { I, with([](cvx_model_instance &k) { k.toModel.m[1][2] = (1 << 24) + 1; }) };
	const cvx_model_instance bigT[2] = { I, with([](cvx_model_instance &k) { k.toModel.t[2] = -((int64_t)1 << 46) - 1; }) };
	const cvx_model_instance wideOne = with([](cvx_model_instance &k) { k.boxMin[0] = k.boxMin[2] = -(1 << 15); k.boxMax[0] = k.boxMax[2] = 1 << 15; }); // 2^32 columns
	const cvx_model_instance wide[2] = { wideOne, wideOne };
	const int32_t pair01[2] = { 0, 1 }, beyond[6] = { 0, 1, 1, 0, 1, 2 }, negative[2] = { -1, 0 }, self[4] = { 1, 0, 1, 1 };
	std::vector<int32_t> many(2 * (size_t)(CVXP_MAX_PAIRS + 1));
	for (size_t k = 0; k < many.size(); k++) { many[k] = (int32_t)(k & 1); }
	cvxp_pair_result results[3];
	cvxp_pair_point points[2];
	cvxp_pairs_summary summary;
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *pairs, int pairCount, cvxp_pair_result *r,
	                cvxp_pair_point *p, int64_t capacity) {
		line(cvxp_model_contacts(ctx, models, modelCount, instances, instanceCount, pairs, pairCount, r, p, capacity, &summary, nullptr));
		line(cvxp_model_contacts_device(ctx, models, modelCount, instances, instanceCount, pairs, pairCount, r, p, capacity, &summary, nullptr));
	};
	std::memset(results, 0x5A, sizeof results);
	std::memset(points, 0x5A, sizeof points);
	std::printf("%d\n", cvxp_model_contacts(nullptr, &good, 1, two, 2, pair01, 1, results, points, 2, &summary, nullptr));
	std::printf("%d\n", cvxp_model_contacts_device(nullptr, &good, 1, two, 2, pair01, 1, results, points, 2, &summary, nullptr));
	// cvxc_world_contacts' checks of models, instances, boxes and maps
	call(nullptr, 1, two, 2, pair01, 1, results, points, 2);
	call(&good, CVX_MODELS_MAX_MODELS + 1, two, 2, pair01, 1, results, points, 2);
	call(&good, 1, nullptr, 2, pair01, 1, results, points, 2);
	call(&good, 1, two, CVX_MODELS_MAX_INSTANCES + 1, pair01, 1, results, points, 2);
	call(&flat, 1, two, 2, pair01, 1, results, points, 2);
	call(&neither, 1, two, 2, pair01, 1, results, points, 2);
	call(&good, 1, badModel, 2, pair01, 1, results, points, 2);
	call(&good, 1, emptyBox, 2, pair01, 1, results, points, 2);
	call(&good, 1, farBox, 2, pair01, 1, results, points, 2);
	call(&good, 1, bigM, 2, pair01, 1, results, points, 2);
	call(&good, 1, bigT, 2, pair01, 1, results, points, 2);
	// the pairs
	call(&good, 1, two, 2, nullptr, 1, results, points, 2);
	call(&good, 1, two, 2, pair01, 0, results, points, 2);
	call(&good, 1, two, 2, many.data(), CVXP_MAX_PAIRS + 1, results, points, 2);
	call(&good, 1, two, 2, beyond, 3, results, points, 2);
	call(&good, 1, two, 2, negative, 1, results, points, 2);
	call(&good, 1, two, 2, self, 2, results, points, 2);
	// results and the list
	call(&good, 1, two, 2, pair01, 1, nullptr, points, 2);
	call(&good, 1, two, 2, pair01, 1, results, points, -1);
	call(&good, 1, two, 2, pair01, 1, results, nullptr, 2);
	// too many jobs: rejected before any device call, with no world uploaded
	call(&good, 1, wide, 2, pair01, 1, results, points, 2);
	// every error left the host arrays alone
	for (size_t k = 0; k < sizeof results; k++) { if (reinterpret_cast<const uint8_t *>(results)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof points; k++) { if (reinterpret_cast<const uint8_t *>(points)[k] != 0x5A) { return 1; } }
	// the helpers: no context at all
	int32_t listed[2];
	int64_t found = 0;
	std::printf("%d\n", cvxp_box_pairs(nullptr, 1, 0, listed, 1, &found));
	std::printf("%d\n", cvxp_box_pairs(two, -1, 0, listed, 1, &found));
	std::printf("%d\n", cvxp_box_pairs(two, 2, -1, listed, 1, &found));
	std::printf("%d\n", cvxp_box_pairs(two, 2, (1 << 20) + 1, listed, 1, &found));
	std::printf("%d\n", cvxp_box_pairs(two, 2, 0, listed, 1, nullptr));
	std::printf("%d\n", cvxp_box_pairs(two, 2, 0, nullptr, 1, &found));
	std::printf("%d\n", cvxp_box_pairs(two, 2, 0, listed, -1, &found));
	int code = cvxp_box_pairs(two, 2, 1 << 20, nullptr, 0, &found); // valid: counts alone
	std::printf("%d %lld\n", code, (long long)found);
	code = cvxp_box_pairs(nullptr, 0, 0, nullptr, 0, &found); // valid: no instances
	std::printf("%d %lld\n", code, (long long)found);
	cvxp_pair_result r{};
	double centre[3], normal[3], depth;
	std::printf("%d\n", cvxp_pair_response(nullptr, 0, centre, normal, &depth));
	std::printf("%d\n", cvxp_pair_response(&r, 0, centre, normal, &depth));
	r.overlap = -1;
	std::printf("%d\n", cvxp_pair_response(&r, 1, centre, normal, &depth));
	r.overlap = 2;
	std::printf("%d\n", cvxp_pair_response(&r, 2, centre, normal, &depth));
	std::printf("%d\n", cvxp_pair_response(&r, -1, centre, normal, &depth));
	std::printf("%d\n", cvxp_pair_response(&r, 0, nullptr, nullptr, nullptr)); // valid
	std::printf("%d\n", cvxp_pair_response(&r, 1, centre, normal, &depth));    // valid
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "boxpairs") == 0) { return BoxPairsCases(argv[2], argv[3]); }
	std::fprintf(stderr, "usage: pair_contacts_rules cases <in> <out> | boxpairs <in> <out> | args\n");
	return 2;
}
