// Host build of the model-pick rules (cpuvox_amd/csrc/cvx_model_pick.h) for tests/test_model_pick_cpu.py.  Its own main: it is also built with
// -fsanitize=address,undefined as a stand-alone program.
//   model_pick_rules cases <cases in> <results out>
//     Each case, as int32 words: tests/models_rules.cpp's call (the models, then the instances), then rayCount and the rays (8 words each: the
//     bits of cvx_pick_ray).  Every (ray, instance) pair goes through the pair rule a voxel at a time (cvxb::ModelPickSequential), the nearest of
//     a ray's hits chosen by comparing the floats, AND the whole call through the kernels' walk (WaveCall below: the jobs in order, steps of 64
//     layers, lane after lane, the key's minimum, the second walk of the winner); the two must agree byte for byte, job for job (exit code 3
//     otherwise).  Out per case: the hits (48 bytes each), then one int64: the jobs.
//   model_pick_rules args
//     The argument checks of the two calls on a context without a device: per call a line "<return code> <the context's message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_context.h"
#include "cvx_model_pick.h"
#include "rules_io.h"

struct PickCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	std::vector<cvx_pick_ray> rays;

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
		if (instanceCount) { std::memcpy(instances.data(), p, (size_t)instanceCount * sizeof(cvx_model_instance)); }
		p += (size_t)instanceCount * (sizeof(cvx_model_instance) / 4);
		const int rayCount = *p++;
		rays.resize(rayCount);
		if (rayCount) { std::memcpy(rays.data(), p, (size_t)rayCount * sizeof(cvx_pick_ray)); }
		return p + (size_t)rayCount * (sizeof(cvx_pick_ray) / 4);
	}
};

struct CallResult {
	std::vector<cvxq_model_hit> hits;
	std::vector<cvxq_model_hit> jobs; // every job's own hit (a miss where it has none), in the list's order
};

// The specification: ray after ray, instance after instance, a voxel at a time; the nearest by the floats themselves.
static CallResult ScalarCall(const PickCall &C)
{
	CallResult out;
	const cvxb::SameInEveryLane U;
	for (const cvx_pick_ray &ray : C.rays) {
		cvxq_model_hit best = cvxb::ModelPickMiss(ray.maxT);
		for (size_t k = 0; k < C.instances.size(); k++) {
			const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(U, C.models.data(), C.instances[k]);
			cvxb::ModelPickRay R;
			cvxb::ModelPickState S;
			int64_t s[3];
			if (!cvxb::ModelPickClip(ray.origin, ray.direction, ray.maxT, B.lo, B.hi, &R, &S)) { continue; }
			cvxq_model_hit hit = cvxb::ModelPickMiss(ray.maxT);
			if (cvxb::ModelPickSequential(R, B, &S, s)) { hit = cvxb::ModelPickHitOf(B, S, s, (int)k); }
			out.jobs.push_back(hit);
			if (hit.instance >= 0 && (best.instance < 0 || hit.t < best.t)) { best = hit; }
		}
		out.hits.push_back(best);
	}
	return out;
}

// One job as a wave of cvx_model_pick.hip walks it, the lanes one after the other: false without a hit.  `key` (may be null): the ray's key so
// far, which ends the walk where the kernel's test does.
static bool WaveJob(const PickCall &C, const cvx_pick_ray &ray, int k, const uint64_t *key, cvxq_model_hit *hit)
{
	const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(cvxb::SameInEveryLane{}, C.models.data(), C.instances[k]);
	cvxb::ModelPickRay R;
	cvxb::ModelPickState start;
	if (!cvxb::ModelPickClip(ray.origin, ray.direction, ray.maxT, B.lo, B.hi, &R, &start)) { std::exit(5); } // (a job crosses its box)
	const int M = cvxb::ModelPickMajor(R);
	const int32_t startM = cvxb::ModelPickOf(M, start.v[0], start.v[1], start.v[2]);
	for (int64_t base = 0;; base += 64) {
		if (key) {
			const float enter = cvxb::ModelPickReported(base == 0 ? R.tEnter : cvxb::ModelPickLayerTime(R, M, startM, base));
			if ((uint64_t)cvxb::ModelPickFloatBits(enter) > (uint64_t)(*key >> 32) + 1u) { return false; }
		}
		for (int lane = 0; lane < 64; lane++) {
			cvxb::ModelPickState S;
			int64_t s[3];
			const int code = cvxb::ModelPickLayer(R, B, start, M, base + lane, &S, s);
			if (code == cvxb::kModelPickGo) { continue; }
			if (code == cvxb::kModelPickHit) { *hit = cvxb::ModelPickHitOf(B, S, s, k); }
			return code == cvxb::kModelPickHit; // (the lowest lane that stops decides)
		}
	}
}

// cvx_model_pick.hip's kernels with the waves run one after the other: the clip's jobs, the walk into the keys, the hits.
static CallResult WaveCall(const PickCall &C)
{
	CallResult out;
	const int n = (int)C.instances.size();
	std::vector<uint64_t> keys(C.rays.size(), cvxb::kModelPickNoKey);
	for (size_t r = 0; r < C.rays.size(); r++) {
		const cvx_pick_ray &ray = C.rays[r];
		for (int k = 0; k < n; k++) {
			cvxb::ModelPickRay R;
			cvxb::ModelPickState S;
			if (!cvxb::ModelPickClip(ray.origin, ray.direction, ray.maxT, C.instances[k].boxMin, C.instances[k].boxMax, &R, &S)) { continue; }
			cvxq_model_hit whole = cvxb::ModelPickMiss(ray.maxT), cut = whole;
			const bool found = WaveJob(C, ray, k, nullptr, &whole);
			out.jobs.push_back(whole);
			// ... and as the kernel runs it, ended by the key: what it leaves out cannot win
			const bool kept = WaveJob(C, ray, k, &keys[r], &cut);
			if (kept && (!found || std::memcmp(&cut, &whole, sizeof cut) != 0)) { std::exit(6); }
			if (found && !kept && cvxb::ModelPickKey(whole.t, k) < keys[r]) { std::exit(6); }
			if (kept) {
				const uint64_t key = cvxb::ModelPickKey(cut.t, k);
				keys[r] = key < keys[r] ? key : keys[r];
			}
		}
	}
	for (size_t r = 0; r < C.rays.size(); r++) {
		cvxq_model_hit hit = cvxb::ModelPickMiss(C.rays[r].maxT);
		if (keys[r] != cvxb::kModelPickNoKey && !WaveJob(C, C.rays[r], (int)(uint32_t)keys[r], nullptr, &hit)) { std::exit(6); }
		if (keys[r] != cvxb::kModelPickNoKey && cvxb::ModelPickKey(hit.t, hit.instance) != keys[r]) { std::exit(6); }
		out.hits.push_back(hit);
	}
	return out;
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<uint8_t> out;
	int at = 0;
	while (p < end) {
		PickCall C;
		p = C.Parse(p);
		const CallResult a = ScalarCall(C), b = WaveCall(C);
		const size_t hitsBytes = a.hits.size() * sizeof(cvxq_model_hit), jobsBytes = a.jobs.size() * sizeof(cvxq_model_hit);
		if (a.jobs.size() != b.jobs.size() || (jobsBytes && std::memcmp(a.jobs.data(), b.jobs.data(), jobsBytes) != 0)) {
			for (size_t j = 0; j < a.jobs.size() && j < b.jobs.size(); j++) {
				if (std::memcmp(&a.jobs[j], &b.jobs[j], sizeof a.jobs[j]) != 0) {
					std::fprintf(stderr, "case %d job %zu: the rule gives voxel %d %d %d face %d t %.9g, the wave voxel %d %d %d face %d t %.9g\n", at, j, a.jobs[j].voxel[0],
					             a.jobs[j].voxel[1], a.jobs[j].voxel[2], a.jobs[j].face, (double)a.jobs[j].t, b.jobs[j].voxel[0], b.jobs[j].voxel[1], b.jobs[j].voxel[2],
					             b.jobs[j].face, (double)b.jobs[j].t);
					break;
				}
			}
			std::fprintf(stderr, "case %d: the wave's jobs differ from the rule's\n", at);
			return 3;
		}
		if (hitsBytes && std::memcmp(a.hits.data(), b.hits.data(), hitsBytes) != 0) {
			std::fprintf(stderr, "case %d: the wave's hits differ from the rule's\n", at);
			return 3;
		}
		const uint8_t *h = reinterpret_cast<const uint8_t *>(a.hits.data());
		if (hitsBytes) { out.insert(out.end(), h, h + hitsBytes); }
		const int64_t jobs = (int64_t)a.jobs.size();
		const uint8_t *j = reinterpret_cast<const uint8_t *>(&jobs);
		out.insert(out.end(), j, j + sizeof jobs);
		at++;
	}
	return WriteFile(outPath, out.data(), out.size());
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
	std::vector<cvx_pick_ray> rays((size_t)CVXQ_PICK_MAX_RAYS + 1, cvx_pick_ray{ { 0.5f, 5.f, 0.5f }, { 0.f, -1.f, 0.f }, 100.f, 0.f });
	cvxq_model_hit hits[2];
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_pick_ray *r, int rayCount, cvxq_model_hit *h) {
		line(cvxq_model_pick(ctx, models, modelCount, instances, instanceCount, r, rayCount, h, nullptr));
		line(cvxq_model_pick_device(ctx, models, modelCount, instances, instanceCount, r, rayCount, h, nullptr));
	};
	std::memset(hits, 0x5A, sizeof hits);
	std::printf("%d\n", cvxq_model_pick(nullptr, &good, 1, two, 2, rays.data(), 2, hits, nullptr));
	std::printf("%d\n", cvxq_model_pick_device(nullptr, &good, 1, two, 2, rays.data(), 2, hits, nullptr));
	// cvxc_world_contacts' checks of models, instances, boxes and maps
	call(nullptr, 1, two, 2, rays.data(), 2, hits);
	call(&good, CVX_MODELS_MAX_MODELS + 1, two, 2, rays.data(), 2, hits);
	call(&good, 1, nullptr, 2, rays.data(), 2, hits);
	call(&good, 1, two, CVX_MODELS_MAX_INSTANCES + 1, rays.data(), 2, hits);
	call(&flat, 1, two, 2, rays.data(), 2, hits);
	call(&neither, 1, two, 2, rays.data(), 2, hits);
	call(&good, 1, badModel, 2, rays.data(), 2, hits);
	call(&good, 1, emptyBox, 2, rays.data(), 2, hits);
	call(&good, 1, farBox, 2, rays.data(), 2, hits);
	call(&good, 1, bigM, 2, rays.data(), 2, hits);
	call(&good, 1, bigT, 2, rays.data(), 2, hits);
	// the rays and the hits
	call(&good, 1, two, 2, nullptr, 2, hits);
	call(&good, 1, two, 2, rays.data(), 2, nullptr);
	call(&good, 1, two, 2, rays.data(), 0, hits);
	call(&good, 1, two, 2, rays.data(), -1, hits);
	call(&good, 1, two, 2, rays.data(), CVXQ_PICK_MAX_RAYS + 1, hits);
	// every error left the host array alone
	for (size_t k = 0; k < sizeof hits; k++) { if (reinterpret_cast<const uint8_t *>(hits)[k] != 0x5A) { return 1; } }
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	std::fprintf(stderr, "usage: model_pick_rules cases <in> <out> | args\n");
	return 2;
}
