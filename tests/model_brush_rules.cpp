// Host build of the model-brush rules (cpuvox_amd/csrc/cvx_model_brush.h) for tests/test_model_brush_cpu.py.  Its own main: it is also built
// stand-alone with -fsanitize=address,undefined (-DMODEL_BRUSH_RULES_NO_LIBRARY leaves `args` out: the rest calls nothing of the library, so
// nothing of it is linked).
//   model_brush_rules cases <cases in> <results out>
//     Each case, as int32 words: tests/models_rules.cpp's call (the models, the instances), strokeCount, then ten words a stroke.  The call goes
//     through cvxb::ModelBrushSequential -- a stroke at a time and a voxel at a time, a later stroke seeing what the earlier ones did -- AND
//     through the kernels' form (WaveForm below: the cull's words, the (instance, column) jobs in order, each found by the 64-probe search,
//     cvxb::ModelBrushColumn with the 64 lanes run in turn into the key array, then the (model, chunk) jobs of cvxb::ModelBrushApplyLane in
//     order, each found by the same search in the prefix of the models' chunks), each
//     on its own copy of the arrays; arrays and results must agree byte for byte (exit code 3 otherwise).  Out per case: per model its argb words
//     and its solid bytes where it has them, the model results (128 bytes each), the instance results (16 each), the summary (32).
//   model_brush_rules spans <in> <out>
//     Per entry (thirteen words: a stroke, cx, cz, dimY): cvxb::StrokeSpanUnclipped's interval against a scan of cvxb::StrokeHolds over the
//     footprint's y range and two voxels either side, and cvxb::StrokeSpan against that interval clipped to [0, dimY); exit code 3 where they
//     differ.  Out per entry, four int32 words: the unclipped interval and the clipped one.
//   model_brush_rules args
//     The argument checks of the two calls on a context without a device: per call a line "<return code> <the context's message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef MODEL_BRUSH_RULES_NO_LIBRARY
#include "cvx_context.h"
#endif
#include "cvx_model_brush.h"
#include "cvx_pair_contacts.h"
#include "rules_io.h"

struct BrushCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	std::vector<cvx_brush_stroke> strokes;
	std::vector<uint64_t> volumePrefix;

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
		}
		const int instanceCount = *p++;
		instances.resize(instanceCount);
		std::memcpy(instances.data(), p, (size_t)instanceCount * sizeof(cvx_model_instance));
		p += (size_t)instanceCount * (sizeof(cvx_model_instance) / 4);
		const int strokeCount = *p++;
		strokes.resize(strokeCount);
		std::memcpy(strokes.data(), p, (size_t)strokeCount * sizeof(cvx_brush_stroke));
		p += (size_t)strokeCount * (sizeof(cvx_brush_stroke) / 4);
		Point();
		return p;
	}
	// (after a copy too: the descriptors point into this call's own arrays)
	void Point()
	{
		volumePrefix.assign(models.size() + 1, 0u);
		for (size_t k = 0; k < models.size(); k++) {
			models[k].argb = argbWords[k].empty() ? nullptr : argbWords[k].data();
			models[k].solid = solidBytes[k].empty() ? nullptr : solidBytes[k].data();
			volumePrefix[k + 1] = volumePrefix[k] + (uint64_t)cvxb::ModelBrushVolume(models[k]);
		}
	}
};

struct BrushAnswer {
	std::vector<cvxd_model_result> models;
	std::vector<cvxd_instance_result> instances;
	cvxd_brush_summary summary;
};

static void Append(std::vector<uint8_t> *out, const void *p, size_t bytes)
{
	out->insert(out->end(), static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes);
}

// cvx_model_brush.hip's kernels with the waves run one after the other and the lanes of a wave too.  Writes C's arrays.
static bool WaveForm(BrushCall &C, BrushAnswer *out)
{
	const int modelCount = (int)C.models.size(), instanceCount = (int)C.instances.size(), strokeCount = (int)C.strokes.size();
	const int words = cvxb::ModelBrushWords(strokeCount);
	// cull: a wave per (instance, word)
	std::vector<uint64_t> lists((size_t)instanceCount * words, 0ull);
	for (int k = 0; k < instanceCount; k++) {
		for (int w = 0; w < words; w++) {
			for (int lane = 0; lane < 64; lane++) {
				if (cvxb::ModelBrushCullLane(C.strokes.data(), strokeCount, C.instances[k], 64 * w + lane)) { lists[(size_t)k * words + w] |= 1ull << lane; }
			}
		}
	}
	// mark: a wave per (instance, column) job
	std::vector<uint32_t> prefix((size_t)instanceCount + 1);
	const int64_t jobs = cvxb::ModelBrushJobs(C.instances.data(), instanceCount, C.strokes.data(), strokeCount, prefix.data());
	if (jobs < 0) { return false; }
	std::vector<uint32_t> keys((size_t)C.volumePrefix[modelCount], 0u);
	out->instances.assign((size_t)instanceCount, cvxd_instance_result{ 0, 0 });
	const cvxb::SameInEveryLane U;
	const cvxb::ModelBrushLanesInTurn lanes{};
	for (int64_t job = 0; job < jobs; job++) {
		int32_t k = 0, within = instanceCount; // the kernel's search: 64 probes a round
		while (within > 1) {
			uint64_t le = 0ull;
			for (int lane = 0; lane < 64; lane++) {
				const int32_t probe = cvxb::PairSearchProbe(k, within, lane);
				if (probe >= 0 && prefix[probe] <= (uint32_t)job) { le |= 1ull << lane; }
			}
			cvxb::PairSearchNarrow(&k, &within, le);
		}
		if (prefix[k] > (uint32_t)job || prefix[k + 1] <= (uint32_t)job) {
			std::fprintf(stderr, "job %lld: the search lands on instance %d, whose jobs are %u .. %u\n", (long long)job, k, prefix[k], prefix[k + 1]);
			return false;
		}
		const cvx_model_instance &I = C.instances[k];
		const uint32_t column = (uint32_t)job - prefix[k], sizeZ = (uint32_t)(I.boxMax[2] - I.boxMin[2]);
		uint32_t carved = 0u, painted = 0u;
		cvxb::ModelBrushColumn(U, lanes, C.models.data(), I, C.strokes.data(), lists.data() + (size_t)k * words, words, I.boxMin[0] + (int32_t)(column / sizeZ),
		                       I.boxMin[2] + (int32_t)(column % sizeZ), keys.data() + C.volumePrefix[I.model], &carved, &painted);
		out->instances[k].carved += carved;
		out->instances[k].painted += painted;
	}
	// apply: a wave per (model, chunk) job, the model found in the prefix of the models' chunks as the kernel finds it
	out->models.resize((size_t)modelCount);
	std::vector<uint32_t> chunkPrefix((size_t)modelCount + 1, 0u);
	for (int g = 0; g < modelCount; g++) {
		cvxb::ModelBrushResultInit(&out->models[g]);
		chunkPrefix[g + 1] = chunkPrefix[g] + cvxb::ModelBrushChunks(cvxb::ModelBrushVolume(C.models[g]));
	}
	for (uint32_t at = 0; at < chunkPrefix[modelCount]; at++) {
		int32_t g = 0, within = modelCount;
		while (within > 1) {
			uint64_t le = 0ull;
			for (int lane = 0; lane < 64; lane++) {
				const int32_t probe = cvxb::PairSearchProbe(g, within, lane);
				if (probe >= 0 && chunkPrefix[probe] <= at) { le |= 1ull << lane; }
			}
			cvxb::PairSearchNarrow(&g, &within, le);
		}
		if (chunkPrefix[g] > at || chunkPrefix[g + 1] <= at) {
			std::fprintf(stderr, "chunk %u: the search lands on model %d, whose chunks are %u .. %u\n", at, g, chunkPrefix[g], chunkPrefix[g + 1]);
			return false;
		}
		const uint32_t chunk = at - chunkPrefix[g];
		for (int lane = 0; lane < 64; lane++) {
			cvxb::ModelBrushSums S;
			cvxb::ModelBrushApplyLane(C.models[g], keys.data() + C.volumePrefix[g], C.strokes.data(), (uint32_t)cvxb::ModelBrushVolume(C.models[g]), chunk, lane, &S);
			cvxb::ModelBrushResultAdd(S, &out->models[g]);
		}
	}
	for (int g = 0; g < modelCount; g++) { cvxb::ModelBrushFinish(&out->models[g]); }
	out->summary = cvxb::ModelBrushSummary(out->models.data(), modelCount, jobs);
	return true;
}

// Both forms of one call, compared; the call's bytes appended to `out`.
static bool BothForms(const BrushCall &given, std::vector<uint8_t> *out)
{
	BrushCall one = given, two = given;
	one.Point();
	two.Point();
	char message[200];
	if (!cvxb::ModelBrushValidate(one.models.data(), (int)one.models.size(), one.instances.data(), (int)one.instances.size(), one.strokes.data(), (int)one.strokes.size(), message,
	                              message, sizeof message)) {
		std::fprintf(stderr, "the case is no valid call: %s\n", message);
		return false;
	}
	BrushAnswer sequential, wave;
	sequential.models.resize(one.models.size());
	sequential.instances.resize(one.instances.size());
	std::vector<uint8_t> touched((size_t)one.volumePrefix.back(), 0);
	cvxb::ModelBrushSequential(one.models.data(), (int)one.models.size(), one.instances.data(), (int)one.instances.size(), one.strokes.data(), (int)one.strokes.size(),
	                           one.volumePrefix.data(), touched.data(), sequential.models.data(), sequential.instances.data());
	if (!WaveForm(two, &wave)) { return false; }
	sequential.summary = cvxb::ModelBrushSummary(sequential.models.data(), (int)one.models.size(), wave.summary.jobs);
	for (size_t g = 0; g < one.models.size(); g++) {
		if (one.argbWords[g] != two.argbWords[g] || one.solidBytes[g] != two.solidBytes[g]) {
			std::fprintf(stderr, "model %zu: the wave form's arrays differ from the sequential rule's\n", g);
			return false;
		}
		if (std::memcmp(&sequential.models[g], &wave.models[g], sizeof(cvxd_model_result)) != 0) {
			std::fprintf(stderr, "model %zu: the wave form's result differs from the sequential rule's (voxels %lld / %lld, carved %lld / %lld, painted %lld / %lld)\n", g,
			             (long long)wave.models[g].voxels, (long long)sequential.models[g].voxels, (long long)wave.models[g].carved, (long long)sequential.models[g].carved,
			             (long long)wave.models[g].painted, (long long)sequential.models[g].painted);
			return false;
		}
	}
	for (size_t k = 0; k < one.instances.size(); k++) {
		if (std::memcmp(&sequential.instances[k], &wave.instances[k], sizeof(cvxd_instance_result)) != 0) {
			std::fprintf(stderr, "instance %zu: the wave form counts (%lld, %lld), the sequential rule (%lld, %lld)\n", k, (long long)wave.instances[k].carved,
			             (long long)wave.instances[k].painted, (long long)sequential.instances[k].carved, (long long)sequential.instances[k].painted);
			return false;
		}
	}
	if (std::memcmp(&sequential.summary, &wave.summary, sizeof(cvxd_brush_summary)) != 0) { return false; }
	for (size_t g = 0; g < two.models.size(); g++) {
		Append(out, two.argbWords[g].data(), two.argbWords[g].size() * 4);
		Append(out, two.solidBytes[g].data(), two.solidBytes[g].size());
	}
	Append(out, wave.models.data(), wave.models.size() * sizeof(cvxd_model_result));
	Append(out, wave.instances.data(), wave.instances.size() * sizeof(cvxd_instance_result));
	Append(out, &wave.summary, sizeof wave.summary);
	return true;
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<uint8_t> out;
	while (p < end) {
		BrushCall C;
		p = C.Parse(p);
		if (!BothForms(C, &out)) { return 3; }
	}
	return WriteFile(outPath, out.data(), out.size());
}

// ---- spans ----------------------------------------------------------------------------------------------------------------------------------------
static int Spans(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	std::vector<int32_t> out;
	for (size_t at = 0; at + 13 <= words.size(); at += 13) {
		cvx_brush_stroke s;
		std::memcpy(&s, words.data() + at, sizeof s);
		const int64_t cx = words[at + 10], cz = words[at + 11], dimY = words[at + 12];
		int64_t lo, hi, clippedLo, clippedHi, boxLo[3], boxHi[3];
		cvxb::StrokeFootprint(s, boxLo, boxHi);
		const bool near = cx >= boxLo[0] && cx < boxHi[0] && cz >= boxLo[2] && cz < boxHi[2]; // (cvxb::ModelBrushLaneKey's test before it forms a span)
		lo = hi = 0;
		if (near) { cvxb::StrokeSpanUnclipped(s, cx, cz, &lo, &hi); }
		int64_t first = 0, last = -1, held = 0; // the scan: the voxels of the column inside the stroke
		for (int64_t y = boxLo[1] - 2; y < boxHi[1] + 2; y++) {
			if (!cvxb::StrokeHolds(s, cx, y, cz)) { continue; }
			first = held == 0 ? y : first;
			last = y;
			held++;
		}
		const bool none = lo >= hi;
		if (none ? held != 0 : (held != hi - lo || first != lo || last != hi - 1)) {
			std::fprintf(stderr, "entry %zu: the span [%lld, %lld), the scan %lld voxels in [%lld, %lld]\n", at / 13, (long long)lo, (long long)hi, (long long)held,
			             (long long)first, (long long)last);
			return 3;
		}
		clippedLo = clippedHi = 0;
		if (near) { cvxb::StrokeSpan(s, cx, cz, dimY, &clippedLo, &clippedHi); }
		const int64_t wantLo = lo < 0 ? 0 : lo, wantHi = hi > dimY ? dimY : hi;
		if (near && (clippedLo != wantLo || clippedHi != wantHi)) {
			std::fprintf(stderr, "entry %zu: StrokeSpan [%lld, %lld), the unclipped interval clipped [%lld, %lld)\n", at / 13, (long long)clippedLo, (long long)clippedHi,
			             (long long)wantLo, (long long)wantHi);
			return 3;
		}
		out.push_back((int32_t)lo);
		out.push_back((int32_t)hi);
		out.push_back((int32_t)clippedLo);
		out.push_back((int32_t)clippedHi);
	}
	return WriteFile(outPath, out);
}

#ifndef MODEL_BRUSH_RULES_NO_LIBRARY
static int Args()
{
	cvx_context context;
	cvx_context *ctx = &context;
	uint32_t argb[16];
	uint8_t solid[16];
	std::memset(argb, 0x5A, sizeof argb);
	std::memset(solid, 0x5A, sizeof solid);
	const cvx_model good{ { 2, 2, 2 }, 0, argb, solid }, neither{ { 2, 2, 2 }, 0, nullptr, nullptr };
	const cvx_model shared[2] = { { { 2, 2, 2 }, 0, argb, nullptr }, { { 2, 2, 1 }, 0, argb + 7, nullptr } };
	const cvx_model apart[2] = { { { 2, 2, 2 }, 0, argb, nullptr }, { { 2, 2, 2 }, 0, argb + 8, solid } };
	const cvx_model crossed[2] = { { { 2, 2, 2 }, 0, nullptr, solid }, { { 2, 2, 2 }, 0, reinterpret_cast<uint32_t *>(solid + 4), nullptr } };
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
	const cvx_model_instance badModel[2] = { I, with([](cvx_model_instance &k) { k.model = 1; }) };
	const cvx_model_instance badMap[2] = { with([](cvx_model_instance &k) { k.toModel.m[2][1] = (1 << 24) + 1; }), I };
	const cvx_model_instance wideOne = with([](cvx_model_instance &k) { k.boxMin[0] = k.boxMin[2] = -(1 << 15); k.boxMax[0] = k.boxMax[2] = 1 << 15; }); // 2^32 columns
	const cvx_brush_stroke carve{ CVX_BRUSH_CARVE, CVX_SHAPE_SPHERE, { 0, 0, 0 }, { 1, 0, 0 }, 0u, 0 };
	auto stroke = [&](auto change) {
		cvx_brush_stroke s = carve;
		change(s);
		return s;
	};
	const cvx_brush_stroke fill[2] = { carve, stroke([](cvx_brush_stroke &s) { s.op = CVX_BRUSH_FILL; s.argb = 5u; }) };
	const cvx_brush_stroke black = stroke([](cvx_brush_stroke &s) { s.op = CVX_BRUSH_PAINT; });
	const cvx_brush_stroke badOp = stroke([](cvx_brush_stroke &s) { s.op = 3; }), badShape = stroke([](cvx_brush_stroke &s) { s.shape = 5; });
	const cvx_brush_stroke negative = stroke([](cvx_brush_stroke &s) { s.b[0] = -1; });
	const cvx_brush_stroke fat = stroke([](cvx_brush_stroke &s) { s.shape = CVX_SHAPE_CAPSULE; s.pad_ = 8192; });
	const cvx_brush_stroke flat = stroke([](cvx_brush_stroke &s) { s.shape = CVX_SHAPE_ELLIPSOID; s.b[0] = 3; s.b[1] = 0; s.b[2] = 3; });
	std::vector<cvx_brush_stroke> many((size_t)CVX_BRUSH_MAX_STROKES + 1, carve);
	cvxd_model_result results[2];
	cvxd_instance_result hit[2];
	cvxd_brush_summary summary;
	std::memset(results, 0x5A, sizeof results);
	std::memset(hit, 0x5A, sizeof hit);
	std::memset(&summary, 0x5A, sizeof summary);
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvx_brush_stroke *strokes, int strokeCount,
	                cvxd_model_result *r) {
		line(cvxd_models_brush(ctx, models, modelCount, instances, instanceCount, strokes, strokeCount, r, hit, &summary, nullptr));
		line(cvxd_models_brush_device(ctx, models, modelCount, instances, instanceCount, strokes, strokeCount, r, hit, &summary, nullptr));
	};
	std::printf("%d\n", cvxd_models_brush(nullptr, &good, 1, two, 2, &carve, 1, results, hit, &summary, nullptr));
	std::printf("%d\n", cvxd_models_brush_device(nullptr, &good, 1, two, 2, &carve, 1, results, hit, &summary, nullptr));
	// cvxc_world_contacts' checks of models, instances, boxes and maps (every one of them: tests/test_world_contacts_cpu.py, through the same function)
	call(nullptr, 1, two, 2, &carve, 1, results);
	call(&good, CVX_MODELS_MAX_MODELS + 1, two, 2, &carve, 1, results);
	call(&good, 1, two, CVX_MODELS_MAX_INSTANCES + 1, &carve, 1, results);
	call(&good, 1, nullptr, 2, &carve, 1, results);
	call(&neither, 1, two, 2, &carve, 1, results);
	call(&good, 1, badModel, 2, &carve, 1, results);
	call(&good, 1, emptyBox, 2, &carve, 1, results);
	call(&good, 1, badMap, 2, &carve, 1, results);
	// cvx_world_brush' checks of the strokes
	call(&good, 1, two, 2, nullptr, 1, results);
	call(&good, 1, two, 2, &carve, 0, results);
	call(&good, 1, two, 2, many.data(), CVX_BRUSH_MAX_STROKES + 1, results);
	call(&good, 1, two, 2, &badOp, 1, results);
	call(&good, 1, two, 2, &badShape, 1, results);
	call(&good, 1, two, 2, &negative, 1, results);
	call(&good, 1, two, 2, &fat, 1, results);
	call(&good, 1, two, 2, &flat, 1, results);
	// its own
	call(&good, 1, two, 2, fill, 2, results);
	call(&good, 1, two, 2, &black, 1, results);
	call(&good, 1, two, 2, &carve, 1, nullptr);
	call(shared, 2, two, 2, &carve, 1, results);
	call(crossed, 2, two, 2, &carve, 1, results);
	// too many jobs: rejected before any device call
	const cvx_brush_stroke everywhere{ CVX_BRUSH_CARVE, CVX_SHAPE_BOX, { -(1 << 20), 0, -(1 << 20) }, { 1 << 20, 1, 1 << 20 }, 0u, 0 };
	call(&good, 1, &wideOne, 1, &everywhere, 1, results);
	// every error left the host arrays alone, the models' too
	for (size_t k = 0; k < sizeof results; k++) { if (reinterpret_cast<const uint8_t *>(results)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof hit; k++) { if (reinterpret_cast<const uint8_t *>(hit)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof summary; k++) { if (reinterpret_cast<const uint8_t *>(&summary)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof argb; k++) { if (reinterpret_cast<const uint8_t *>(argb)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof solid; k++) { if (solid[k] != 0x5A) { return 1; } }
	// arrays that lie side by side do not overlap; the same strokes far away give the wide instance no job (no device here: the checks alone)
	char message[200];
	std::printf("%d\n", cvxb::ModelBrushValidate(apart, 2, two, 2, &carve, 1, results, message, sizeof message) ? 1 : 0);
	uint32_t prefix[2];
	const cvx_brush_stroke away{ CVX_BRUSH_CARVE, CVX_SHAPE_BOX, { 1 << 20, 0, 0 }, { (1 << 20) + 5, 1, 1 }, 0u, 0 };
	std::printf("%lld\n", (long long)cvxb::ModelBrushJobs(&wideOne, 1, &away, 1, prefix));
	// cvxd_model_mass
	cvxd_model_result none{};
	std::printf("%d %d\n", cvxd_model_mass(nullptr, nullptr, nullptr), cvxd_model_mass(&none, nullptr, nullptr));
	return 0;
}
#endif

int main(int argc, char **argv)
{
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "spans") == 0) { return Spans(argv[2], argv[3]); }
#ifndef MODEL_BRUSH_RULES_NO_LIBRARY
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
#endif
	std::fprintf(stderr, "usage: model_brush_rules cases <in> <out> | spans <in> <out> | args\n");
	return 2;
}
