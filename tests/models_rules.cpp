// Host build of the model-placement rules (cpuvox_amd/csrc/cvx_models.h) for tests/test_world_models_cpu.py.  Its own main: it may also be
// built with -fsanitize=address,undefined as a stand-alone program.
//   A call, as the files hold it (int32 words): modelCount, per model sx sy sz hasArgb hasSolid, the argb words (if hasArgb) and the mask, a
//   word per voxel (if hasSolid), both in the (X, Z, Y) layout; instanceCount, per instance the 24 words of a cvx_model_instance.
//   models_rules columns <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then the call.  Every column goes through cvxb::ModelsColumn AND through
//     the kernels' walk (WaveColumn below: the cull, then the steps of cvx_dense.h with cvxb::ModelsLaneVoxel, lane after lane); the two must
//     agree word for word (exit code 3 otherwise).  Out per case and column: the edited-column block (tests/rules_world.h).
//   models_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <call> <x0> <z0> <sizeX> <sizeZ> <blob out> [dense]
//     Uploads the LOD-0 blob into a context that never touches a device, runs both walks on every column of the rectangle (count, scan, write,
//     as cvx_models.hip does) and writes the sub-world blob.  `dense`: the call is one instance with the identity map whose box is its model's;
//     cvxb::DenseColumn of the model's arrays and that box must give the same words as cvxb::ModelsColumn (exit code 4 otherwise).
//   models_rules read <blob> <dimX> <dimY> <dimZ> <columnCount> <sx> <sy> <sz> <m x 9> <t x 3> <out>
//     cvxb::ModelReadVoxel over the model in the arrays' order: the argb words, then the mask bytes.
//   models_rules args
//     The argument checks of the five calls on a context without a device or world: one return code per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_models.h"
#include "rules_world.h"

struct ModelsCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;

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
				argbWords[k].assign(reinterpret_cast<const uint32_t *>(p), reinterpret_cast<const uint32_t *>(p) + n);
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
		return p + (size_t)instanceCount * (sizeof(cvx_model_instance) / 4);
	}
};

static uint32_t Below(uint64_t mask, int lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }

// cvx_models.hip's WalkColumn with the wave's lanes run one after the other.
static cvxb::BrushResult WaveColumn(const cvxb::ArenaColumn &col, const uint32_t *slots, int colorShift, const ModelsCall &C, int cx, int cz, int dimY, uint32_t *outRuns,
                                    uint32_t *outColours)
{
	// the cull: 64 instances a pass, the kept ones appended in order
	std::vector<uint16_t> list;
	int64_t lo = INT64_MAX, hi = INT64_MIN;
	for (size_t base = 0; base < C.instances.size(); base += 64) {
		for (size_t s = base; s < base + 64 && s < C.instances.size(); s++) {
			cvxb::ModelCullBox b;
			if (!cvxb::ModelCullBoxOf(C.instances[s], (int64_t)1 << 30, dimY, (int64_t)1 << 30, &b) || !cvxb::ModelCullCovers(b, cx, cz)) { continue; }
			list.push_back((uint16_t)s);
			lo = b.y0 < lo ? b.y0 : lo;
			hi = b.y1 > hi ? b.y1 : hi;
		}
	}
	if (list.empty()) { lo = hi = 0; }
	const uint32_t count = col.Count();
	uint32_t cursor = 0u;
	cvxb::DenseWalk w;
	for (int yTop = dimY - 1; yTop >= 0; yTop -= 64) {
		const int air = cvxb::DenseAirSteps(col, count, &cursor, lo, hi, yTop);
		if (air > 0) {
			const int voxels = air * 64 < yTop + 1 ? air * 64 : yTop + 1;
			cvxb::DenseAdvanceAir(w, (uint32_t)voxels, outRuns);
			yTop -= (air - 1) * 64;
			continue;
		}
		const uint32_t valid = (uint32_t)(yTop + 1 < 64 ? yTop + 1 : 64);
		cvxb::Voxel v[64];
		uint64_t mask = 0;
		for (int lane = 0; lane < 64; lane++) {
			v[lane] = cvxb::ModelsLaneVoxel(cvxb::SameInEveryLane{}, col, slots, colorShift, C.models.data(), C.instances.data(), list.data(), (int)list.size(), cx, cz, yTop,
			                                yTop - lane);
			if (v[lane].solid) { mask |= 1ull << lane; }
		}
		const uint64_t starts = cvxb::DenseStarts(w, mask, valid);
		if (outRuns) {
			for (int lane = 0; lane < 64; lane++) {
				cvxb::DenseLaneRun(w, mask, starts, lane, Below(starts, lane), Below(mask, lane), outRuns);
				if (v[lane].solid) { outColours[w.colours + Below(mask, lane)] = v[lane].argb; }
			}
		}
		cvxb::DenseAdvance(w, mask, starts, valid, yTop, outRuns);
	}
	return cvxb::DenseFinish(w, outRuns);
}

static bool Same(const cvxb::BrushResult &a, const cvxb::BrushResult &b)
{
	return a.runCount == b.runCount && a.colours == b.colours && a.worldMin == b.worldMin && a.worldMax == b.worldMax && a.overLimit == b.overLimit;
}

static cvxb::BrushResult Rule(const cvxb::ArenaColumn &col, const uint32_t *slots, int colorShift, const ModelsCall &C, int cx, int cz, int dimY, uint32_t *runs, uint32_t *colours)
{
	return cvxb::ModelsColumn(col, slots, colorShift, C.models.data(), C.instances.data(), nullptr, (int)C.instances.size(), cx, cz, dimY, runs, colours);
}

// Both walks of one column; false: they disagree.  The runs and colours are the scalar rule's.
static bool BothWalks(const cvxb::ArenaColumn &col, const uint32_t *slots, int colorShift, const ModelsCall &C, int cx, int cz, int dimY, cvxb::BrushResult *result,
                      std::vector<uint32_t> *runs, std::vector<uint32_t> *colours)
{
	const cvxb::BrushResult r = Rule(col, slots, colorShift, C, cx, cz, dimY, nullptr, nullptr);
	const cvxb::BrushResult counted = WaveColumn(col, slots, colorShift, C, cx, cz, dimY, nullptr, nullptr);
	*result = r;
	runs->assign(r.runCount + 1u, 0xDEADBEEFu);
	colours->assign(r.colours + 1u, 0xDEADBEEFu);
	if (!Same(r, counted)) { std::fprintf(stderr, "column (%d, %d): the wave's count differs from the rule's\n", cx, cz); return false; }
	if (r.overLimit || r.runCount == 0u) { return true; } // (an empty column is not walked again: the kernel writes its zero header and leaves)
	std::vector<uint32_t> waveRuns(*runs), waveColours(*colours);
	const cvxb::BrushResult again = Rule(col, slots, colorShift, C, cx, cz, dimY, runs->data(), colours->data());
	const cvxb::BrushResult written = WaveColumn(col, slots, colorShift, C, cx, cz, dimY, waveRuns.data(), waveColours.data());
	if (!Same(r, again) || !Same(r, written) || waveRuns != *runs || waveColours != *colours || runs->back() != 0xDEADBEEFu || colours->back() != 0xDEADBEEFu) {
		std::fprintf(stderr, "column (%d, %d): the wave's runs or colours differ from the rule's\n", cx, cz);
		return false;
	}
	return true;
}

static int Columns(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		CaseWorld world;
		p = world.Read(p);
		const int dimY = world.dimY, gx = world.gx, gz = world.gz;
		ModelsCall C;
		p = C.Parse(p);
		const cvxb::CopyWorld W = world.View();
		for (int c = 0; c < gx * gz; c++) {
			const int cx = c / gz, cz = c % gz;
			cvxb::BrushResult r;
			std::vector<uint32_t> newRuns, newColours;
			if (!BothWalks(cvxb::CopyColumnAt(W, cx, cz), W.colourSlots, W.colorShift, C, cx, cz, dimY, &r, &newRuns, &newColours)) { return 3; }
			out.push_back(r.overLimit ? 1u : 0u);
			out.push_back(r.runCount);
			out.push_back(r.colours);
			out.push_back(r.worldMin);
			out.push_back(r.worldMax);
			if (!r.overLimit) {
				out.insert(out.end(), newRuns.begin(), newRuns.begin() + r.runCount);
				out.insert(out.end(), newColours.begin(), newColours.begin() + r.colours);
			}
		}
	}
	return WriteFile(outPath, out.data(), out.size() * 4);
}

static BlobWorld Upload(char **argv) { return LoadBlobWorld(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])); }

static int World(char **argv, bool dense)
{
	const BlobWorld blob = Upload(argv);
	const cvx_context::HostLevel &H = *blob.H;
	const cvxb::CopyWorld &W = blob.W;
	const std::vector<uint8_t> callBytes = ReadFile(argv[7]);
	ModelsCall C;
	C.Parse(reinterpret_cast<const int32_t *>(callBytes.data()));
	const int x0 = std::atoi(argv[8]), z0 = std::atoi(argv[9]), sizeX = std::atoi(argv[10]), sizeZ = std::atoi(argv[11]);
	cvxb::DenseBox box{};
	if (dense) {
		if (C.instances.size() != 1) { return 2; }
		for (int a = 0; a < 3; a++) {
			box.min[a] = C.instances[0].boxMin[a];
			box.size[a] = C.models[C.instances[0].model].size[a];
			if (C.instances[0].boxMax[a] - C.instances[0].boxMin[a] != box.size[a]) { return 2; }
		}
	}
	// count, scan, write: what models_count_kernel, cvxi::ExclusiveScan and models_write_kernel do
	const int columns = sizeX * sizeZ;
	std::vector<uint32_t> headers(3 * (size_t)columns, 0u), pool;
	int over = 0;
	for (int i = 0; i < columns; i++) {
		const int cx = x0 + i / sizeZ, cz = z0 + i % sizeZ;
		const cvxb::ArenaColumn col = cvxb::CopyColumnAt(W, cx, cz);
		cvxb::BrushResult r;
		std::vector<uint32_t> runs, colours;
		if (!BothWalks(col, W.colourSlots, W.colorShift, C, cx, cz, W.dimY, &r, &runs, &colours)) { return 3; }
		if (dense) {
			const cvx_model &M = C.models[C.instances[0].model];
			std::vector<uint32_t> denseRuns(runs.size(), 0xDEADBEEFu), denseColours(colours.size(), 0xDEADBEEFu);
			const bool emit = !r.overLimit && r.runCount != 0u;
			const cvxb::BrushResult d = cvxb::DenseColumn(col, W.colourSlots, W.colorShift, box, M.argb, M.solid, C.instances[0].op, cx, cz, W.dimY,
			                                              emit ? denseRuns.data() : nullptr, emit ? denseColours.data() : nullptr);
			if (!Same(r, d) || (emit && (denseRuns != runs || denseColours != colours))) {
				std::fprintf(stderr, "column (%d, %d): cvxb::DenseColumn differs from cvxb::ModelsColumn at the identity\n", cx, cz);
				return 4;
			}
		}
		over |= r.overLimit ? 1 : 0;
		if (r.runCount == 0u || r.overLimit) { continue; }
		const size_t off = pool.size();
		pool.resize(off + r.runCount + 2u + r.colours, 0u);
		WaveColumn(col, W.colourSlots, W.colorShift, C, cx, cz, W.dimY, pool.data() + off + 1, pool.data() + off + r.runCount + 2u);
		headers[3 * (size_t)i] = (uint32_t)off;
		headers[3 * (size_t)i + 1] = r.runCount | (r.worldMin << 16);
		headers[3 * (size_t)i + 2] = r.worldMax;
	}
	headers.insert(headers.end(), pool.begin(), pool.end());
	std::printf("colorShift %d listed %lld over %d\n", H.colorShift, (long long)H.listedColumns, over);
	return WriteFile(argv[12], headers.data(), headers.size() * 4);
}

static int Read(char **argv)
{
	const BlobWorld blob = Upload(argv);
	const cvxb::CopyWorld &W = blob.W;
	int64_t size[3];
	for (int a = 0; a < 3; a++) { size[a] = std::atoll(argv[7 + a]); }
	cvx_model_map M{};
	for (int k = 0; k < 9; k++) { M.m[k / 3][k % 3] = (int32_t)std::atoll(argv[10 + k]); }
	for (int k = 0; k < 3; k++) { M.t[k] = std::atoll(argv[19 + k]); }
	const size_t n = (size_t)(size[0] * size[1] * size[2]);
	std::vector<uint8_t> out(n * 5);
	uint32_t *argb = reinterpret_cast<uint32_t *>(out.data());
	uint8_t *solid = out.data() + n * 4;
	for (int64_t x = 0; x < size[0]; x++) {
		for (int64_t z = 0; z < size[2]; z++) {
			for (int64_t y = 0; y < size[1]; y++) {
				const cvxb::Voxel v = cvxb::ModelReadVoxel(W, M, x, y, z);
				const size_t i = (size_t)((x * size[2] + z) * size[1] + y);
				argb[i] = v.argb;
				solid[i] = v.solid ? 1 : 0;
			}
		}
	}
	return WriteFile(argv[22], out.data(), out.size());
}

static int Args()
{
	cvx_context context;
	cvx_context *ctx = &context;
	uint32_t argb[8] = {};
	uint8_t solid[8] = {};
	const cvx_model good{ { 2, 2, 2 }, 0, argb, solid }, maskOnly{ { 2, 2, 2 }, 0, nullptr, solid }, neither{ { 2, 2, 2 }, 0, nullptr, nullptr };
	const cvx_model flat{ { 2, 0, 2 }, 0, argb, solid }, huge{ { 2048, 2048, 512 }, 0, argb, solid };
	const cvx_model pair[2] = { good, maskOnly };
	cvx_model_instance I{};
	for (int a = 0; a < 3; a++) {
		I.toModel.m[a][a] = 65536;
		I.boxMax[a] = 2;
	}
	I.op = CVX_COPY_REPLACE;
	auto with = [&](auto change) {
		cvx_model_instance k = I;
		change(k);
		return k;
	};
	const cvx_model_instance badModel = with([](cvx_model_instance &k) { k.model = 1; }), negativeModel = with([](cvx_model_instance &k) { k.model = -1; });
	const cvx_model_instance badOp = with([](cvx_model_instance &k) { k.op = 4; }), negativeOp = with([](cvx_model_instance &k) { k.op = -1; });
	const cvx_model_instance emptyBox = with([](cvx_model_instance &k) { k.boxMax[1] = 0; }), farBox = with([](cvx_model_instance &k) { k.boxMax[2] = (1 << 30) + 1; });
	const cvx_model_instance farBoxMin = with([](cvx_model_instance &k) { k.boxMin[0] = -(1 << 30) - 1; });
	const cvx_model_instance bigM = with([](cvx_model_instance &k) { k.toModel.m[1][2] = (1 << 24) + 1; }), bigT = with([](cvx_model_instance &k) { k.toModel.t[2] = -((int64_t)1 << 46) - 1; });
	const cvx_model_instance paintsMaskOnly = with([](cvx_model_instance &k) { k.model = 1; k.op = CVX_BRUSH_PAINT; });
	const cvx_model_instance carvesMaskOnly = with([](cvx_model_instance &k) { k.model = 1; k.op = CVX_BRUSH_CARVE; });
	const cvx_model_instance thirdBad[5] = { I, I, I, badOp, I };
	const int32_t size[3] = { 2, 2, 2 }, flatSize[3] = { 2, 0, 2 }, hugeSize[3] = { 2048, 2048, 512 };
	cvx_model_map bigMap = I.toModel, farMap = I.toModel;
	bigMap.m[0][0] = -(1 << 24) - 1;
	farMap.t[0] = ((int64_t)1 << 46) + 1;
	const double identity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }, singular[12] = { 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0 };
	double notFinite[12], tiny[12], far[12];
	std::memcpy(notFinite, identity, sizeof identity);
	std::memcpy(tiny, identity, sizeof identity);
	std::memcpy(far, identity, sizeof identity);
	notFinite[5] = __builtin_nan("");
	tiny[0] = 1.0 / 1024.0; // the inverse's 1024 is beyond |m| <= 256
	far[3] = 3e9;           // the translation is beyond 2^30
	cvx_model_instance made{};
	const int codes[] = {
		// place
		cvx_world_place_models(nullptr, &good, 1, &I, 1, 0, nullptr),
		cvx_world_place_models(ctx, nullptr, 1, &I, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 0, &I, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, CVX_MODELS_MAX_MODELS + 1, &I, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 1, nullptr, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &I, 0, 0, nullptr), cvx_world_place_models(ctx, &good, 1, &I, CVX_MODELS_MAX_INSTANCES + 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &I, 1, 6, nullptr), cvx_world_place_models(ctx, &good, 1, &I, 1, -1, nullptr),
		cvx_world_place_models(ctx, &flat, 1, &I, 1, 0, nullptr), cvx_world_place_models(ctx, &huge, 1, &I, 1, 0, nullptr),
		cvx_world_place_models(ctx, &neither, 1, &I, 1, 0, nullptr), cvx_world_place_models(ctx, pair, 2, &paintsMaskOnly, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &badModel, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 1, &negativeModel, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &badOp, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 1, &negativeOp, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &emptyBox, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 1, &farBox, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &farBoxMin, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 1, &bigM, 1, 0, nullptr),
		cvx_world_place_models(ctx, &good, 1, &bigT, 1, 0, nullptr), cvx_world_place_models(ctx, &good, 1, thirdBad, 5, 0, nullptr),
		cvx_world_place_models_device(ctx, &neither, 1, &I, 1, 0, nullptr), cvx_world_place_models_device(ctx, &good, 1, &badOp, 1, 0, nullptr),
		// read
		cvx_world_read_model(nullptr, size, &I.toModel, argb, solid, nullptr),
		cvx_world_read_model(ctx, nullptr, &I.toModel, argb, solid, nullptr), cvx_world_read_model(ctx, size, nullptr, argb, solid, nullptr),
		cvx_world_read_model(ctx, flatSize, &I.toModel, argb, solid, nullptr), cvx_world_read_model(ctx, hugeSize, &I.toModel, argb, solid, nullptr),
		cvx_world_read_model(ctx, size, &bigMap, argb, solid, nullptr), cvx_world_read_model(ctx, size, &farMap, argb, solid, nullptr),
		cvx_world_read_model(ctx, size, &I.toModel, nullptr, nullptr, nullptr), cvx_world_read_model_device(ctx, size, &I.toModel, nullptr, nullptr, nullptr),
		cvx_world_read_model_device(ctx, flatSize, &I.toModel, argb, solid, nullptr),
		// the helper
		cvx_model_instance_from_matrix(nullptr, size, 0, 0, &made), cvx_model_instance_from_matrix(identity, nullptr, 0, 0, &made),
		cvx_model_instance_from_matrix(identity, size, 0, 0, nullptr), cvx_model_instance_from_matrix(notFinite, size, 0, 0, &made),
		cvx_model_instance_from_matrix(singular, size, 0, 0, &made), cvx_model_instance_from_matrix(tiny, size, 0, 0, &made),
		cvx_model_instance_from_matrix(far, size, 0, 0, &made),
		// valid: no world yet
		cvx_world_place_models(ctx, &good, 1, &I, 1, 5, nullptr), cvx_world_place_models(ctx, pair, 2, &carvesMaskOnly, 1, 0, nullptr),
		cvx_world_place_models_device(ctx, &good, 1, &I, 1, 3, nullptr), cvx_world_read_model(ctx, size, &I.toModel, argb, nullptr, nullptr),
		cvx_world_read_model_device(ctx, size, &I.toModel, nullptr, solid, nullptr),
		// valid, no context needed
		cvx_model_instance_from_matrix(identity, size, 0, CVX_BRUSH_FILL, &made),
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "columns") == 0) { return Columns(argv[2], argv[3]); }
	if (argc == 13 && std::strcmp(argv[1], "world") == 0) { return World(argv, false); }
	if (argc == 14 && std::strcmp(argv[1], "world") == 0 && std::strcmp(argv[13], "dense") == 0) { return World(argv, true); }
	if (argc == 23 && std::strcmp(argv[1], "read") == 0) { return Read(argv); }
	std::fprintf(stderr, "usage: models_rules columns <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <call> <x0> <z0> <sizeX> <sizeZ> <out> [dense] | "
	                     "read <blob> <dimX> <dimY> <dimZ> <columnCount> <size x y z> <m x 9> <t x 3> <out> | args\n");
	return 2;
}
