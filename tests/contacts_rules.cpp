// Host build of the contact rules (cpuvox_amd/csrc/cvx_contacts.h) for tests/test_world_contacts_cpu.py.  Its own main: it is also built with
// -fsanitize=address,undefined as a stand-alone program.
//   A call, as the files hold it (int32 words): tests/models_rules.cpp's call (the models, then the instances), then solidOutside.
//   contacts_rules cases <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then the call.  Every instance goes through cvxb::ContactsInstance, a voxel
//     at a time, AND the whole call through the kernels' walk (WaveCall below: the pairs in order, the steps of 64 lanes, lane after lane, the
//     pair's sums added as the atomics add them, the finish); the two must agree byte for byte (exit code 3 otherwise).  Out per case: the
//     results (120 bytes each), the summary (32 bytes), every point (24 bytes each).
//   contacts_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <call> <out>
//     The same on a LOD-0 blob uploaded into a context that never touches a device.
//   contacts_rules args
//     The argument checks of the two world calls and of cvxc_contact_response on a context without a device or world: per call a line
//     "<return code> <the context's message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_contacts.h"
#include "rules_world.h"

struct ContactsCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	int solidOutside = 0;

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
		p += (size_t)instanceCount * (sizeof(cvx_model_instance) / 4);
		solidOutside = *p++;
		return p;
	}
};

struct CallResult {
	std::vector<cvxc_contact_result> results;
	std::vector<cvxc_contact_point> points;
	cvxc_contacts_summary summary{};

	void Finish() // firstPoint and the summary (cvx_contacts.hip's finish kernel; the box is already [min, max))
	{
		for (cvxc_contact_result &r : results) {
			r.firstPoint = summary.points;
			summary.touching += r.overlap > 0 ? 1 : 0;
			summary.overlap += r.overlap;
			summary.points += r.points;
			summary.voxels += r.voxels;
		}
	}
};

// The specification: instance after instance, a voxel at a time.
static CallResult ScalarCall(const cvxb::CopyWorld &W, const ContactsCall &C)
{
	CallResult out;
	out.results.resize(C.instances.size());
	for (size_t k = 0; k < C.instances.size(); k++) {
		cvxb::ContactsInstance(W, C.models.data(), C.instances[k], (int)k, C.solidOutside, &out.results[k], [&](const cvxc_contact_point &p) { out.points.push_back(p); });
	}
	out.Finish();
	return out;
}

// cvx_contacts.hip's count and write kernels with the waves run one after the other and the lanes of a wave too.
static CallResult WaveCall(const cvxb::CopyWorld &W, const ContactsCall &C)
{
	CallResult out;
	const int n = (int)C.instances.size();
	out.results.resize(n);
	std::vector<uint32_t> prefix((size_t)n + 1);
	const int64_t pairs = cvxb::ContactsPairs(C.instances.data(), n, prefix.data());
	if (pairs < 0) { std::exit(4); }
	for (int k = 0; k < n; k++) { cvxb::ContactResultInit(C.instances[k], &out.results[k]); }
	const cvxb::SameInEveryLane U;
	for (int64_t pair = 0; pair < pairs; pair++) {
		const int k = cvxb::ContactsPairInstance(prefix.data(), n, (uint32_t)pair);
		const cvx_model_instance &I = C.instances[k];
		const uint32_t sizeZ = (uint32_t)(I.boxMax[2] - I.boxMin[2]), column = (uint32_t)pair - prefix[k];
		const int32_t cx = I.boxMin[0] + (int32_t)(column / sizeZ), cz = I.boxMin[2] + (int32_t)(column % sizeZ);
		const cvxb::ContactsColumnJob J = cvxb::ContactsColumnJobOf(U, C.models.data(), I, cx, cz);
		const cvxb::DistanceColumn centre = cvxb::DistanceColumnAt(W, cx, cz, C.solidOutside);
		cvxb::ContactsColumnSums S;
		uint64_t ySum = 0u;
		int32_t top, low;
		cvxb::ContactsStepRange(J, &top, &low);
		for (int32_t yTop = top; yTop >= low; yTop -= 64) {
			uint64_t body = 0ull, solid = 0ull, points = 0ull, face[6] = { 0ull, 0ull, 0ull, 0ull, 0ull, 0ull };
			for (int lane = 0; lane < 64; lane++) {
				if (cvxb::ContactsLaneVoxel(J, yTop - lane)) { body |= 1ull << lane; }
			}
			if (body == 0ull) { continue; }
			for (int lane = 0; lane < 64; lane++) {
				if (cvxb::ContactColumnSolid(centre, W.dimY, yTop - lane)) { solid |= 1ull << lane; }
			}
			const uint64_t overlap = body & solid;
			const bool above = cvxb::ContactColumnSolid(centre, W.dimY, (int64_t)yTop + 1), below = cvxb::ContactColumnSolid(centre, W.dimY, (int64_t)yTop - 64);
			for (int lane = 0; lane < 64; lane++) {
				if (((overlap >> lane) & 1ull) == 0ull) { continue; }
				const int32_t y = yTop - lane;
				const int faces = cvxb::ContactsLaneSideFaces(W, cx, cz, C.solidOutside, y) | cvxb::ContactsLaneEndFaces(solid, above, below, lane);
				for (int f = 0; f < 6; f++) { face[f] |= (uint64_t)((faces >> f) & 1) << lane; }
				ySum += (uint64_t)(uint32_t)(y - J.yLo);
				if (faces == 0) { continue; }
				points |= 1ull << lane;
				out.points.push_back(cvxc_contact_point{ { cx, y, cz }, k, faces, cvxb::ContactColour(W, cx, y, cz) }); // (pairs and lanes in order: the scan's offsets)
			}
			cvxb::ContactsStep(S, body, overlap, points, face, yTop);
		}
		cvxb::ContactsColumnDone(S, ySum, J, &out.results[k]);
	}
	for (cvxc_contact_result &r : out.results) { cvxb::ContactResultFinish(&r); }
	out.Finish();
	return out;
}

// Both forms of one call, compared; the bytes of the scalar one appended to `out`.
static bool BothForms(const cvxb::CopyWorld &W, const ContactsCall &C, std::vector<uint8_t> *out)
{
	const CallResult a = ScalarCall(W, C), b = WaveCall(W, C);
	const size_t resultsBytes = a.results.size() * sizeof(cvxc_contact_result), pointsBytes = a.points.size() * sizeof(cvxc_contact_point);
	if (a.points.size() != b.points.size() || std::memcmp(a.results.data(), b.results.data(), resultsBytes) != 0 ||
	    (pointsBytes && std::memcmp(a.points.data(), b.points.data(), pointsBytes) != 0) || std::memcmp(&a.summary, &b.summary, sizeof a.summary) != 0) {
		std::fprintf(stderr, "the wave's results differ from the rule's\n");
		return false;
	}
	const uint8_t *r = reinterpret_cast<const uint8_t *>(a.results.data()), *s = reinterpret_cast<const uint8_t *>(&a.summary),
	              *p = reinterpret_cast<const uint8_t *>(a.points.data());
	out->insert(out->end(), r, r + resultsBytes);
	out->insert(out->end(), s, s + sizeof a.summary);
	if (pointsBytes) { out->insert(out->end(), p, p + pointsBytes); }
	return true;
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint8_t> out;
	while (p < end) {
		CaseWorld world;
		p = world.Read(p);
		ContactsCall C;
		p = C.Parse(p);
		if (!BothForms(world.View(), C, &out)) { return 3; }
	}
	return WriteFile(outPath, out.data(), out.size());
}

static int World(char **argv)
{
	const BlobWorld blob = LoadBlobWorld(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
	const std::vector<uint8_t> callBytes = ReadFile(argv[7]);
	ContactsCall C;
	C.Parse(reinterpret_cast<const int32_t *>(callBytes.data()));
	std::vector<uint8_t> out;
	if (!BothForms(blob.W, C, &out)) { return 3; }
	return WriteFile(argv[8], out.data(), out.size());
}

static int Args()
{
	cvx_context context;
	cvx_context *ctx = &context;
	uint32_t argb[8] = {};
	uint8_t solid[8] = {};
	const cvx_model good{ { 2, 2, 2 }, 0, argb, solid }, maskOnly{ { 2, 2, 2 }, 0, nullptr, solid }, neither{ { 2, 2, 2 }, 0, nullptr, nullptr };
	const cvx_model flat{ { 2, 0, 2 }, 0, argb, solid }, huge{ { 2048, 2048, 512 }, 0, argb, solid };
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
	const cvx_model_instance badModel = with([](cvx_model_instance &k) { k.model = 1; }), negativeModel = with([](cvx_model_instance &k) { k.model = -1; });
	const cvx_model_instance emptyBox = with([](cvx_model_instance &k) { k.boxMax[1] = 0; }), farBox = with([](cvx_model_instance &k) { k.boxMax[2] = (1 << 30) + 1; });
	const cvx_model_instance farBoxMin = with([](cvx_model_instance &k) { k.boxMin[0] = -(1 << 30) - 1; });
	const cvx_model_instance bigM = with([](cvx_model_instance &k) { k.toModel.m[1][2] = (1 << 24) + 1; }), bigT = with([](cvx_model_instance &k) { k.toModel.t[2] = -((int64_t)1 << 46) - 1; });
	const cvx_model_instance thirdBad[5] = { I, I, I, emptyBox, I };
	const cvx_model_instance wide = with([](cvx_model_instance &k) { k.boxMin[0] = k.boxMin[2] = -(1 << 15); k.boxMax[0] = k.boxMax[2] = 1 << 15; }); // 2^32 columns
	cvxc_contact_result results[5];
	cvxc_contact_point points[2];
	cvxc_contacts_summary summary;
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, int solidOutside, cvxc_contact_result *r,
	                cvxc_contact_point *p, int64_t capacity) {
		line(cvxc_world_contacts(ctx, models, modelCount, instances, instanceCount, solidOutside, r, p, capacity, &summary, nullptr));
		line(cvxc_world_contacts_device(ctx, models, modelCount, instances, instanceCount, solidOutside, r, p, capacity, &summary, nullptr));
	};
	std::printf("%d\n", cvxc_world_contacts(nullptr, &good, 1, &I, 1, 0, results, points, 2, &summary, nullptr));
	std::printf("%d\n", cvxc_world_contacts_device(nullptr, &good, 1, &I, 1, 0, results, points, 2, &summary, nullptr));
	call(nullptr, 1, &I, 1, 0, results, points, 2);
	call(&good, 0, &I, 1, 0, results, points, 2);
	call(&good, CVX_MODELS_MAX_MODELS + 1, &I, 1, 0, results, points, 2);
	call(&good, 1, nullptr, 1, 0, results, points, 2);
	call(&good, 1, &I, 0, 0, results, points, 2);
	call(&good, 1, &I, CVX_MODELS_MAX_INSTANCES + 1, 0, results, points, 2);
	call(&flat, 1, &I, 1, 0, results, points, 2);
	call(&huge, 1, &I, 1, 0, results, points, 2);
	call(&neither, 1, &I, 1, 0, results, points, 2);
	call(&good, 1, &badModel, 1, 0, results, points, 2);
	call(&good, 1, &negativeModel, 1, 0, results, points, 2);
	call(&good, 1, &emptyBox, 1, 0, results, points, 2);
	call(&good, 1, &farBox, 1, 0, results, points, 2);
	call(&good, 1, &farBoxMin, 1, 0, results, points, 2);
	call(&good, 1, &bigM, 1, 0, results, points, 2);
	call(&good, 1, &bigT, 1, 0, results, points, 2);
	call(&good, 1, thirdBad, 5, 0, results, points, 2);
	call(&good, 1, &I, 1, 0x40, results, points, 2);
	call(&good, 1, &I, 1, -1, results, points, 2);
	call(&good, 1, &I, 1, 0, nullptr, points, 2);
	call(&good, 1, &I, 1, 0, results, points, -1);
	call(&good, 1, &I, 1, 0, results, nullptr, 2);
	// valid: no world yet (a model without argb and an op no place takes are fine here)
	call(&good, 1, &I, 1, 0x3F, results, nullptr, 0);
	call(&maskOnly, 1, &I, 1, CVX_SURFACE_OUTSIDE_DEFAULT, results, points, 2);
	// an 8 x 8 x 8 world of empty columns on the host side of the context: too many pairs are rejected before any device call
	std::vector<uint32_t> blob(3 * 64, 0u);
	if (cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size() * 4, 8, 8, 8, 64) != CVX_OK) { return 1; }
	call(&good, 1, &wide, 1, 0, results, points, 2);
	// the helper: no context at all
	cvxc_contact_result r{};
	double centre[3], normal[3], depth;
	std::printf("%d\n", cvxc_contact_response(nullptr, centre, normal, &depth));
	std::printf("%d\n", cvxc_contact_response(&r, centre, normal, &depth));
	r.overlap = -1;
	std::printf("%d\n", cvxc_contact_response(&r, centre, normal, &depth));
	r.overlap = 2;
	std::printf("%d\n", cvxc_contact_response(&r, nullptr, nullptr, nullptr)); // valid
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 9 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	std::fprintf(stderr, "usage: contacts_rules cases <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <call> <out> | args\n");
	return 2;
}
