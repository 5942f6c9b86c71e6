// Host build of the sweep rules (cpuvox_amd/csrc/cvx_sweep.h) for tests/test_world_sweep_cpu.py.  Its own main: it is also built stand-alone with
// -fsanitize=address,undefined (-DSWEEP_RULES_NO_LIBRARY leaves `world` and `args` out: the rest calls nothing of the library, so nothing of it
// is linked).
//   A call, as the files hold it (int32 words): tests/contacts_rules.cpp's call (the models, the instances, solidOutside), then three words of
//   motion per instance.
//   sweep_rules cases <cases in> <results out>
//     Each case is a case world (int32 words, tests/rules_world.h), then the call.  Every instance goes through cvxb::SweepInstance, a pose at
//     a time with cvxb::ContactsInstance's own overlap, AND the whole call through the kernel's walk (WaveFirst below: the jobs in order, the
//     station, the steps of 64 lanes, lane after lane, the minimum); the two must agree (exit code 3 otherwise).  Out per case: the sweeps (48
//     bytes each), the summary (32 bytes), the contact results of the instances moved to `at` (120 bytes each), every point (24 bytes each).
//   sweep_rules path <motions in> <out>
//     Per motion (three words): n, then for j = 0 .. n the merge loop's (o_j, axis) and the closed form's (eight words), then the H + 1
//     stations (five words each: ox oz j0 dy0 dyCount).
//   sweep_rules world <blob> <dimX> <dimY> <dimZ> <columnCount> <call> <out>
//     `cases` on a LOD-0 blob uploaded into a context that never touches a device.
//   sweep_rules args
//     The argument checks of the two world calls on a context without a device or world: per call a line "<return code> <the context's message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_sweep.h"
#include "rules_world.h"

struct SweepCall {
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	std::vector<int32_t> motions;
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
		motions.assign(p, p + 3 * (size_t)instanceCount);
		return p + 3 * (size_t)instanceCount;
	}
};

static void Append(std::vector<uint8_t> *out, const void *p, size_t bytes)
{
	out->insert(out->end(), static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes);
}

// cvx_sweep.hip's kernel with the waves run one after the other and the lanes of a wave too: first[] of every instance.
static std::vector<uint32_t> WaveFirst(const cvxb::CopyWorld &W, const SweepCall &C, int64_t *jobsOut)
{
	const int n = (int)C.instances.size();
	std::vector<uint32_t> prefix((size_t)n + 1), first((size_t)n, cvxb::kSweepNone);
	std::vector<cvxb::SweepInstanceJob> info((size_t)n);
	int64_t stationCount = 0;
	const int64_t jobs = cvxb::SweepJobs(C.instances.data(), C.motions.data(), n, prefix.data(), info.data(), &stationCount);
	if (jobs < 0) { std::exit(4); }
	std::vector<cvxb::SweepStation> stations((size_t)stationCount);
	for (int k = 0; k < n; k++) { cvxb::SweepStations(C.motions.data() + 3 * (size_t)k, stations.data() + info[k].stationBase); }
	const cvxb::SameInEveryLane U;
	for (int64_t job = 0; job < jobs; job++) {
		const int k = cvxb::ContactsPairInstance(prefix.data(), n, (uint32_t)job);
		const cvx_model_instance &I = C.instances[k];
		const uint32_t sizeZ = (uint32_t)(I.boxMax[2] - I.boxMin[2]), footprint = (uint32_t)(I.boxMax[0] - I.boxMin[0]) * sizeZ;
		const uint32_t local = (uint32_t)job - prefix[k], q = local / footprint, column = local - q * footprint;
		if ((int32_t)q >= info[k].stations) { std::exit(5); }
		const cvxb::SweepStation S = stations[info[k].stationBase + q];
		const int32_t cx = I.boxMin[0] + (int32_t)(column / sizeZ), cz = I.boxMin[2] + (int32_t)(column % sizeZ);
		const cvxb::ContactsColumnJob J = cvxb::ContactsColumnJobOf(U, C.models.data(), I, cx, cz);
		const cvxb::DistanceColumn world = cvxb::DistanceColumnAt(W, (int64_t)cx + S.ox, (int64_t)cz + S.oz, C.solidOutside);
		uint32_t best = cvxb::kSweepNone;
		int32_t top, low;
		cvxb::ContactsStepRange(J, &top, &low);
		for (int32_t yTop = top; yTop >= low; yTop -= 64) {
			for (int lane = 0; lane < 64; lane++) {
				const uint32_t mine = cvxb::SweepLane(J, world, W.dimY, S, info[k].signY, yTop - lane);
				best = mine < best ? mine : best;
			}
		}
		first[k] = best < first[k] ? best : first[k];
	}
	*jobsOut = jobs;
	return first;
}

// Both forms of one call, compared; the call's bytes appended to `out`.
static bool BothForms(const cvxb::CopyWorld &W, const SweepCall &C, std::vector<uint8_t> *out)
{
	const int n = (int)C.instances.size();
	int64_t jobs = 0;
	const std::vector<uint32_t> first = WaveFirst(W, C, &jobs);
	std::vector<cvxs_sweep_result> sweeps((size_t)n);
	std::vector<cvxc_contact_result> results((size_t)n);
	std::vector<cvxc_contact_point> points;
	cvxs_sweeps_summary summary{ 0, 0, jobs, 0 };
	for (int k = 0; k < n; k++) {
		const int32_t *v = C.motions.data() + 3 * (size_t)k;
		const int32_t hit = cvxb::SweepInstance(W, C.models.data(), C.instances[k], v, C.solidOutside);
		sweeps[k] = cvxb::SweepResultOf(v, first[k]);
		if (hit != sweeps[k].hit) {
			std::fprintf(stderr, "instance %d: the wave's hit %d differs from the rule's %d\n", k, sweeps[k].hit, hit);
			return false;
		}
		// `free` and `at` by the merge loop, not the closed form SweepResultOf uses
		int32_t at[3] = { v[0], v[1], v[2] }, before[3] = { v[0], v[1], v[2] };
		int axis = -1, unused = -1;
		if (hit >= 0 && (!cvxb::SweepOffset(v, hit, at, &axis) || !cvxb::SweepOffset(v, hit > 0 ? hit - 1 : 0, before, &unused))) { return false; }
		if (std::memcmp(at, sweeps[k].at, sizeof at) != 0 || std::memcmp(before, sweeps[k].free, sizeof before) != 0 || axis != sweeps[k].axis) {
			std::fprintf(stderr, "instance %d: the closed form's offsets differ from the merge loop's\n", k);
			return false;
		}
		summary.hits += hit >= 0 ? 1 : 0;
		summary.startsSolid += hit == 0 ? 1 : 0;
		cvx_model_instance moved;
		if (!cvxb::SweepInstanceMoved(C.instances[k], sweeps[k].at, &moved)) { return false; }
		cvxb::ContactsInstance(W, C.models.data(), moved, k, C.solidOutside, &results[k], [&](const cvxc_contact_point &p) { points.push_back(p); });
		results[k].firstPoint = summary.points;
		summary.points += results[k].points;
	}
	Append(out, sweeps.data(), sweeps.size() * sizeof(cvxs_sweep_result));
	Append(out, &summary, sizeof summary);
	Append(out, results.data(), results.size() * sizeof(cvxc_contact_result));
	if (!points.empty()) { Append(out, points.data(), points.size() * sizeof(cvxc_contact_point)); }
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
		SweepCall C;
		p = C.Parse(p);
		if (!BothForms(world.View(), C, &out)) { return 3; }
	}
	return WriteFile(outPath, out.data(), out.size());
}

static int Path(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint8_t> out;
	for (; p + 3 <= end; p += 3) {
		const int32_t n = (int32_t)cvxb::SweepSteps(p);
		Append(&out, &n, 4);
		int32_t taken[3] = { 0, 0, 0 };
		int axis = -1;
		for (int32_t j = 0; j <= n; j++) {
			int32_t words[8] = { cvxb::SweepSign(p[0]) * taken[0], cvxb::SweepSign(p[1]) * taken[1], cvxb::SweepSign(p[2]) * taken[2], axis, 0, 0, 0, 0 };
			int closedAxis = -2;
			if (!cvxb::SweepOffsetClosed(p, j, words + 4, &closedAxis)) { return 3; }
			words[7] = closedAxis;
			Append(&out, words, sizeof words);
			axis = cvxb::SweepPathNext(p, taken);
		}
		if (axis != -1) { return 3; } // (the loop ends with the path)
		std::vector<cvxb::SweepStation> stations((size_t)cvxb::SweepStationCount(p));
		cvxb::SweepStations(p, stations.data());
		for (const cvxb::SweepStation &S : stations) {
			const int32_t words[5] = { S.ox, S.oz, S.j0, S.dy0, S.dyCount };
			Append(&out, words, sizeof words);
		}
	}
	return WriteFile(outPath, out.data(), out.size());
}

#ifndef SWEEP_RULES_NO_LIBRARY
static int World(char **argv)
{
	const BlobWorld blob = LoadBlobWorld(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
	const std::vector<uint8_t> callBytes = ReadFile(argv[7]);
	SweepCall C;
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
	const cvx_model_instance emptyBox = with([](cvx_model_instance &k) { k.boxMax[1] = 0; });
	const cvx_model_instance nearEdge = with([](cvx_model_instance &k) { k.boxMin[0] = (1 << 30) - 12; k.boxMax[0] = (1 << 30) - 10; });
	const cvx_model_instance nearT = with([](cvx_model_instance &k) { k.toModel.t[1] = -((int64_t)1 << 46) + 65536; });
	const cvx_model_instance wide = with([](cvx_model_instance &k) { k.boxMin[0] = k.boxMin[2] = -(1 << 14); k.boxMax[0] = k.boxMax[2] = 1 << 14; }); // 2^30 columns
	const cvx_model_instance two[2] = { I, I };
	const int32_t still[6] = { 0, 0, 0, 0, 0, 0 }, far[3] = { 0, CVXS_MAX_MOTION + 1, 0 }, farDown[6] = { 0, 0, 0, 0, 0, -CVXS_MAX_MOTION - 1 }, right[3] = { 11, 0, 0 },
	              up[3] = { 0, 2, 0 }, across[3] = { 1, 0, 1 };
	cvxs_sweep_result sweeps[2];
	cvxc_contact_result contacts[2];
	cvxc_contact_point points[2];
	cvxs_sweeps_summary summary;
	std::memset(sweeps, 0x5A, sizeof sweeps);
	std::memset(contacts, 0x5A, sizeof contacts);
	std::memset(points, 0x5A, sizeof points);
	std::memset(&summary, 0x5A, sizeof summary);
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const int32_t *motions, int solidOutside, cvxs_sweep_result *s,
	                cvxc_contact_result *c, cvxc_contact_point *p, int64_t capacity) {
		line(cvxs_world_sweep(ctx, models, modelCount, instances, instanceCount, motions, solidOutside, s, c, p, capacity, &summary, nullptr));
		line(cvxs_world_sweep_device(ctx, models, modelCount, instances, instanceCount, motions, solidOutside, s, c, p, capacity, &summary, nullptr));
	};
	std::printf("%d\n", cvxs_world_sweep(nullptr, &good, 1, &I, 1, still, 0, sweeps, contacts, points, 2, &summary, nullptr));
	std::printf("%d\n", cvxs_world_sweep_device(nullptr, &good, 1, &I, 1, still, 0, sweeps, contacts, points, 2, &summary, nullptr));
	// cvxc_world_contacts' checks (every one of them: tests/test_world_contacts_cpu.py, through the same function)
	call(nullptr, 1, &I, 1, still, 0, sweeps, contacts, points, 2);
	call(&good, 1, &I, CVX_MODELS_MAX_INSTANCES + 1, still, 0, sweeps, contacts, points, 2);
	call(&neither, 1, &I, 1, still, 0, sweeps, contacts, points, 2);
	call(&good, 1, &emptyBox, 1, still, 0, sweeps, contacts, points, 2);
	call(&good, 1, &I, 1, still, 0x40, sweeps, contacts, points, 2);
	call(&good, 1, &I, 1, still, 0, sweeps, contacts, points, -1);
	call(&good, 1, &I, 1, still, 0, sweeps, contacts, nullptr, 2);
	// its own
	call(&good, 1, &I, 1, nullptr, 0, sweeps, contacts, points, 2);
	call(&good, 1, &I, 1, still, 0, nullptr, contacts, points, 2);
	call(&good, 1, &I, 1, still, 0, sweeps, nullptr, points, 2);
	call(&good, 1, &I, 1, far, 0, sweeps, contacts, points, 2);
	call(&good, 1, two, 2, farDown, 0, sweeps, contacts, points, 2);
	call(&good, 1, &nearEdge, 1, right, 0, sweeps, contacts, points, 2);
	call(&good, 1, &nearT, 1, up, 0, sweeps, contacts, points, 2);
	// valid: no world yet (contacts may be NULL)
	call(&good, 1, &I, 1, still, 0x3F, sweeps, nullptr, nullptr, 0);
	call(&good, 1, two, 2, still, CVX_SURFACE_OUTSIDE_DEFAULT, sweeps, contacts, points, 2);
	// an 8 x 8 x 8 world of empty columns on the host side of the context: too many jobs are rejected before any device call
	std::vector<uint32_t> blob(3 * 64, 0u);
	if (cvx_world_upload(ctx, 0, blob.data(), (int64_t)blob.size() * 4, 8, 8, 8, 64) != CVX_OK) { return 1; }
	call(&good, 1, &wide, 1, across, 0, sweeps, contacts, points, 2);
	// every error left the host arrays alone
	for (size_t k = 0; k < sizeof sweeps; k++) { if (reinterpret_cast<const uint8_t *>(sweeps)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof contacts; k++) { if (reinterpret_cast<const uint8_t *>(contacts)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof points; k++) { if (reinterpret_cast<const uint8_t *>(points)[k] != 0x5A) { return 1; } }
	for (size_t k = 0; k < sizeof summary; k++) { if (reinterpret_cast<const uint8_t *>(&summary)[k] != 0x5A) { return 1; } }
	// the two host calls
	int32_t offset[3];
	int axis;
	cvx_model_instance out;
	const int32_t big[3] = { 1 << 30, 0, 0 };
	std::printf("%d %d %d %d %d %d %d\n", cvxs_sweep_offset(nullptr, 0, offset, &axis), cvxs_sweep_offset(up, 0, nullptr, &axis), cvxs_sweep_offset(up, 0, offset, nullptr),
	            cvxs_sweep_offset(far, 0, offset, &axis), cvxs_sweep_offset(up, -1, offset, &axis), cvxs_sweep_offset(up, 3, offset, &axis), cvxs_sweep_offset(up, 2, offset, &axis));
	std::printf("%d %d %d %d %d %d\n", cvxs_instance_moved(nullptr, up, &out), cvxs_instance_moved(&I, nullptr, &out), cvxs_instance_moved(&I, up, nullptr),
	            cvxs_instance_moved(&I, big, &out), cvxs_instance_moved(&nearT, up, &out), cvxs_instance_moved(&I, up, &out));
	return 0;
}
#endif

int main(int argc, char **argv)
{
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "path") == 0) { return Path(argv[2], argv[3]); }
#ifndef SWEEP_RULES_NO_LIBRARY
	if (argc == 9 && std::strcmp(argv[1], "world") == 0) { return World(argv); }
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
#endif
	std::fprintf(stderr, "usage: sweep_rules cases <in> <out> | path <in> <out> | world <blob> <dimX> <dimY> <dimZ> <columnCount> <call> <out> | args\n");
	return 2;
}
