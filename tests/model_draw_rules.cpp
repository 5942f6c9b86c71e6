// Host build of the model-draw rules (cpuvox_amd/csrc/cvx_model_draw.h) for tests/test_model_draw_cpu.py and tests/test_gpu_model_draw.py.  Its own
// main: it is also built stand-alone with -fsanitize=address,undefined (-DMODEL_DRAW_RULES_NO_LIBRARY leaves `args` out: the rest calls
// nothing of the library, so nothing of it is linked).
//   model_draw_rules cases <cases in> <results out>
//     Each case, as int32 words: hasWorld; with a world the case world of tests/rules_world.h and one word `repeat`; tests/models_rules.cpp's call
//     (the models, then the instances); the view (24 words: the bytes of cvxv_view); flags; hasBuffers, and with buffers the image, the depth and
//     the ids the call starts from (width * height words each; without: image 0, depth +inf, ids -1).
//     Every pixel goes through the rule with NO cull (every instance, no skip), AND the whole frame through the kernel's tile walk (the
//     rectangle per instance, the list per 8 x 8 tile 64 rectangles a step, the skip behind the key); the two must agree in every byte and
//     count (exit code 3 otherwise).  Out per case: image, depth, ids (width * height words each), then the summary (32 bytes).
//   model_draw_rules rays <cases in> <results out>
//     Each case: a view, x0 y0 w h: the rule's rays of that window (cvxb::ModelDrawRayOf), 32 bytes each.
//   model_draw_rules args
//     The argument checks of the two draw calls on a context without a device: per call a line "<return code> <the context's message>"; then
//     the checks of cvxv_view_rays and cvxv_view_from_camera.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_model_draw.h"
#include "rules_world.h"

struct DrawCall {
	bool hasWorld = false;
	CaseWorld world;
	std::vector<uint4> guarded; // the world's records with a row + 4 either side, as the arena has them
	cvxb::PickWorld W{};
	std::vector<std::vector<uint32_t>> argbWords;
	std::vector<std::vector<uint8_t>> solidBytes;
	std::vector<cvx_model> models;
	std::vector<cvx_model_instance> instances;
	cvxv_view view{};
	uint32_t flags = 0;
	std::vector<uint32_t> image;
	std::vector<float> depth;
	std::vector<int32_t> ids;

	const int32_t *Parse(const int32_t *p)
	{
		hasWorld = *p++ != 0;
		if (hasWorld) {
			p = world.Read(p);
			const size_t guard = ((size_t)1 << world.rowShift) + 4;
			guarded.assign(guard + world.records.size() + guard, uint4{ 0u, 0u, 0u, 0u });
			std::memcpy(guarded.data() + guard, world.records.data(), world.records.size() * sizeof(uint4));
			world.runs.resize(world.runs.size() + 8, 0u);
			W.records = reinterpret_cast<const uint32_t *>(guarded.data() + guard);
			W.runs = world.runs.data();
			W.colours = reinterpret_cast<const uint8_t *>(world.slots.data());
			W.rowShift = world.rowShift;
			W.colorShift = world.ColorShift();
			W.dimX = world.gx;
			W.dimY = world.dimY;
			W.dimZ = world.gz;
			W.repeat = *p++;
		}
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
		std::memcpy(&view, p, sizeof view);
		p += sizeof view / 4;
		flags = (uint32_t)*p++;
		const size_t pixels = (size_t)view.width * (size_t)view.height;
		image.assign(pixels, 0u);
		depth.assign(pixels, __builtin_inff());
		ids.assign(pixels, -1);
		if (*p++ != 0) {
			std::memcpy(image.data(), p, pixels * 4);
			std::memcpy(depth.data(), p + pixels, pixels * 4);
			std::memcpy(ids.data(), p + 2 * pixels, pixels * 4);
			p += 3 * pixels;
		}
		return p;
	}
};

struct Frame {
	std::vector<uint32_t> image;
	std::vector<float> depth;
	std::vector<int32_t> ids;
	cvxv_draw_summary summary{};
};

// A pixel's ray (step 1 with the depth test); false: a miss.
static bool PixelRay(const DrawCall &C, const std::vector<float> &depth, int x, int y, cvx_pick_ray *ray)
{
	bool live = cvxb::ModelDrawRayOf(C.view, x, y, ray);
	if ((C.flags & CVXV_DRAW_DEPTH_TEST) && live) { live = cvxb::ModelDrawDepthLimit(depth[(size_t)y * C.view.width + x], &ray->maxT); }
	return live;
}

// Steps 3 and 4 for a pixel whose bodies gave `key`.
static void Finish(const DrawCall &C, const cvx_pick_ray &ray, size_t pixel, uint64_t key, uint32_t argb, Frame *F)
{
	if (key == cvxb::kModelPickNoKey) { return; }
	const float t = cvxb::ModelDrawKeyT(key);
	if ((C.flags & CVXV_DRAW_WORLD) && cvxb::ModelDrawOccluded(C.W, ray, t)) {
		F->summary.pixelsOccluded++;
		return;
	}
	F->summary.pixelsDrawn++;
	F->image[pixel] = argb;
	F->depth[pixel] = t;
	F->ids[pixel] = (int32_t)(uint32_t)key;
}

// The specification: pixel after pixel, every instance, no cull and no skip.
static Frame RuleFrame(const DrawCall &C)
{
	Frame F{ C.image, C.depth, C.ids, {} };
	const cvxb::SameInEveryLane U;
	for (int y = 0; y < C.view.height; y++) {
		for (int x = 0; x < C.view.width; x++) {
			cvx_pick_ray ray;
			if (!PixelRay(C, C.depth, x, y, &ray)) { continue; }
			uint64_t key = cvxb::kModelPickNoKey;
			uint32_t argb = 0u;
			for (size_t k = 0; k < C.instances.size(); k++) {
				const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(U, C.models.data(), C.instances[k]);
				if (cvxb::ModelDrawBody(B, (int)k, ray, false, &key, &argb)) { F.summary.jobs++; }
			}
			Finish(C, ray, (size_t)y * C.view.width + x, key, argb, &F);
		}
	}
	return F;
}

// cvx_model_draw.hip's kernels with the waves run one after the other: the rectangles, then tile after tile the lists and the lanes' walks.
static Frame TileFrame(const DrawCall &C, const cvxb::ModelDrawCull &cull, int64_t *listed)
{
	Frame F{ C.image, C.depth, C.ids, {} };
	const cvxb::SameInEveryLane U;
	const int tile = cvxb::kModelDrawTile, n = (int)C.instances.size();
	std::vector<cvxb::ModelDrawRect> rects;
	for (const cvx_model_instance &I : C.instances) { rects.push_back(cvxb::ModelDrawRectOf(cull, C.view.origin, I.boxMin, I.boxMax, C.view.width, C.view.height)); }
	for (int ty = 0; ty < C.view.height; ty += tile) {
		for (int tx = 0; tx < C.view.width; tx += tile) {
			cvx_pick_ray rays[64];
			bool live[64];
			uint64_t keys[64];
			uint32_t argb[64] = {};
			for (int lane = 0; lane < 64; lane++) {
				const int x = tx + (lane & (tile - 1)), y = ty + lane / tile;
				live[lane] = x < C.view.width && y < C.view.height;
				live[lane] = live[lane] && PixelRay(C, C.depth, x, y, &rays[lane]);
				keys[lane] = cvxb::kModelPickNoKey;
			}
			for (int base = 0; base < n; base += 64) {
				uint64_t list = 0ull;
				for (int lane = 0; lane < 64 && base + lane < n; lane++) {
					if (cvxb::ModelDrawRectMeetsTile(rects[base + lane], tx, ty)) { list |= 1ull << lane; }
				}
				while (list != 0ull) {
					const int k = base + __builtin_ctzll(list);
					list &= list - 1ull;
					(*listed)++;
					const cvxb::ModelPickBody B = cvxb::ModelPickBodyOf(U, C.models.data(), C.instances[k]);
					for (int lane = 0; lane < 64; lane++) {
						if (live[lane] && cvxb::ModelDrawBody(B, k, rays[lane], true, &keys[lane], &argb[lane])) { F.summary.jobs++; }
					}
				}
			}
			for (int lane = 0; lane < 64; lane++) {
				if (!live[lane]) { continue; }
				const int x = tx + (lane & (tile - 1)), y = ty + lane / tile;
				Finish(C, rays[lane], (size_t)y * C.view.width + x, keys[lane], argb[lane], &F);
			}
		}
	}
	return F;
}

static void Append(std::vector<uint8_t> *out, const void *p, size_t bytes)
{
	const uint8_t *b = static_cast<const uint8_t *>(p);
	out->insert(out->end(), b, b + bytes);
}

static int Cases(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<uint8_t> out;
	int at = 0;
	while (p < end) {
		DrawCall C;
		p = C.Parse(p);
		char message[160];
		cvxb::ModelDrawCull cull;
		if (!cvxb::ModelDrawValidate(C.models.data(), (int)C.models.size(), C.instances.data(), (int)C.instances.size(), &C.view, C.flags, C.image.data(), C.depth.data(),
		                             C.ids.data(), &cull, message, sizeof message)) {
			std::fprintf(stderr, "case %d: %s\n", at, message);
			return 4;
		}
		int64_t listed = 0;
		const Frame a = RuleFrame(C), b = TileFrame(C, cull, &listed);
		const size_t pixels = a.image.size();
		for (size_t i = 0; i < pixels; i++) {
			if (a.image[i] != b.image[i] || std::memcmp(&a.depth[i], &b.depth[i], 4) != 0 || a.ids[i] != b.ids[i]) {
				std::fprintf(stderr, "case %d pixel (%zu, %zu): the rule gives id %d t %.9g argb %08x, the tiles id %d t %.9g argb %08x\n", at, i % C.view.width, i / C.view.width,
				             a.ids[i], (double)a.depth[i], a.image[i], b.ids[i], (double)b.depth[i], b.image[i]);
				return 3;
			}
		}
		if (std::memcmp(&a.summary, &b.summary, sizeof a.summary) != 0) {
			std::fprintf(stderr, "case %d: the rule counts %lld drawn %lld occluded %lld jobs, the tiles %lld %lld %lld\n", at, (long long)a.summary.pixelsDrawn,
			             (long long)a.summary.pixelsOccluded, (long long)a.summary.jobs, (long long)b.summary.pixelsDrawn, (long long)b.summary.pixelsOccluded,
			             (long long)b.summary.jobs);
			return 3;
		}
		std::printf("case %d: grow %d, %lld (tile, instance) pairs listed of %lld\n", at, cull.grow, (long long)listed,
		            (long long)C.instances.size() * (((C.view.width + 7) / 8) * (long long)((C.view.height + 7) / 8)));
		Append(&out, a.image.data(), pixels * 4);
		Append(&out, a.depth.data(), pixels * 4);
		Append(&out, a.ids.data(), pixels * 4);
		Append(&out, &a.summary, sizeof a.summary);
		at++;
	}
	return WriteFile(outPath, out.data(), out.size());
}

static int Rays(const char *in, const char *outPath)
{
	const std::vector<int32_t> words = ReadWords<int32_t>(in);
	const int32_t *p = words.data(), *end = p + words.size();
	std::vector<uint8_t> out;
	while (p < end) {
		cvxv_view view;
		std::memcpy(&view, p, sizeof view);
		p += sizeof view / 4;
		const int x0 = p[0], y0 = p[1], w = p[2], h = p[3];
		p += 4;
		for (int y = 0; y < h; y++) {
			for (int x = 0; x < w; x++) {
				cvx_pick_ray ray;
				cvxb::ModelDrawRayOf(view, x0 + x, y0 + y, &ray);
				Append(&out, &ray, sizeof ray);
			}
		}
	}
	return WriteFile(outPath, out.data(), out.size());
}

#ifndef MODEL_DRAW_RULES_NO_LIBRARY
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
	cvx_model_instance emptyBox = I;
	emptyBox.boxMax[1] = 0;
	const cvxv_view V{ { 1.f, 1.f, -10.f }, 100.f, { -0.25, -0.25, 1.0 }, { 0.125, 0.0, 0.0 }, { 0.0, 0.125, 0.0 }, 4, 4 };
	auto with = [&](auto change) {
		cvxv_view v = V;
		change(v);
		return v;
	};
	const cvxv_view wide = with([](cvxv_view &v) { v.width = CVXV_MAX_SIZE + 1; }), flat = with([](cvxv_view &v) { v.height = 0; }),
	                negative = with([](cvxv_view &v) { v.maxT = -1.f; }), nan = with([](cvxv_view &v) { v.maxT = __builtin_nanf(""); }),
	                farEye = with([](cvxv_view &v) { v.origin[2] = 3e30f; }), infinite = with([](cvxv_view &v) { v.dirX[1] = __builtin_inf(); }),
	                singular = with([](cvxv_view &v) { v.dirY[0] = 0.25, v.dirY[1] = 0.0; }), zero = with([](cvxv_view &v) { v.dir0[0] = v.dir0[1] = v.dir0[2] = 0.0; });
	uint32_t image[16];
	float depth[16];
	int32_t ids[16];
	cvxv_draw_summary summary;
	std::memset(image, 0x5A, sizeof image);
	std::memset(depth, 0x5A, sizeof depth);
	std::memset(ids, 0x5A, sizeof ids);
	std::memset(&summary, 0x5A, sizeof summary);
	auto line = [&](int code) { std::printf("%d %s\n", code, code == CVX_OK ? "" : cvx_last_error(ctx)); };
	auto call = [&](const cvx_model *models, int modelCount, const cvx_model_instance *instances, int instanceCount, const cvxv_view *view, uint32_t flags, uint32_t *im, float *de,
	                int32_t *id) {
		line(cvxv_models_draw(ctx, models, modelCount, instances, instanceCount, view, flags, im, de, id, &summary, nullptr));
		line(cvxv_models_draw_device(ctx, models, modelCount, instances, instanceCount, view, flags, im, de, id, &summary, nullptr));
	};
	std::printf("%d\n", cvxv_models_draw(nullptr, &good, 1, &I, 1, &V, 0, image, depth, ids, &summary, nullptr));
	std::printf("%d\n", cvxv_models_draw_device(nullptr, &good, 1, &I, 1, &V, 0, image, depth, ids, &summary, nullptr));
	// cvxc_world_contacts' checks of models and instances (every one of them: tests/test_model_pick_cpu.py, through the same function)
	call(nullptr, 1, &I, 1, &V, 0, image, depth, ids);
	call(&good, 1, &I, CVX_MODELS_MAX_INSTANCES + 1, &V, 0, image, depth, ids);
	call(&neither, 1, &I, 1, &V, 0, image, depth, ids);
	call(&good, 1, &emptyBox, 1, &V, 0, image, depth, ids);
	// the view
	call(&good, 1, &I, 1, nullptr, 0, image, depth, ids);
	call(&good, 1, &I, 1, &wide, 0, image, depth, ids);
	call(&good, 1, &I, 1, &flat, 0, image, depth, ids);
	call(&good, 1, &I, 1, &negative, 0, image, depth, ids);
	call(&good, 1, &I, 1, &nan, 0, image, depth, ids);
	call(&good, 1, &I, 1, &farEye, 0, image, depth, ids);
	call(&good, 1, &I, 1, &infinite, 0, image, depth, ids);
	call(&good, 1, &I, 1, &singular, 0, image, depth, ids);
	call(&good, 1, &I, 1, &zero, 0, image, depth, ids);
	// the flags and the outputs
	call(&good, 1, &I, 1, &V, 4, image, depth, ids);
	call(&good, 1, &I, 1, &V, 0, nullptr, nullptr, nullptr);
	call(&good, 1, &I, 1, &V, CVXV_DRAW_DEPTH_TEST, image, nullptr, ids);
	// the world, which this context never got
	call(&good, 1, &I, 1, &V, CVXV_DRAW_WORLD, image, depth, ids);
	// every error left the host arrays alone
	for (size_t k = 0; k < sizeof image; k++) {
		if (reinterpret_cast<const uint8_t *>(image)[k] != 0x5A || reinterpret_cast<const uint8_t *>(depth)[k] != 0x5A || reinterpret_cast<const uint8_t *>(ids)[k] != 0x5A) { return 1; }
	}
	for (size_t k = 0; k < sizeof summary; k++) { if (reinterpret_cast<const uint8_t *>(&summary)[k] != 0x5A) { return 1; } }
	// the two host calls
	cvx_pick_ray rays[16];
	cvx_camera_data camera{};
	cvxv_view made;
	std::printf("%d %d %d %d %d %d\n", cvxv_view_rays(nullptr, 0, 0, 1, 1, rays), cvxv_view_rays(&V, 0, 0, 1, 1, nullptr), cvxv_view_rays(&V, 3, 0, 2, 1, rays),
	            cvxv_view_rays(&V, 0, -1, 1, 1, rays), cvxv_view_rays(&V, 0, 0, 0, 1, rays), cvxv_view_rays(&V, 0, 0, 4, 4, rays));
	std::printf("%d %d %d %d\n", cvxv_view_from_camera(nullptr, 4, 4, 1.f, &made), cvxv_view_from_camera(&camera, 4, 4, 1.f, nullptr),
	            cvxv_view_from_camera(&camera, 0, 4, 1.f, &made), cvxv_view_from_camera(&camera, 4, 4, 1.f, &made) /* (a zero matrix) */);
	return 0;
}
#endif

int main(int argc, char **argv)
{
	if (argc == 4 && std::strcmp(argv[1], "cases") == 0) { return Cases(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "rays") == 0) { return Rays(argv[2], argv[3]); }
#ifndef MODEL_DRAW_RULES_NO_LIBRARY
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
#endif
	std::fprintf(stderr, "usage: model_draw_rules cases <in> <out> | rays <in> <out> | args\n");
	return 2;
}
