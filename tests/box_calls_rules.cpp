// The refusals of the calls that take a box and read the world (tests/test_box_calls_cpu.py): which arguments they refuse, with which code and
// text, in which order, and what passes as far as "no world yet".  No device and no world: a bare context, every call ends before it needs one.
//   box_calls_rules
//     Per entry a line "# <entry>", then one line "code|message" per case, the cases in the order of Cases() below.  The snapshot diff takes no
//     box and has its own short list at the end.
//   box_calls_rules cases
//     The names of the cases, a line each, in that order.
#include <cstdio>
#include <cstring>
#include <vector>

#include "cpuvox_gpu.h"
#include "cpuvox_gpu_contacts.h"
#include "cpuvox_gpu_heights.h"
#include "cpuvox_gpu_models.h"
#include "cpuvox_gpu_snapshot.h"
#include "cpuvox_gpu_spread.h"
#include "cpuvox_gpu_surface_rects.h"
#include "cvx_context.h"

namespace {

// what a case breaks besides the box (an entry without that argument ignores it)
enum Fault { kNone, kBadFlags, kNullOutput, kNegativeCapacity, kNullList };

struct Case {
	const char *what;
	bool nullMin, nullMax;
	int32_t min[3], max[3];
	Fault fault;
};

constexpr int32_t k30 = 1 << 30;

std::vector<Case> Cases()
{
	std::vector<Case> cases;
	const Case good{ "valid, no world yet", false, false, { 0, 0, 0 }, { 8, 8, 8 }, kNone };
	auto add = [&](const char *what, auto change) {
		Case c = good;
		c.what = what;
		change(c);
		cases.push_back(c);
	};
	add("NULL boxMin", [](Case &c) { c.nullMin = true; });
	add("NULL boxMax", [](Case &c) { c.nullMax = true; });
	static const char *const equal[3] = { "min == max on axis 0", "min == max on axis 1", "min == max on axis 2" };
	static const char *const above[3] = { "min > max on axis 0", "min > max on axis 1", "min > max on axis 2" };
	for (int a = 0; a < 3; a++) {
		add(equal[a], [a](Case &c) { c.min[a] = c.max[a] = 3; });
		add(above[a], [a](Case &c) { c.min[a] = 5; c.max[a] = 4; });
	}
	add("max at 2^30", [](Case &c) { c.min[0] = k30 - 1; c.max[0] = k30; });
	add("min at -2^30", [](Case &c) { c.min[2] = -k30; c.max[2] = -k30 + 1; });
	add("max at 2^30 + 1", [](Case &c) { c.min[1] = k30; c.max[1] = k30 + 1; });
	add("min at -2^30 - 1", [](Case &c) { c.min[2] = -k30 - 1; c.max[2] = -k30; });
	auto sized = [](int x, int y, int z) {
		return [=](Case &c) {
			const int size[3] = { x, y, z };
			for (int a = 0; a < 3; a++) {
				c.min[a] = -(size[a] / 2);
				c.max[a] = c.min[a] + size[a];
			}
		};
	};
	add("2048 x 1024 x 1024", sized(2048, 1024, 1024));
	add("2047 x 1024 x 1024", sized(2047, 1024, 1024));
	add("65536 x 1 x 32768", sized(65536, 1, 32768));
	add("65535 x 1 x 32768", sized(65535, 1, 32768));
	add("negative capacity", [](Case &c) { c.fault = kNegativeCapacity; });
	add("capacity with a NULL list", [](Case &c) { c.fault = kNullList; });
	add("bad flags", [](Case &c) { c.fault = kBadFlags; });
	add("NULL output", [](Case &c) { c.fault = kNullOutput; });
	add("empty box and bad flags", [](Case &c) { c.max[1] = 0; c.fault = kBadFlags; });
	add("empty box and NULL output", [](Case &c) { c.max[1] = 0; c.fault = kNullOutput; });
	cases.push_back(good);
	return cases;
}

cvx_context *ctx;
// what the calls are handed: never written, every call ends before it has anything to hand out
uint32_t words[64];
uint8_t bytes[64];
float ms;

void Line(int code) { std::printf("%d|%s\n", code, code != CVX_OK ? cvx_last_error(ctx) : ""); }

// An entry whose box is two pointers
template <class F> void PointerBox(const char *entry, F call)
{
	std::printf("# %s\n", entry);
	for (const Case &c : Cases()) { Line(call(c.nullMin ? nullptr : c.min, c.nullMax ? nullptr : c.max, c.fault)); }
}

// An entry whose box lies in a struct: the two NULL cases fall away
template <class F> void StructBox(const char *entry, F call)
{
	std::printf("# %s\n", entry);
	for (const Case &c : Cases()) {
		if (!c.nullMin && !c.nullMax) { Line(call(c.min, c.max, c.fault)); }
	}
}

int64_t CapacityOf(Fault f) { return f == kNegativeCapacity ? -1 : 2; }
template <class T> T *ListOf(Fault f, T *list) { return f == kNullList ? nullptr : list; }

} // namespace

int main(int argc, char **)
{
	if (argc > 1) {
		for (const Case &c : Cases()) { std::printf("%s\n", c.what); }
		return 0;
	}
	ctx = new cvx_context();
	int32_t *const ints = reinterpret_cast<int32_t *>(words);

	PointerBox("cvx_world_read_voxels", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_read_voxels(ctx, mn, mx, f == kNullOutput ? nullptr : words, f == kNullOutput ? nullptr : bytes, &ms);
	});
	PointerBox("cvx_world_read_voxels_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_read_voxels_device(ctx, mn, mx, f == kNullOutput ? nullptr : words, f == kNullOutput ? nullptr : bytes, nullptr);
	});
	PointerBox("cvx_world_write_voxels", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_write_voxels(ctx, mn, mx, f == kNullOutput ? nullptr : words, bytes, f == kBadFlags ? 99 : CVX_BRUSH_FILL, 0, &ms);
	});
	PointerBox("cvx_world_write_voxels_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_write_voxels_device(ctx, mn, mx, f == kNullOutput ? nullptr : words, bytes, f == kBadFlags ? 99 : CVX_BRUSH_FILL, 0, &ms);
	});
	PointerBox("cvx_world_read_heights", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_read_heights(ctx, mn, mx, f == kNullOutput ? nullptr : ints, nullptr, nullptr, &ms);
	});
	PointerBox("cvx_world_read_heights_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_read_heights_device(ctx, mn, mx, f == kNullOutput ? nullptr : ints, nullptr, nullptr, nullptr);
	});
	PointerBox("cvx_world_write_heights", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_write_heights(ctx, mn, mx, f == kNullOutput ? nullptr : ints, words, nullptr, 0, f == kBadFlags ? 0x80 : 0, CVX_BRUSH_FILL, 0, &ms);
	});
	PointerBox("cvx_world_write_heights_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_write_heights_device(ctx, mn, mx, f == kNullOutput ? nullptr : ints, words, nullptr, 0, f == kBadFlags ? 0x80 : 0, CVX_BRUSH_FILL, 0, &ms);
	});
	PointerBox("cvx_world_distance", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_distance(ctx, mn, mx, 8, CVX_DISTANCE_TO_SOLID, f == kBadFlags ? 0x40 : 0, f == kNullOutput ? nullptr : ints, &ms);
	});
	PointerBox("cvx_world_distance_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_distance_device(ctx, mn, mx, 8, CVX_DISTANCE_TO_SOLID, f == kBadFlags ? 0x40 : 0, f == kNullOutput ? nullptr : ints, &ms);
	});

	const cvx_spread_seed seed{ { 0, 0, 0 }, 0 };
	auto spread = [&](const int32_t *mn, const int32_t *mx, Fault f) {
		cvx_spread_params p = { { mn[0], mn[1], mn[2] }, { mx[0], mx[1], mx[2] }, f == kBadFlags ? 7 : CVX_SPREAD_AIR, 0x3F, 10, 0 };
		return p;
	};
	StructBox("cvx_world_spread", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		const cvx_spread_params p = spread(mn, mx, f);
		return cvx_world_spread(ctx, &p, &seed, 1, f == kNullOutput ? nullptr : ints, nullptr, &ms);
	});
	StructBox("cvx_world_spread_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		const cvx_spread_params p = spread(mn, mx, f);
		return cvx_world_spread_device(ctx, &p, &seed, 1, f == kNullOutput ? nullptr : ints, nullptr, &ms);
	});

	cvx_surface_quad quads[2];
	cvx_surface_summary surfaceSummary;
	PointerBox("cvx_world_surface", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_surface(ctx, mn, mx, 0, f == kBadFlags ? 0x80 : 0, ListOf(f, quads), CapacityOf(f), f == kNullOutput ? nullptr : &surfaceSummary, &ms);
	});
	PointerBox("cvx_world_surface_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_surface_device(ctx, mn, mx, 0, f == kBadFlags ? 0x80 : 0, ListOf(f, quads), CapacityOf(f), f == kNullOutput ? nullptr : &surfaceSummary, &ms);
	});
	cvx_surface_rect rects[2];
	cvx_surface_rects_summary rectsSummary;
	PointerBox("cvx_world_surface_rects", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_surface_rects(ctx, mn, mx, 0, f == kBadFlags ? 0x80 : 0, ListOf(f, rects), CapacityOf(f), f == kNullOutput ? nullptr : &rectsSummary, &ms);
	});
	PointerBox("cvx_world_surface_rects_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_surface_rects_device(ctx, mn, mx, 0, f == kBadFlags ? 0x80 : 0, ListOf(f, rects), CapacityOf(f), f == kNullOutput ? nullptr : &rectsSummary, &ms);
	});

	cvx_piece pieces[2];
	cvx_pieces_summary piecesSummary;
	PointerBox("cvx_world_pieces", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		return cvx_world_pieces(ctx, mn, mx, f == kBadFlags ? 0x80 : CVX_ANCHOR_GROUND, CVX_PIECES_REPORT, 0, ListOf(f, pieces), (int)CapacityOf(f),
		                        f == kNullOutput ? nullptr : &piecesSummary, &ms);
	});
	cvx_cavities_summary cavitiesSummary;
	StructBox("cvx_world_cavities", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		cvx_cavity_params p{};
		for (int a = 0; a < 3; a++) {
			p.boxMin[a] = mn[a];
			p.boxMax[a] = mx[a];
		}
		p.openFaces = f == kBadFlags ? 0x40 : CVX_CAVITY_OPEN_DEFAULT;
		p.op = CVX_CAVITIES_REPORT;
		return cvx_world_cavities(ctx, &p, 0, ListOf(f, pieces), (int)CapacityOf(f), f == kNullOutput ? nullptr : &cavitiesSummary, &ms);
	});
	const int32_t goals[3] = { 1, 1, 1 };
	cvx_nav_summary navSummary;
	StructBox("cvx_world_nav_build", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		cvx_nav_params p{};
		for (int a = 0; a < 3; a++) {
			p.boxMin[a] = mn[a];
			p.boxMax[a] = mx[a];
		}
		p.width = f == kBadFlags ? 0 : 2;
		p.height = 3;
		p.stepUp = 1;
		p.maxDrop = 4;
		cvx_nav_field *field = nullptr;
		return cvx_world_nav_build(ctx, &p, goals, 1, f == kNullOutput ? nullptr : &field, &navSummary, &ms);
	});
	auto light = [&](const int32_t *mn, const int32_t *mx) {
		cvx_light_params p{};
		for (int a = 0; a < 3; a++) {
			p.boxMin[a] = mn[a];
			p.boxMax[a] = mx[a];
		}
		p.sunDir[1] = 1;
		p.sunLevel = 100;
		p.sunRange = 64;
		p.skyLevel = 100;
		p.skyRange = 8;
		return p;
	};
	StructBox("cvx_world_light", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		const cvx_light_params p = light(mn, mx);
		return cvx_world_light(ctx, &p, f == kBadFlags ? 9 : 0, &ms);
	});
	StructBox("cvx_world_light_lamps", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		const cvx_light_params p = light(mn, mx);
		return cvx_world_light_lamps(ctx, &p, nullptr, 0, f == kBadFlags ? 9 : 0, &ms);
	});

	// the instance box of the placed-model calls
	const cvx_model model{ { 2, 2, 2 }, 0, words, bytes };
	auto instance = [&](const int32_t *mn, const int32_t *mx) {
		cvx_model_instance I{};
		for (int a = 0; a < 3; a++) {
			I.toModel.m[a][a] = 65536;
			I.boxMin[a] = mn[a];
			I.boxMax[a] = mx[a];
		}
		return I;
	};
	cvxc_contact_result results[1];
	cvxc_contact_point points[2];
	cvxc_contacts_summary contactsSummary;
	StructBox("cvxc_world_contacts", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		const cvx_model_instance I = instance(mn, mx);
		return cvxc_world_contacts(ctx, &model, 1, &I, 1, f == kBadFlags ? 0x40 : 0, f == kNullOutput ? nullptr : results, ListOf(f, points), CapacityOf(f), &contactsSummary,
		                           &ms);
	});
	StructBox("cvxc_world_contacts_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		const cvx_model_instance I = instance(mn, mx);
		return cvxc_world_contacts_device(ctx, &model, 1, &I, 1, f == kBadFlags ? 0x40 : 0, f == kNullOutput ? nullptr : results, ListOf(f, points), CapacityOf(f),
		                                  &contactsSummary, &ms);
	});
	StructBox("cvx_world_place_models", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		cvx_model_instance I = instance(mn, mx);
		I.op = f == kBadFlags ? 99 : CVX_BRUSH_FILL;
		return cvx_world_place_models(ctx, &model, 1, &I, 1, 0, &ms);
	});
	StructBox("cvx_world_place_models_device", [&](const int32_t *mn, const int32_t *mx, Fault f) {
		cvx_model_instance I = instance(mn, mx);
		I.op = f == kBadFlags ? 99 : CVX_BRUSH_FILL;
		return cvx_world_place_models_device(ctx, &model, 1, &I, 1, 0, &ms);
	});

	// The snapshot diff: the snapshot is the library's own type, and before they fail the calls below read its first member alone, the context it
	// was taken from.
	void *snapshotWords[64] = { ctx };
	const cvx_snapshot *snap = reinterpret_cast<const cvx_snapshot *>(snapshotWords);
	cvx_snapshot_change changes[2];
	cvx_snapshot_diff_summary diffSummary;
	for (int device = 0; device < 2; device++) {
		std::printf("# %s\n", device ? "cvx_world_snapshot_diff_device" : "cvx_world_snapshot_diff");
		auto diff = [&](const cvx_snapshot *s, int flags, cvx_snapshot_change *list, int64_t capacity) {
			Line(device ? cvx_world_snapshot_diff_device(ctx, s, flags, list, capacity, &diffSummary, &ms)
			            : cvx_world_snapshot_diff(ctx, s, flags, list, capacity, &diffSummary, &ms));
		};
		diff(nullptr, 0, changes, 2);
		diff(snap, 0x80, changes, 2);
		diff(snap, 0, changes, -1);
		diff(snap, 0, nullptr, 2);
		diff(snap, 0x80, changes, -1); // the flags are named first
		diff(nullptr, 0x80, nullptr, 2); // ... and the snapshot before them
		diff(snap, 0, nullptr, 0);       // valid, no world yet
		diff(snap, CVX_SNAPSHOT_IGNORE_COLOUR, changes, 2);
	}
	return 0;
}
