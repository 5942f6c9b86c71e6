// Host build of the rules of cvx_world_lift_pieces (cpuvox_amd/csrc/cvx_lift.h) for tests/test_world_lift_cpu.py.
//   lift_rules sums <nodes in> <sums out>            (uint64 words)
//     Per node: px pz lo hi.  Out: cvxb::LiftNodeSums' nine words per node, then nine words more: the sums of all nodes added up as the moments
//     kernel adds them, modulo 2^64.
//   lift_rules plan <cases in> <results out>         (int64 words)
//     Per case: capacity count, then min0 min1 min2 max0 max1 max2 per piece.  Out per case: cvxb::LiftPlan's offset per piece, storedPieces,
//     storedVoxels.  Every case is planned twice, over a cvx_piece array and over a cvx_lifted_piece array (the stride): they must agree.
//   lift_rules element <cases in> <results out>      (int64 words)
//     Per case: px py pz sizeY sizeZ.  Out: cvxb::LiftElement.
//   lift_rules mass <pieces in> <results out>        (cvx_lifted_piece in, double out)
//     Out per piece: centre[3], inertia[6] of cvxb::LiftMass (what cvx_lifted_piece_mass computes behind its argument check).
//   lift_rules args
//     The argument checks of the three entry points that need no device: `code|message` per call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_lift.h"
#ifndef LIFT_RULES_NO_LIBRARY // (the sanitizer build: the rules alone, nothing of the library is linked)
#include "cvx_context.h"
#endif
#include "rules_io.h"

static int Sums(const char *in, const char *outPath)
{
	const std::vector<uint64_t> w = ReadWords<uint64_t>(in);
	std::vector<uint64_t> out;
	uint64_t total[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	for (size_t at = 0; at + 4 <= w.size(); at += 4) {
		uint64_t s[9];
		cvxb::LiftNodeSums(w[at], w[at + 1], w[at + 2], w[at + 3], s);
		for (int k = 0; k < 9; k++) {
			out.push_back(s[k]);
			total[k] += s[k];
		}
	}
	out.insert(out.end(), total, total + 9);
	return WriteFile(outPath, out);
}

static int Plan(const char *in, const char *outPath)
{
	const std::vector<int64_t> w = ReadWords<int64_t>(in);
	std::vector<int64_t> out;
	for (size_t at = 0; at + 2 <= w.size();) {
		const int64_t capacity = w[at], count = w[at + 1];
		at += 2;
		std::vector<cvx_piece> plain((size_t)count);
		std::vector<cvx_lifted_piece> lifted((size_t)count);
		for (int64_t i = 0; i < count; i++, at += 6) {
			cvx_piece p{};
			for (int a = 0; a < 3; a++) {
				p.min[a] = (int32_t)w[at + a];
				p.max[a] = (int32_t)w[at + 3 + a];
			}
			plain[(size_t)i] = p;
			lifted[(size_t)i] = cvx_lifted_piece{};
			lifted[(size_t)i].piece = p;
		}
		std::vector<int64_t> a((size_t)count + 1, 7), b((size_t)count + 1, 7); // (one word more: nothing is written behind the list)
		const cvxb::LiftStored sa = cvxb::LiftPlan(plain.data(), sizeof(cvx_piece), count, capacity, a.data());
		const cvxb::LiftStored sb = cvxb::LiftPlan(lifted.data(), sizeof(cvx_lifted_piece), count, capacity, b.data());
		if (a != b || sa.pieces != sb.pieces || sa.voxels != sb.voxels || a.back() != 7) { return 3; }
		out.insert(out.end(), a.begin(), a.end() - 1);
		out.push_back(sa.pieces);
		out.push_back(sa.voxels);
	}
	return WriteFile(outPath, out);
}

static int Element(const char *in, const char *outPath)
{
	const std::vector<int64_t> w = ReadWords<int64_t>(in);
	std::vector<int64_t> out;
	for (size_t at = 0; at + 5 <= w.size(); at += 5) { out.push_back(cvxb::LiftElement(w[at], w[at + 1], w[at + 2], w[at + 3], w[at + 4])); }
	return WriteFile(outPath, out);
}

static int Mass(const char *in, const char *outPath)
{
	const std::vector<cvx_lifted_piece> pieces = ReadWords<cvx_lifted_piece>(in);
	std::vector<double> out;
	for (const cvx_lifted_piece &p : pieces) {
		double centre[3], inertia[6];
		cvxb::LiftMass(p, centre, inertia);
		out.insert(out.end(), centre, centre + 3);
		out.insert(out.end(), inertia, inertia + 6);
	}
	return WriteFile(outPath, out);
}

#ifndef LIFT_RULES_NO_LIBRARY
static int Args()
{
	cvx_context *ctx = new cvx_context();
	const int32_t lo[3] = { 0, 0, 0 }, hi[3] = { 8, 8, 8 }, none[3] = { 4, 8, 8 };
	cvx_lifted_piece list[2];
	uint32_t argb[4];
	uint8_t solid[4];
	cvx_lift_summary summary;
	std::memset(&summary, 0x5A, sizeof summary);
	std::memset(list, 0x5A, sizeof list);
	float ms = -1.f;
	auto say = [&](int code, bool onContext) { std::printf("%d|%s\n", code, onContext ? cvx_last_error(ctx) : ""); };
	say(cvx_world_lift_pieces(nullptr, lo, hi, 0, CVX_LIFT_COPY, 0, list, 2, argb, solid, 4, &summary, &ms), false);
	say(cvx_world_lift_pieces_device(nullptr, lo, hi, 0, CVX_LIFT_COPY, 0, list, 2, argb, solid, 4, &summary, &ms), false);
	say(cvx_world_lift_pieces(ctx, nullptr, hi, 0, CVX_LIFT_COPY, 0, list, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, none, hi, 0, CVX_LIFT_COPY, 0, list, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 8, CVX_LIFT_COPY, 0, list, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, 2, 0, list, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, -1, 0, list, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, CVX_LIFT_REMOVE, 0, list, 2, argb, solid, -1, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, CVX_LIFT_REMOVE, 0, list, 2, nullptr, nullptr, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces_device(ctx, lo, hi, 0, CVX_LIFT_COPY, 0, list, 2, nullptr, nullptr, 1, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, CVX_LIFT_COPY, 6, list, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, CVX_LIFT_COPY, 0, list, -1, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, CVX_LIFT_COPY, 0, nullptr, 2, argb, solid, 4, &summary, &ms), true);
	say(cvx_world_lift_pieces(ctx, lo, hi, 0, CVX_LIFT_COPY, 0, list, 2, argb, solid, 4, &summary, &ms), true); // nothing uploaded
	// nothing was handed out
	const uint8_t *s = reinterpret_cast<const uint8_t *>(&summary), *l = reinterpret_cast<const uint8_t *>(list);
	bool untouched = ms == -1.f;
	for (size_t k = 0; k < sizeof summary; k++) { untouched = untouched && s[k] == 0x5A; }
	for (size_t k = 0; k < sizeof list; k++) { untouched = untouched && l[k] == 0x5A; }
	std::printf("%d|untouched\n", untouched ? 1 : 0);
	cvx_lifted_piece p{};
	double centre[3], inertia[6];
	say(cvx_lifted_piece_mass(nullptr, centre, inertia), false);
	say(cvx_lifted_piece_mass(&p, centre, inertia), false);
	p.piece.voxels = -3;
	say(cvx_lifted_piece_mass(&p, centre, inertia), false);
	p.piece.voxels = 1;
	say(cvx_lifted_piece_mass(&p, nullptr, nullptr), false);
	return 0;
}
#endif

int main(int argc, char **argv)
{
	if (argc == 4 && !std::strcmp(argv[1], "sums")) { return Sums(argv[2], argv[3]); }
	if (argc == 4 && !std::strcmp(argv[1], "plan")) { return Plan(argv[2], argv[3]); }
	if (argc == 4 && !std::strcmp(argv[1], "element")) { return Element(argv[2], argv[3]); }
	if (argc == 4 && !std::strcmp(argv[1], "mass")) { return Mass(argv[2], argv[3]); }
#ifndef LIFT_RULES_NO_LIBRARY
	if (argc == 2 && !std::strcmp(argv[1], "args")) { return Args(); }
#endif
	std::fprintf(stderr, "usage: lift_rules sums|plan|element|mass <in> <out> | args\n");
	return 1;
}
