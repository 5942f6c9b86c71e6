// Worlds for the host rules programs (tests/*_rules.cpp): the case-world reader, the blob-world loader and the edited-column result block.
// The file helpers of tests/rules_io.h come with it.  tests/ruleslib.py writes and reads the same formats.
//
// A CASE WORLD is a small world of gx x gz columns in the reference's layout, as int32 words:
//     dimY gx gz stride, then per column (x-major): colorsBase runCount (colorsIndex length)* colourCount colour*
// The runs are the reference's, top-down (colorsIndex < 0: air).  Every column gets its record from the edit's record rule (cvx_edit.h; a listed
// column its run-list block) and its colours at slot colorsBase + k * stride (stride 1: column after column, colorShift 2; any other: the
// blocked layout, colorShift 7).  worldMin / worldMax are those of the solid runs; a column with runs that are all air gets what the rule
// makes of it, a listed column without runs, which every rule reads like the empty record (cvxb::ArenaColumn::Count() == 0).  What follows the columns (placements, boxes, parameters,
// lamps, strokes) is the program's own.  A program that reads ONE column (brush_rules, shape_rules, stamp_rules) reads the per-column words with
// CaseColumn; readback_rules and snapshot_rules, whose cases state worldMin / worldMax themselves, use its parts.
//
// A BLOB WORLD is a LOD-0 blob uploaded into a context that never touches a device: cvx_world_upload lays the level out on the host.
//
// The EDITED-COLUMN BLOCK of a result file, as uint32 words: overLimit runCount colourCount worldMin worldMax, then (unless over the limits)
// the runs and the colours.
#pragma once

#include "cvx_context.h"
#include "cvx_copy.h"
#include "cvx_edit.h"
#include "rules_io.h"

inline int CaseColorShift(int stride) { return stride == 1 ? 2 : 7; }

// "(colorsIndex length)*" at p as a blob column's elements, [guard][runs][guard]; lowest / highest: the bounds of the solid runs (-1: none)
inline const int32_t *ReadCaseRuns(const int32_t *p, int runCount, int dimY, std::vector<uint32_t> *elements, int64_t *lowest = nullptr, int64_t *highest = nullptr)
{
	elements->assign(1, 0u);
	uint32_t start = 0;
	int64_t lo = -1, hi = -1;
	for (int r = 0; r < runCount; r++) {
		const int32_t ci = *p++, length = *p++;
		elements->push_back(((uint32_t)ci & 0xFFFFu) | ((uint32_t)length << 16));
		if (ci >= 0) {
			const int64_t top = (int64_t)dimY - start;
			if (hi < 0) { hi = top; }
			lo = top - length;
		}
		start += (uint32_t)length;
	}
	elements->push_back(0u);
	if (lowest) { *lowest = lo; }
	if (highest) { *highest = hi; }
	return p;
}

// "colourCount colour*" at p into the slots colorsBase + k * stride (the array grows as needed, with room behind the last colour)
inline const int32_t *ReadCaseColours(const int32_t *p, int colorsBase, int stride, std::vector<uint32_t> *slots)
{
	const int colourCount = *p++;
	const size_t need = (size_t)colorsBase + (size_t)stride * (colourCount + 1) + 64;
	if (slots->size() < need) { slots->resize(need, 0u); }
	for (int k = 0; k < colourCount; k++) { (*slots)[(size_t)colorsBase + (size_t)k * stride] = (uint32_t)*p++; }
	return p;
}

// The record of a column with runs (the edit's record rule); a listed column's run-list block is appended to *runs, 8 spare words behind it.
inline uint4 CaseRecord(const uint32_t header[3], const std::vector<uint32_t> &elements, int lod, int dimY, int colorsBase, std::vector<uint32_t> *runs)
{
	const cvxe::ColumnWords w = cvxe::BuildColumnWords(header, elements.data(), lod, dimY);
	uint4 rec{ w.x | (uint32_t)colorsBase, w.y, w.z, w.w };
	if (w.code == 0u) {
		const size_t entry = runs->size() / 2;
		rec.z = (uint32_t)entry;
		runs->resize(runs->size() + 2u * w.solid + 8u, 0u);
		cvxe::BuildListedRuns(header, elements.data(), lod, dimY, runs->data() + 2 * entry);
	}
	return rec;
}

// One column's words at p, "colorsBase runCount (colorsIndex length)* colourCount colour*": the colours into *slots, the record returned in *rec
inline const int32_t *ReadCaseColumn(const int32_t *p, int dimY, int stride, std::vector<uint32_t> *runs, std::vector<uint32_t> *slots, uint4 *rec)
{
	const int colorsBase = *p++, runCount = *p++;
	std::vector<uint32_t> elements;
	int64_t lowest, highest;
	p = ReadCaseRuns(p, runCount, dimY, &elements, &lowest, &highest);
	p = ReadCaseColours(p, colorsBase, stride, slots);
	const uint32_t header[3] = { 0u, (uint32_t)runCount | ((uint32_t)(lowest < 0 ? 0 : lowest) << 16), (uint32_t)(highest < 0 ? 0 : highest) };
	*rec = uint4{ 0u, 0u, 0u, 0u };
	if (runCount > 0) { *rec = CaseRecord(header, elements, 0, dimY, colorsBase, runs); }
	return p;
}

// One column on its own, with its run list and colour slots
struct CaseColumn {
	std::vector<uint32_t> runs = std::vector<uint32_t>(8, 0u), slots;
	uint4 rec{ 0u, 0u, 0u, 0u };

	const int32_t *Read(const int32_t *p, int dimY, int stride) { return ReadCaseColumn(p, dimY, stride, &runs, &slots, &rec); }
	cvxb::ArenaColumn Column() const { return cvxb::ArenaColumn{ rec.x, rec.y, rec.z, rec.w, runs.data() }; }
};

struct CaseWorld {
	std::vector<uint4> records;
	std::vector<uint32_t> runs, slots;
	int dimY = 0, gx = 0, gz = 0, stride = 0, rowShift = 0;

	// one case's world part at p; returns the cursor behind it
	const int32_t *Read(const int32_t *p)
	{
		dimY = *p++, gx = *p++, gz = *p++, stride = *p++;
		rowShift = 0;
		while ((1 << rowShift) < gz) { rowShift++; }
		records.assign((size_t)gx << rowShift, uint4{ 0u, 0u, 0u, 0u });
		runs.assign(8, 0u);
		slots.assign(64, 0u);
		for (int c = 0; c < gx * gz; c++) { p = ReadCaseColumn(p, dimY, stride, &runs, &slots, &records[((size_t)(c / gz) << rowShift) + (size_t)(c % gz)]); }
		return p;
	}

	int ColorShift() const { return CaseColorShift(stride); }

	cvxb::CopyWorld View() const
	{
		cvxb::CopyWorld W;
		W.records = reinterpret_cast<const uint32_t *>(records.data());
		W.runs = runs.data();
		W.colourSlots = slots.data();
		W.rowShift = rowShift;
		W.colorShift = ColorShift();
		W.dimX = gx;
		W.dimY = dimY;
		W.dimZ = gz;
		return W;
	}
};

// A level's blob uploaded into `ctx` on the host; a failed upload prints its message and ends the program with exit code 1.
inline void UploadBlobLevel(cvx_context *ctx, int lod, const std::vector<uint8_t> &blob, int dimX, int dimY, int dimZ, int columnCount)
{
	const int rc = cvx_world_upload(ctx, lod, blob.data(), (int64_t)blob.size(), dimX, dimY, dimZ, columnCount);
	if (rc != CVX_OK) {
		std::printf("upload failed %d: %s\n", rc, ctx->error.c_str());
		std::exit(1);
	}
}

struct BlobWorld {
	std::vector<uint8_t> blob;
	cvx_context *ctx = nullptr;
	const cvx_context::HostLevel *H = nullptr; // ctx->hostLevel[0]
	cvxb::CopyWorld W;                         // ... and its view
};

inline BlobWorld LoadBlobWorld(const char *blobPath, int dimX, int dimY, int dimZ, int columnCount)
{
	BlobWorld B;
	B.blob = ReadFile(blobPath);
	B.ctx = new cvx_context();
	UploadBlobLevel(B.ctx, 0, B.blob, dimX, dimY, dimZ, columnCount);
	B.H = &B.ctx->hostLevel[0];
	B.W.records = reinterpret_cast<const uint32_t *>(B.H->records.data());
	B.W.runs = reinterpret_cast<const uint32_t *>(B.H->runs.data());
	B.W.colourSlots = B.H->elements.data();
	B.W.rowShift = B.H->rowShift;
	B.W.colorShift = B.H->colorShift;
	B.W.dimX = dimX;
	B.W.dimY = dimY;
	B.W.dimZ = dimZ;
	return B;
}

// Appends the edited-column block of rule(outRuns, outColours) -> cvxb::BrushResult, which is run twice as the kernels run it: to count (null
// arrays), then to write.  false: the second pass counted differently (the programs return 3).
template <class Rule>
inline bool AppendEditedColumn(std::vector<uint32_t> *out, Rule rule)
{
	const cvxb::BrushResult r = rule(nullptr, nullptr);
	out->push_back(r.overLimit ? 1u : 0u);
	out->push_back(r.runCount);
	out->push_back(r.colours);
	out->push_back(r.worldMin);
	out->push_back(r.worldMax);
	if (!r.overLimit) {
		std::vector<uint32_t> newRuns(r.runCount + 1u), newColours(r.colours + 1u);
		const cvxb::BrushResult again = rule(newRuns.data(), newColours.data());
		if (again.runCount != r.runCount || again.colours != r.colours) { return false; }
		out->insert(out->end(), newRuns.begin(), newRuns.begin() + r.runCount);
		out->insert(out->end(), newColours.begin(), newColours.begin() + r.colours);
	}
	return true;
}
