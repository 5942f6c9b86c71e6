// Host build of the stamp rules (cpuvox_amd/csrc/cvx_stamp.h) for tests/test_world_stamp_cpu.py, tests/test_gpu_world_stamp.py and
// tests/test_gpu_world_stamp_limits.py.
//   stamp_rules voxelise <mesh in> <voxels out>
//     mesh: int32 dimX dimY dimZ vertexCount indexCount materialCount, the cvx_mesh_vertex array, the int32 indices, then per material int32 width
//     height (width 0: no texture) and width * height * 4 texel bytes.  Every triangle through cvxs::VoxelizeTriangle in order; out: int32
//     (x, y, z, argb) per emitted voxel, in emission order.
//   stamp_rules counts <mesh in> <counts out>
//     What the device's pipeline (cvx_stamp.hip) makes of every triangle, from TriangleSetup / TriangleHit / TriangleColour in VoxelizeTriangle's
//     loop order: int32 box columns (the device's pairs; 0 without area), hits, kept hits (capped at cvxs::kVoxelizeBufferMax), opaque kept
//     hits, the most hits in one column, and 1 when the cap falls strictly inside a column (rank < cap < rank + hits).
//   stamp_rules hits <mesh in> <hits out>
//     The same loop: int32 (triangle, x, y, z) per hit, the hits past the cap and the transparent ones included.
//   stamp_rules stamp <cases in> <results out>
//     Each case is one column plus stamped voxels (int32 words): dimY stride, the column's words (tests/rules_world.h), op voxelCount
//     (y argb)*.  The voxels (any order, duplicates allowed) are sorted top-down and merged with cvxs::MergeStamped, then cvxs::StampColumn.
//     Out per case: the edited-column block (tests/rules_world.h).
//   stamp_rules args
//     The argument checks of cvx_world_stamp_mesh on a context that never touched a device (no world): one return code per call.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvx_stamp.h"
#include "rules_world.h"

// the mesh file of the voxelise / counts / hits modes
struct MeshFile {
	int dimX, dimY, dimZ, indexCount, materialCount;
	std::vector<cvx_mesh_vertex> vertices;
	std::vector<int32_t> indices;
	std::vector<cvxs::Texture> textures;
	std::vector<uint8_t> texels;
	const cvx_mesh_vertex &Corner(int t, int k) const { return vertices[(size_t)indices[(size_t)t + (size_t)k]]; }
};

static MeshFile ReadMesh(const char *in)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const uint8_t *p = bytes.data();
	int32_t head[6];
	std::memcpy(head, p, sizeof head);
	p += sizeof head;
	MeshFile m{ head[0], head[1], head[2], head[4], head[5], {}, {}, {}, {} };
	m.vertices.resize((size_t)head[3]);
	std::memcpy(m.vertices.data(), p, m.vertices.size() * sizeof(cvx_mesh_vertex));
	p += m.vertices.size() * sizeof(cvx_mesh_vertex);
	m.indices.resize((size_t)m.indexCount);
	std::memcpy(m.indices.data(), p, m.indices.size() * 4);
	p += m.indices.size() * 4;
	for (int k = 0; k < m.materialCount; k++) {
		int32_t wh[2];
		std::memcpy(wh, p, sizeof wh);
		p += sizeof wh;
		if (wh[0] == 0) {
			m.textures.push_back(cvxs::Texture{ 0, 0, -1 });
			continue;
		}
		m.textures.push_back(cvxs::Texture{ wh[0], wh[1], (int64_t)m.texels.size() });
		m.texels.insert(m.texels.end(), p, p + (size_t)wh[0] * wh[1] * 4);
		p += (size_t)wh[0] * wh[1] * 4;
	}
	return m;
}

static int Voxelise(const char *in, const char *outPath)
{
	const MeshFile m = ReadMesh(in);
	std::vector<uint32_t> out;
	for (int t = 0; t + 2 < m.indexCount; t += 3) {
		cvxs::VoxelizeTriangle(m.Corner(t, 0), m.Corner(t, 1), m.Corner(t, 2), m.dimX, m.dimY, m.dimZ, m.textures.data(), m.materialCount, m.texels.data(),
		                       [&](int x, int y, int z, uint32_t argb) {
			                       out.push_back((uint32_t)x);
			                       out.push_back((uint32_t)y);
			                       out.push_back((uint32_t)z);
			                       out.push_back(argb);
		                       });
	}
	return WriteFile(outPath, out);
}

// VoxelizeTriangle's loop (cvx_stamp.h) without its cap, counted per triangle; with allHits, every hit as (triangle, x, y, z) instead
static int Counts(const char *in, const char *outPath, bool allHits)
{
	const MeshFile m = ReadMesh(in);
	const uint32_t cap = (uint32_t)cvxs::kVoxelizeBufferMax;
	std::vector<uint32_t> out;
	for (int t = 0; t + 2 < m.indexCount; t += 3) {
		const cvx_mesh_vertex &v0 = m.Corner(t, 0), &v1 = m.Corner(t, 1), &v2 = m.Corner(t, 2);
		uint32_t columns = 0, hits = 0, opaque = 0, most = 0, inside = 0;
		cvxs::TriSetup s;
		if (cvxs::TriangleSetup(v0, v1, v2, m.dimX, m.dimY, m.dimZ, &s)) {
			columns = (uint32_t)(s.hi[0] - s.lo[0] + 1) * (uint32_t)(s.hi[2] - s.lo[2] + 1);
			for (int x = s.lo[0]; x <= s.hi[0]; x++) {
				for (int z = s.lo[2]; z <= s.hi[2]; z++) {
					const uint32_t rank = hits;
					for (int y = s.lo[1]; y <= s.hi[1]; y++) {
						float bx, by, bz;
						if (!cvxs::TriangleHit(s, x, y, z, &bx, &by, &bz)) { continue; }
						uint32_t argb;
						if (hits < cap && cvxs::TriangleColour(v0, v1, v2, bx, by, bz, m.textures.data(), m.materialCount, m.texels.data(), &argb)) { opaque++; }
						hits++;
						if (allHits) { out.insert(out.end(), { (uint32_t)(t / 3), (uint32_t)x, (uint32_t)y, (uint32_t)z }); }
					}
					most = std::max(most, hits - rank);
					if (rank < cap && cap < hits) { inside = 1; }
				}
			}
		}
		if (!allHits) { out.insert(out.end(), { columns, hits, std::min(hits, cap), opaque, most, inside }); }
	}
	return WriteFile(outPath, out);
}

static int Stamp(const char *in, const char *outPath)
{
	const std::vector<uint8_t> bytes = ReadFile(in);
	const int32_t *p = reinterpret_cast<const int32_t *>(bytes.data());
	const int32_t *end = p + bytes.size() / 4;
	std::vector<uint32_t> out;
	while (p < end) {
		const int dimY = *p++, stride = *p++;
		CaseColumn C;
		p = C.Read(p, dimY, stride);
		const int op = *p++, voxelCount = *p++;
		std::vector<std::pair<uint32_t, uint32_t>> voxels((size_t)voxelCount);
		for (int v = 0; v < voxelCount; v++) {
			voxels[(size_t)v].first = (uint32_t)*p++;
			voxels[(size_t)v].second = (uint32_t)*p++;
		}
		// the device's order: by y descending (the sort is stable; the merge does not depend on the order anyway)
		std::stable_sort(voxels.begin(), voxels.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
		std::vector<uint32_t> ys, argbs;
		for (size_t i = 0; i < voxels.size();) {
			size_t e = i + 1;
			while (e < voxels.size() && voxels[e].first == voxels[i].first) { e++; }
			std::vector<uint32_t> group;
			for (size_t k = i; k < e; k++) { group.push_back(voxels[k].second); }
			ys.push_back(voxels[i].first);
			argbs.push_back(cvxs::MergeStamped(group.data(), (int)group.size()));
			i = e;
		}
		const cvxb::ArenaColumn col = C.Column();
		const int colorShift = CaseColorShift(stride);
		const int m = (int)ys.size();
		if (!AppendEditedColumn(&out, [&](uint32_t *runs, uint32_t *colours) {
			    return cvxs::StampColumn(col, C.slots.data(), colorShift, ys.data(), argbs.data(), m, op, dimY, runs, colours);
		    })) { return 3; }
	}
	return WriteFile(outPath, out);
}

static int Args()
{
	cvx_context *ctx = new cvx_context();
	cvx_mesh_vertex v[3] = {};
	for (int k = 0; k < 3; k++) { v[k].material = -1; }
	v[1].position[0] = 4.f;
	v[2].position[2] = 4.f;
	const int32_t tri[3] = { 0, 1, 2 }, bad[3] = { 0, 1, 3 };
	cvx_mesh_vertex nanV[3] = { v[0], v[1], v[2] }, farV[3] = { v[0], v[1], v[2] };
	nanV[1].position[1] = __builtin_nanf("");
	farV[2].position[0] = 3.0e7f;
	cvx_mesh_texture emptyTex{ 0, 4, reinterpret_cast<const uint8_t *>(tri) };
	cvx_mesh_texture noTex{ 0, 0, nullptr };
	std::vector<cvx_mesh_texture> many(CVX_STAMP_MAX_MATERIALS + 1, noTex);
	const int codes[] = {
		cvx_world_stamp_mesh(nullptr, v, 3, tri, 3, nullptr, 0, CVX_BRUSH_FILL, 0, nullptr),
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, nullptr, 0, 3, 0, nullptr),           // op
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, nullptr, 0, CVX_BRUSH_FILL, 6, nullptr), // levelCount
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, nullptr, 0, CVX_BRUSH_FILL, -1, nullptr),
		cvx_world_stamp_mesh(ctx, v, 3, tri, 2, nullptr, 0, CVX_BRUSH_FILL, 0, nullptr), // indexCount
		cvx_world_stamp_mesh(ctx, v, 3, bad, 3, nullptr, 0, CVX_BRUSH_FILL, 0, nullptr), // index
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, many.data(), (int)many.size(), CVX_BRUSH_FILL, 0, nullptr), // materialCount
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, nullptr, -1, CVX_BRUSH_FILL, 0, nullptr),
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, &emptyTex, 1, CVX_BRUSH_FILL, 0, nullptr), // texture size
		cvx_world_stamp_mesh(ctx, nanV, 3, tri, 3, nullptr, 0, CVX_BRUSH_FILL, 0, nullptr), // coordinates
		cvx_world_stamp_mesh(ctx, farV, 3, tri, 3, nullptr, 0, CVX_BRUSH_FILL, 0, nullptr),
		cvx_world_stamp_mesh(ctx, v, 3, tri, 3, &noTex, 1, CVX_BRUSH_PAINT, 5, nullptr), // valid: no world yet
	};
	for (int c : codes) { std::printf("%d ", c); }
	std::printf("\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && std::strcmp(argv[1], "args") == 0) { return Args(); }
	if (argc == 4 && std::strcmp(argv[1], "voxelise") == 0) { return Voxelise(argv[2], argv[3]); }
	if (argc == 4 && std::strcmp(argv[1], "counts") == 0) { return Counts(argv[2], argv[3], false); }
	if (argc == 4 && std::strcmp(argv[1], "hits") == 0) { return Counts(argv[2], argv[3], true); }
	if (argc == 4 && std::strcmp(argv[1], "stamp") == 0) { return Stamp(argv[2], argv[3]); }
	std::fprintf(stderr, "usage: stamp_rules voxelise <mesh> <voxels> | counts <mesh> <counts> | hits <mesh> <hits> | stamp <cases> <results> | args\n");
	return 2;
}
