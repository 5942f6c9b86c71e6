// CpuVoxGpu.cs -- P/Invoke binding of libcpuvox_gpu.so (include/cpuvox_gpu.h) for the reference's C# host.
// No Unity, no Burst.  NOT compiled in this repository's image (no dotnet/mono/csc there); kept dependency-free
// (System.Runtime.InteropServices only) so that `dotnet build` on any machine with a .NET SDK picks it up.
// Struct layouts are the reference's own blittable structs:
//   SegmentData  <- RenderManager.SegmentData (Assets/Code/RenderManager.cs:503-510)
//   CameraData   <- CameraData (Assets/Code/Utils/CameraData.cs:11-16)
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct SegmentData
	{
		public fixed float MinScreen[2];
		public fixed float MaxScreen[2];
		public fixed float CamLocalPlaneRayMin[2];
		public fixed float CamLocalPlaneRayMax[2];
		public int RayCount;
	}

	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct CameraData
	{
		public fixed float WorldToScreenMatrix[16]; // column major: c0, c1, c2, c3 (Unity.Mathematics.float4x4)
		public fixed float PositionXZ[2];
		public float PositionY;
		public byte InverseElementIterationDirection; // C# bool in the reference struct
		fixed byte pad[3];
		public float FarClip;
		public fixed float LODDistances[6];
	}

	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct Counters
	{
		public long S, E, C, P, R;
		public fixed long LodVisits[6];
	}

	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public struct RaybufferLayout
	{
		public int Width, RayCapacity, TileRays, TileCapacity;
		public long TileBytes;
	}

	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public struct RowSpan
	{
		public long PoolRow, PackedRow;
		public int Rows, Kind;
	}

	// cvx_world_brush: one stroke (include/cpuvox_gpu.h, 40 bytes).  Op: 0 fill, 1 carve, 2 paint; Shape: 0 box [A, B), 1 sphere (centre A, radius B[0]),
	// 16 capsule (the voxels within radius Pad of the segment from voxel A to voxel B; 0 <= Pad <= 8191, |B[i] - A[i]| <= 8191, |A[i]| <= 2^30),
	// 17 ellipsoid (centre A, radii B, each 1 .. 1024).  The codes 2 .. 15 are not shapes.  Pad (pad_): the capsule's radius, ignored by every other shape.
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct BrushStroke
	{
		public int Op, Shape;
		public fixed int A[3];
		public fixed int B[3];
		public uint Argb;
		public int Pad;
	}

	// cvx_world_pick: a ray (32 bytes) and its hit (24 bytes; Face -1 = miss, 0..5 = -X, +X, -Y, +Y, -Z, +Z, 6 = started inside)
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct PickRay
	{
		public fixed float Origin[3];
		public fixed float Direction[3];
		public float MaxT, Pad;
	}

	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct PickHit
	{
		public fixed int Voxel[3];
		public int Face;
		public uint Argb;
		public float T;
	}

	// cvx_world_stamp_mesh: a mesh vertex (28 bytes, SimpleMesh.Vertex: position in LOD-0 voxels, colour, uv, material used as (sbyte)) and a
	// material's diffuse texture (16 bytes: Width x Height RGBA8 texels, row 0 = the bottom row; Rgba null = no texture)
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct MeshVertex
	{
		public fixed float Position[3];
		public fixed byte Rgba[4];
		public fixed float Uv[2];
		public int Material;
	}

	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public unsafe struct MeshTexture
	{
		public int Width, Height;
		public byte* Rgba;
	}

	// cvx_world_pieces: one floating piece (48 bytes): bounding box [Min, Max) in LOD-0 voxels, its first voxel in (x, z, descending y) order, its voxels
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public unsafe struct Piece
	{
		public fixed int Min[3];
		public fixed int Max[3];
		public fixed int Seed[3];
		public int Pad;
		public long Voxels;
	}

	// cvx_world_pieces: the totals (32 bytes)
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public struct PiecesSummary
	{
		public long FloatingPieces, FloatingVoxels, AnchoredPieces, AnchoredVoxels;
	}

	// cvx_world_settle: the totals (40 bytes): the floating pieces as PiecesSummary counts them, those that fell (drop > 0), the largest drop
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public struct SettleSummary
	{
		public long FloatingPieces, FloatingVoxels, FallenPieces, FallenVoxels;
		public int LargestDrop, Pad;
	}

	// cvx_world_cavities: the call's parameters (48 bytes).  Box [BoxMin, BoxMax) in LOD-0 voxels; OpenFaces bits 0..5 = -X,+X,-Y,+Y,-Z,+Z: the faces
	// of the clipped box air may escape through (0x3B: every face but -Y); Op 0 report, 1 fill with Argb; MaxVoxels 0: no limit
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public unsafe struct CavityParams
	{
		public fixed int BoxMin[3];
		public fixed int BoxMax[3];
		public int OpenFaces, Op;
		public uint Argb;
		public int Pad;
		public long MaxVoxels;
	}

	// cvx_world_cavities: the totals (48 bytes): every enclosed cavity, those within MaxVoxels (listed, and filled by a FILL), the open regions
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public struct CavitiesSummary
	{
		public long EnclosedCavities, EnclosedVoxels, SelectedCavities, SelectedVoxels, OpenRegions, OpenVoxels;
	}

	// cvx_world_surface: one quad (24 bytes): its lowest voxel, Face 0 .. 5 = -X, +X, -Y, +Y, -Z, +Z, Length voxels along +Y (1 for -Y / +Y), the colour word
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct SurfaceQuad
	{
		public fixed int Voxel[3];
		public int Face, Length;
		public uint Argb;
	}

	// cvx_world_surface: the totals (64 bytes): every quad whatever the capacity, the sum of their lengths (the exposed voxel faces), the quads per face
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public unsafe struct SurfaceSummary
	{
		public long Quads, UnitFaces;
		public fixed long QuadsPerFace[6];
	}

	// cvx_world_light: the call's parameters (64 bytes).  Box [BoxMin, BoxMax) in LOD-0 voxels; SunDir points TOWARDS the sun (integers, |.| <= 1024,
	// all 0: no sun term); levels 0 .. 255; SunRange 0 .. 4096 voxels of the shadow walk, SkyRange 0 .. 32 voxels per sky direction; Target 0: the
	// shade is multiplied into R, G, B (one-shot), 1: it is stored in A
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct LightParams
	{
		public fixed int BoxMin[3];
		public fixed int BoxMax[3];
		public fixed int SunDir[3];
		public int SunLevel, SunRange, SkyLevel, SkyRange, FloorLevel, Target, Pad;
	}

	// cvx_world_light_lamps: a point light (32 bytes).  Pos is the LOD-0 voxel at whose centre the lamp sits (anywhere, |.| <= 2^20); Radius 1 .. 64
	// voxels; Level 0 .. 255.  Lamps are white.
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct Lamp
	{
		public fixed int Pos[3];
		public int Radius, Level;
		public fixed int Pad[3];
	}

	// cvx_world_move: a body (48 bytes) and its result (16 bytes), in units of 1 / 256 LOD-0 voxel.  Pos is the box's min corner; Size 1 .. 64 * 256
	// per axis; |Delta| <= 256 * 256; StepUp 0 .. 4 * 256; Flags: 1 = solid below y 0, 2 = solid beyond the tile's sides.  Result flags: bits 0 .. 5
	// stopped going -X, +X, -Y, +Y, -Z, +Z; 64 resting, 128 started inside solid, 256 stepped up, 1 << 31 a body outside the limits (device call)
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct MoveBody
	{
		public fixed int Pos[3];
		public fixed int Size[3];
		public fixed int Delta[3];
		public int StepUp, Flags, Pad;
	}

	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct MoveResult
	{
		public fixed int Pos[3];
		public int Flags;
	}

	// cvx_world_nav_build: the call's parameters (48 bytes).  Box [BoxMin, BoxMax) in LOD-0 voxels; the body is Width x Height x Width voxels
	// (1 .. 8, 1 .. 64); StepUp 0 .. Height and MaxDrop 0 .. 4096 voxels per step; MaxSteps 0: no bound
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct NavParams
	{
		public fixed int BoxMin[3];
		public fixed int BoxMax[3];
		public int Width, Height, StepUp, MaxDrop, MaxSteps, Pad;
	}

	// cvx_nav_query: what a position resolves to (32 bytes).  Cell: the stand cell ({-1,-1,-1}: none); Distance: steps to the nearest goal (-1: no
	// cell or unreached); Next: the cell to step to (the own cell at a goal); Direction 0, 1, 4, 5 = -X, +X, -Z, +Z (-1: at a goal or Distance < 0)
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct NavStep
	{
		public fixed int Cell[3];
		public int Distance;
		public fixed int Next[3];
		public int Direction;
	}

	// cvx_world_nav_build / cvx_nav_field_goals: the totals (40 bytes); Launches is informative, not part of the deterministic result
	[StructLayout(LayoutKind.Sequential, Pack = 8)]
	public struct NavSummary
	{
		public long Nodes, Reached;
		public int GoalsResolved, LargestDistance;
		public long ColumnsWithSeveralNodes;
		public int Launches, Pad;
	}

	// cvx_world_copy: one placement (48 bytes).  Source box [SrcMin, SrcMax) in LOD-0 voxels, destination min corner Dst; Transform bits 0-1 quarter
	// turns, bit 2 mirror X (before turning), bit 3 flip Y; Op: 0 fill, 1 carve, 2 paint, 3 replace; Move 1: the source box becomes air
	[StructLayout(LayoutKind.Sequential, Pack = 4)]
	public unsafe struct CopyPlacement
	{
		public fixed int SrcMin[3];
		public fixed int SrcMax[3];
		public fixed int Dst[3];
		public int Transform, Op, Move;
	}

	public sealed class CvxException : Exception
	{
		public readonly int Code;
		public CvxException(int code, string message) : base(message) { Code = code; }
	}

	/// <summary>The mesh entry points of libcpuvox_host.so (include/cpuvox_host.h): OBJ import, SimpleMesh.Rescale and the arrays
	/// cvx_world_stamp_mesh takes.</summary>
	public static unsafe class MeshHost
	{
		const string HostLib = "cpuvox_host"; // libcpuvox_host.so

		[DllImport(HostLib)] public static extern int cvxh_mesh_load_obj(string path, int swapYZ, out IntPtr mesh);
		[DllImport(HostLib)] public static extern int cvxh_mesh_create(MeshVertex* vertices, int vertexCount, int* indices, long indexCount, MeshTexture* materials,
		                                                               int materialCount, out IntPtr mesh);
		[DllImport(HostLib)] public static extern int cvxh_mesh_rescale(IntPtr mesh, float maxDimension, int flipX, int flipY, int flipZ, int* outDims);
		[DllImport(HostLib)] public static extern int cvxh_mesh_vertices(IntPtr mesh, out MeshVertex* outVertices, out int outCount);
		[DllImport(HostLib)] public static extern int cvxh_mesh_indices(IntPtr mesh, out int* outIndices, out long outCount);
		[DllImport(HostLib)] public static extern int cvxh_mesh_material_count(IntPtr mesh);
		[DllImport(HostLib)] public static extern int cvxh_mesh_texture(IntPtr mesh, int material, out MeshTexture texture);
		[DllImport(HostLib)] public static extern void cvxh_mesh_free(IntPtr mesh);
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu.h.</summary>
	public static unsafe class Native
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		[DllImport(Lib)] public static extern int cvx_create(int device, out IntPtr ctx);
		[DllImport(Lib)] public static extern void cvx_destroy(IntPtr ctx);
		[DllImport(Lib)] public static extern IntPtr cvx_last_error(IntPtr ctx);
		[DllImport(Lib)] public static extern int cvx_set_stream(IntPtr ctx, IntPtr hipStream);
		[DllImport(Lib)] public static extern int cvx_world_upload(IntPtr ctx, int lod, void* storage, long byteLength, int dimX, int dimY, int dimZ, int columnCount);
		[DllImport(Lib)] public static extern int cvx_world_downsample(IntPtr ctx, void* storage, long byteLength, int dimX, int dimY, int dimZ, int lod, int columnCount, int extraLods,
		                                                               out IntPtr outStorage, out long outByteLength, out int outColumnCount, out long outVoxelCount, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_build_lods(IntPtr ctx, void* storage, long byteLength, int dimX, int dimY, int dimZ, int columnCount, int levelCount,
		                                                               IntPtr* outStorage, long* outByteLength, int* outColumnCount, out float outDeviceMs);
		[DllImport(Lib)] public static extern void cvx_free(IntPtr p);
		// World.SetVoxelColumn (World.cs:151) for a rectangle of one level / a LOD-0 rectangle + its LOD refresh, on the device-resident world
		[DllImport(Lib)] public static extern int cvx_world_set_columns(IntPtr ctx, int lod, int x0, int z0, int sizeX, int sizeZ, void* storage, long byteLength, int columnCount);
		[DllImport(Lib)] public static extern int cvx_world_edit(IntPtr ctx, int x0, int z0, int sizeX, int sizeZ, void* storage, long byteLength, int columnCount, int levelCount,
		                                                         out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_edit_stats(IntPtr ctx, out long usedBytes, out long abandonedBytes, out long spareBytes);
		// voxel brushes (a LOD-0 edit + its LOD refresh, computed on the device) and first-hit ray picking against LOD 0
		public const int CVX_SHAPE_BOX = 0, CVX_SHAPE_SPHERE = 1, CVX_SHAPE_CAPSULE = 16, CVX_SHAPE_ELLIPSOID = 17;
		[DllImport(Lib)] public static extern int cvx_world_brush(IntPtr ctx, BrushStroke* strokes, int strokeCount, int levelCount, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_pick(IntPtr ctx, int rayCount, PickRay* rays, PickHit* hits);
		[DllImport(Lib)] public static extern int cvx_world_pick_device(IntPtr ctx, int rayCount, IntPtr raysDevice, IntPtr hitsDevice, IntPtr hipStream);
		// the device-resident world read back (a rectangle / a whole level, blobs in the builder's encoding; release with cvx_free) and its arena compacted
		[DllImport(Lib)] public static extern int cvx_world_read_region(IntPtr ctx, int lod, int x0, int z0, int sizeX, int sizeZ, out IntPtr outStorage, out long outByteLength, out int outColumnCount);
		[DllImport(Lib)] public static extern int cvx_world_read_level(IntPtr ctx, int lod, out IntPtr outStorage, out long outByteLength, out int outColumnCount);
		[DllImport(Lib)] public static extern int cvx_world_compact(IntPtr ctx, out long outReclaimedBytes, out float outDeviceMs);
		// a triangle mesh voxelised on the device (the host voxeliser's rule) and merged into LOD 0 (op 0 fill, 1 carve, 2 paint) + its LOD refresh
		[DllImport(Lib)] public static extern int cvx_world_stamp_mesh(IntPtr ctx, MeshVertex* vertices, int vertexCount, int* indices, long indexCount,
		                                                               MeshTexture* materials, int materialCount, int op, int levelCount, out float outDeviceMs);
		// boxes of voxels copied, moved, turned or mirrored inside LOD 0 (every read from the world before the call) + its LOD refresh
		[DllImport(Lib)] public static extern int cvx_world_copy(IntPtr ctx, CopyPlacement* placements, int placementCount, int levelCount, out float outDeviceMs);
		// the pieces of LOD 0 inside a box that nothing anchors (anchors: 1 ground, 2 outside the box, 4 the largest; op 0 report, 1 remove + LOD refresh)
		[DllImport(Lib)] public static extern int cvx_world_pieces(IntPtr ctx, int* boxMin, int* boxMax, int anchors, int op, int levelCount, Piece* pieces,
		                                                           int pieceCapacity, PiecesSummary* summary, out float outDeviceMs);
		// the floating pieces fall straight down until they rest, at most maxDrop voxels (0: all the way); pieces: before the fall, drops: how far each fell
		public const int CVX_SETTLE_UNLIMITED = 0;
		[DllImport(Lib)] public static extern int cvx_world_settle(IntPtr ctx, int* boxMin, int* boxMax, int anchors, int maxDrop, int levelCount, Piece* pieces,
		                                                           int* drops, int pieceCapacity, SettleSummary* summary, out float outDeviceMs);
		// the enclosed cavities of LOD 0 inside a box (air regions that reach no open face of it), listed as Piece; op 1 fills them + LOD refresh
		public const int CVX_CAVITY_OPEN_DEFAULT = 0x3B;
		[DllImport(Lib)] public static extern int cvx_world_cavities(IntPtr ctx, CavityParams* cavityParams, int levelCount, Piece* cavities, int cavityCapacity,
		                                                             CavitiesSummary* summary, out float outDeviceMs);
		// sky occlusion and a sun shadow baked into the solid voxels of LOD 0 inside a box (from occupancy alone) + its LOD refresh
		[DllImport(Lib)] public static extern int cvx_world_light(IntPtr ctx, LightParams* lightParams, int levelCount, out float outDeviceMs);
		// ... with point lights in the same bake (at most CVX_LIGHT_MAX_LAMPS; lampCount 0: cvx_world_light)
		public const int CVX_LIGHT_MAX_LAMPS = 4096, CVX_LAMP_MAX_RADIUS = 64;
		[DllImport(Lib)] public static extern int cvx_world_light_lamps(IntPtr ctx, LightParams* lightParams, Lamp* lamps, int lampCount, int levelCount,
		                                                                out float outDeviceMs);
		// boxes moved through LOD 0 with collision, sliding and step-up (host arrays; device arrays with lanesPerBody 0 / 1 / 4 / 16 / 64, enqueued only)
		public const int CVX_MOVE_UNIT = 256, CVX_MOVE_SOLID_BELOW = 1, CVX_MOVE_SOLID_SIDES = 2;
		public const int CVX_MOVED_BLOCKED_MASK = 0x3F, CVX_MOVED_RESTING = 1 << 6, CVX_MOVED_STARTS_SOLID = 1 << 7, CVX_MOVED_STEPPED = 1 << 8, CVX_MOVED_INVALID = int.MinValue;
		[DllImport(Lib)] public static extern int cvx_world_move(IntPtr ctx, int bodyCount, MoveBody* bodies, MoveResult* results);
		[DllImport(Lib)] public static extern int cvx_world_move_device(IntPtr ctx, int bodyCount, IntPtr bodiesDevice, IntPtr resultsDevice, int lanesPerBody, IntPtr hipStream);
		// a walking-distance field over the places a Width x Height x Width box can stand, towards goals (int triples): built and solved on the device,
		// re-solved for new goals, queried for host or device arrays of positions (int triples -> NavStep); a snapshot, destroyed before its context
		public const int CVX_NAV_MAX_GOALS = 4096;
		[DllImport(Lib)] public static extern int cvx_world_nav_build(IntPtr ctx, NavParams* navParams, int* goals, int goalCount, out IntPtr outField, NavSummary* summary,
		                                                              out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_nav_field_goals(IntPtr ctx, IntPtr field, int* goals, int goalCount, int maxSteps, NavSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_nav_query(IntPtr ctx, IntPtr field, int count, int* cells, NavStep* steps);
		[DllImport(Lib)] public static extern int cvx_nav_query_device(IntPtr ctx, IntPtr field, int count, IntPtr cellsDevice, IntPtr stepsDevice, IntPtr hipStream);
		[DllImport(Lib)] public static extern void cvx_nav_field_destroy(IntPtr field);
		// the exposed faces of LOD 0 inside a box as coloured quads in (x, z, face, descending y) order (solidOutside bits 0 .. 5: what lies across a face of
		// the world; flags 1: colour does not end a quad); capacity 0 with no list asks for the count; the device call leaves the quads in device memory;
		// cvx_surface_triangles (host only) expands quads into 4 vertices and 6 indices each, wound outward
		public const int CVX_SURFACE_OUTSIDE_DEFAULT = 0x04, CVX_SURFACE_IGNORE_COLOUR = 1;
		[DllImport(Lib)] public static extern int cvx_world_surface(IntPtr ctx, int* boxMin, int* boxMax, int solidOutside, int flags, SurfaceQuad* quads, long quadCapacity,
		                                                            SurfaceSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_surface_device(IntPtr ctx, int* boxMin, int* boxMax, int solidOutside, int flags, IntPtr quadsDevice, long quadCapacity,
		                                                                   SurfaceSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_surface_triangles(SurfaceQuad* quads, long quadCount, MeshVertex* vertices, int* indices);
		// dense voxel boxes [boxMin, boxMax) out of and into LOD 0: element ((x - min.x) * size.z + (z - min.z)) * size.y + (y - min.y), colour words and / or a
		// 0 / 1 mask (either may be null on a read; on a write argb only for a CARVE with a mask); op: CVX_COPY_REPLACE or a CVX_BRUSH_* op; the device
		// calls take device arrays (a read enqueues on hipStream without waiting, a write reads them on the context's stream)
		[DllImport(Lib)] public static extern int cvx_world_read_voxels(IntPtr ctx, int* boxMin, int* boxMax, uint* argb, byte* solid, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_read_voxels_device(IntPtr ctx, int* boxMin, int* boxMax, IntPtr argbDevice, IntPtr solidDevice, IntPtr hipStream);
		[DllImport(Lib)] public static extern int cvx_world_write_voxels(IntPtr ctx, int* boxMin, int* boxMax, uint* argb, byte* solid, int op, int levelCount,
		                                                                 out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_write_voxels_device(IntPtr ctx, int* boxMin, int* boxMax, IntPtr argbDevice, IntPtr solidDevice, int op,
		                                                                        int levelCount, out float outDeviceMs);
		// the exact squared distance (LOD-0 voxels) of every voxel of [boxMin, boxMax) to the nearest solid / air voxel within maxDistance (1 .. 255), in the
		// dense layout above; CVX_DISTANCE_FAR where there is none; solidOutside as for cvx_world_surface; the device call leaves the field in device memory
		public const int CVX_DISTANCE_FAR = 0x7FFFFFFF, CVX_DISTANCE_TO_SOLID = 0, CVX_DISTANCE_TO_AIR = 1, CVX_DISTANCE_SIGNED = 2;
		[DllImport(Lib)] public static extern int cvx_world_distance(IntPtr ctx, int* boxMin, int* boxMax, int maxDistance, int mode, int solidOutside, int* @out,
		                                                             out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_distance_device(IntPtr ctx, int* boxMin, int* boxMax, int maxDistance, int mode, int solidOutside,
		                                                                    IntPtr outDevice, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_set_resolution(IntPtr ctx, int resolutionX, int resolutionY);
		[DllImport(Lib)] public static extern int cvx_set_buffer_count(IntPtr ctx, int bufferCount);
		[DllImport(Lib)] public static extern int cvx_draw_segments(IntPtr ctx, SegmentData* segments, CameraData* camera, int screenWidth, int screenHeight, float* vanishingPointScreenSpace, int bufferIndex, int flags);
		[DllImport(Lib)] public static extern int cvx_draw_segments_batch(IntPtr ctx, int frameCount, SegmentData* segments, CameraData* cameras, int screenWidth, int screenHeight, float* vanishingPoints, int firstBufferIndex, int flags);
		[DllImport(Lib)] public static extern int cvx_set_shard(IntPtr ctx, int shardIndex, int shardCount);
		public const int CVX_LATENCY_AUTO = 0, CVX_LATENCY_NEVER = 1, CVX_LATENCY_ALWAYS = 2;
		[DllImport(Lib)] public static extern int cvx_set_latency_kernel(IntPtr ctx, int mode);
		[DllImport(Lib)] public static extern int cvx_set_world_repeat(IntPtr ctx, int repeat);
		[DllImport(Lib)] public static extern int cvx_synchronize(IntPtr ctx);
		[DllImport(Lib)] public static extern int cvx_clear_raybuffer(IntPtr ctx, int bufferIndex, int which, uint argb);
		[DllImport(Lib)] public static extern int cvx_read_raybuffer(IntPtr ctx, int bufferIndex, int which, int firstRay, int rayCount, void* dst);
		[DllImport(Lib)] public static extern int cvx_blit_segments(IntPtr ctx, int bufferIndex, void* dstHost);
		[DllImport(Lib)] public static extern int cvx_blit_segments_batch(IntPtr ctx, int firstBufferIndex, int frameCount, void* dstDevice, out IntPtr imagesDevice);
		[DllImport(Lib)] public static extern int cvx_bind_raybuffers(IntPtr ctx, void* topDown, long topDownBytes, void* leftRight, long leftRightBytes);
		[DllImport(Lib)] public static extern int cvx_raybuffer_device_ptr(IntPtr ctx, int bufferIndex, int which, out IntPtr ptr, out long bytes);
		[DllImport(Lib)] public static extern int cvx_screen_device_ptr(IntPtr ctx, out IntPtr ptr, out long bytes);
		[DllImport(Lib)] public static extern int cvx_last_draw_ms(IntPtr ctx, out float ms);
		[DllImport(Lib)] public static extern int cvx_draw_time_stats(IntPtr ctx, out double totalMs, out int draws, int reset);
		[DllImport(Lib)] public static extern int cvx_enable_counters(IntPtr ctx, int enable);
		[DllImport(Lib)] public static extern int cvx_get_counters(IntPtr ctx, out Counters counters);
		[DllImport(Lib)] public static extern IntPtr cvx_version();
		[DllImport(Lib)] public static extern int cvx_draw_segments_placed(IntPtr ctx, int frameCount, SegmentData* segments, CameraData* cameras, int screenWidth, int screenHeight, float* vanishingPoints, long tileCount, ulong* tileOut, int flags);
		[DllImport(Lib)] public static extern int cvx_get_raybuffer_layout(IntPtr ctx, int which, out RaybufferLayout layout);
		[DllImport(Lib)] public static extern int cvx_copy_rows(IntPtr ctx, IntPtr hipStream, int toPacked, long spanCount, RowSpan* spansDevice, void* packedDevice);
		// multi-GPU: shard plan (host arithmetic), library-owned RCCL communicator, tile exchange (RenderManager.cs:358-363 sharded)
		[DllImport(Lib)] public static extern int cvx_shard_plan_create(int frameCount, SegmentData* segments, float* vanishingPoints, int screenWidth, int screenHeight, int rank, int worldSize, out IntPtr plan);
		[DllImport(Lib)] public static extern void cvx_shard_plan_destroy(IntPtr plan);
		[DllImport(Lib)] public static extern long cvx_shard_plan_tile_count(IntPtr plan);
		[DllImport(Lib)] public static extern int cvx_shard_plan_sections(IntPtr plan, long* sendStart, long* dispStart);
		[DllImport(Lib)] public static extern int cvx_shard_plan_transfer(IntPtr plan, int peer, out long sendRow, out long sendRows, out long recvRow, out long recvRows);
		[DllImport(Lib)] public static extern int cvx_shard_plan_tile_out(IntPtr plan, void* sendBase, void* dispBase, ulong* tileOut);
		[DllImport(Lib)] public static extern int cvx_comm_unique_id(void* id128);
		[DllImport(Lib)] public static extern int cvx_comm_create(IntPtr ctx, void* id128, int rank, int worldSize, out IntPtr comm);
		[DllImport(Lib)] public static extern int cvx_comm_create_timeout(IntPtr ctx, void* id128, int rank, int worldSize, double timeoutSeconds, out IntPtr comm);
		[DllImport(Lib)] public static extern int cvx_comm_destroy(IntPtr comm);
		[DllImport(Lib)] public static extern int cvx_exchange(IntPtr ctx, IntPtr plan, IntPtr comm, IntPtr hipStream, void* sendBase, void* dispBase);
		// multi-GPU, image gather: every rank blits its own tiles' pixels, the display rank receives W * H pixels per frame
		[DllImport(Lib)] public static extern int cvx_image_plan_create(IntPtr ctx, int frameCount, SegmentData* segments, float* vanishingPoints, int screenWidth, int screenHeight, int rank, int worldSize, out IntPtr plan);
		[DllImport(Lib)] public static extern void cvx_image_plan_destroy(IntPtr plan);
		[DllImport(Lib)] public static extern long cvx_image_plan_tile_count(IntPtr plan);
		[DllImport(Lib)] public static extern int cvx_image_plan_sizes(IntPtr plan, out long localStoreBytes, out long sendPixels, out long recvPixels, out int imagesDisplayed);
		[DllImport(Lib)] public static extern int cvx_image_plan_transfer(IntPtr plan, int peer, out long sendPixel, out long sendPixels, out long recvPixel, out long recvPixels);
		[DllImport(Lib)] public static extern int cvx_image_plan_tile_out(IntPtr plan, void* localStore, ulong* tileOut);
		[DllImport(Lib)] public static extern int cvx_image_pack(IntPtr ctx, IntPtr plan, IntPtr hipStream, void* localStore, void* sendStream, void* images);
		[DllImport(Lib)] public static extern int cvx_image_exchange(IntPtr ctx, IntPtr plan, IntPtr comm, IntPtr hipStream, void* sendStream, void* recvStream);
		[DllImport(Lib)] public static extern int cvx_image_unpack(IntPtr ctx, IntPtr plan, IntPtr hipStream, void* recvStream, void* images);
	}

	/// <summary>
	/// Owns the device-side state RenderManager owns in the reference (RenderManager.cs:12-56): uploaded world LODs and
	/// the raybuffer pairs.  DrawSegments has the reference's signature minus the Unity texture wrappers.
	/// </summary>
	public sealed unsafe class GpuRenderer : IDisposable
	{
		IntPtr ctx;

		public GpuRenderer(int device = 0)
		{
			int rc = Native.cvx_create(device, out ctx);
			if (rc != 0) { throw new CvxException(rc, Marshal.PtrToStringAnsi(Native.cvx_last_error(IntPtr.Zero))); }
		}

		void Check(int rc)
		{
			if (rc != 0) { throw new CvxException(rc, Marshal.PtrToStringAnsi(Native.cvx_last_error(ctx))); }
		}

		/// <summary>Replaces `fixed (World* worldPtr = worldLODs)` (RenderManager.cs:155): hand over each World's raw storage.</summary>
		public void UploadWorld(int lod, void* storageStartPointer, long byteLength, int dimX, int dimY, int dimZ, int columnCount)
		{
			Check(Native.cvx_world_upload(ctx, lod, storageStartPointer, byteLength, dimX, dimY, dimZ, columnCount));
		}

		/// <summary>World.DownSample(extraLods) (World.cs:45) on the GPU: returns the new level's storage blob (headers + elements, the
		/// layout WorldSaveFile writes), to be wrapped exactly like WorldSaveFile.Deserialize wraps a file's world (WorldSaveFile.cs:86-92).
		/// The caller copies it into its own allocation and calls <see cref="Native.cvx_free"/> on the pointer.</summary>
		public IntPtr DownSample(void* storageStartPointer, long byteLength, int dimX, int dimY, int dimZ, int lod, int columnCount, int extraLods,
		                         out long outByteLength, out int outColumnCount, out long outVoxelCount)
		{
			Check(Native.cvx_world_downsample(ctx, storageStartPointer, byteLength, dimX, dimY, dimZ, lod, columnCount, extraLods,
			                                  out IntPtr blob, out outByteLength, out outColumnCount, out outVoxelCount, out float _));
			return blob;
		}

		/// <summary>RenderManager.SetResolution (RenderManager.cs:94-109).</summary>
		public void SetResolution(int resolutionX, int resolutionY) { Check(Native.cvx_set_resolution(ctx, resolutionX, resolutionY)); }

		/// <summary>Which kernel a draw runs on: Native.CVX_LATENCY_AUTO (default: one blocking frame -> the latency kernel), _NEVER, _ALWAYS.</summary>
		public void SetLatencyKernel(int mode) { Check(Native.cvx_set_latency_kernel(ctx, mode)); }
		/// <summary>World.REPEAT_WORLD (World.cs:10): false bounded (default), true the world repeats in X and Z.</summary>
		public void SetWorldRepeat(bool repeat) { Check(Native.cvx_set_world_repeat(ctx, repeat ? 1 : 0)); }

		/// <summary>RenderManager.DrawSegments (RenderManager.cs:258-372); blocks like render.Complete().</summary>
		public void DrawSegments(SegmentData* segments4, CameraData* camera, int screenWidth, int screenHeight, float vpX, float vpY, int bufferIndex)
		{
			float* vp = stackalloc float[2];
			vp[0] = vpX;
			vp[1] = vpY;
			Check(Native.cvx_draw_segments(ctx, segments4, camera, screenWidth, screenHeight, vp, bufferIndex, 0));
		}

		/// <summary>RenderManager.BlitSegments + RayBufferBlit.shader: W*H ARGB32 pixels, row 0 = bottom.</summary>
		public void BlitSegments(int bufferIndex, void* dstArgb32) { Check(Native.cvx_blit_segments(ctx, bufferIndex, dstArgb32)); }

		/// <summary>Phase 2 of a batch in one launch; the images stay in device memory (returns the address of image 0).</summary>
		public IntPtr BlitSegmentsBatch(int firstBufferIndex, int frameCount, void* dstDevice = null) { Check(Native.cvx_blit_segments_batch(ctx, firstBufferIndex, frameCount, dstDevice, out IntPtr images)); return images; }

		/// <summary>Rows of a raybuffer in the reference's layout (RayBuffer.Native.GetRayColumn, RayBuffer.cs:121-128).</summary>
		public void ReadRayBuffer(int bufferIndex, int which, int firstRay, int rayCount, void* dst) { Check(Native.cvx_read_raybuffer(ctx, bufferIndex, which, firstRay, rayCount, dst)); }

		/// <summary>One frame sharded over worldSize GPUs (one process and one GpuRenderer per GPU): this rank renders its tiles straight into
		/// the send / display areas and the exchange completes the frames this rank displays -- the multi-GPU form of
		/// `render.Complete()` (RenderManager.cs:358-363).  comm: cvx_comm_create (the 128-byte id travels over the host's own channel).</summary>
		public void DrawSegmentsSharded(int frameCount, SegmentData* segments, CameraData* cameras, float* vanishingPoints, int screenWidth, int screenHeight,
		                                int rank, int worldSize, IntPtr comm, void* sendArea, void* displayArea)
		{
			int rc = Native.cvx_shard_plan_create(frameCount, segments, vanishingPoints, screenWidth, screenHeight, rank, worldSize, out IntPtr plan);
			if (rc != 0) { throw new CvxException(rc, Marshal.PtrToStringAnsi(Native.cvx_last_error(IntPtr.Zero))); }
			try {
				long tiles = Native.cvx_shard_plan_tile_count(plan);
				ulong[] tileOut = new ulong[Math.Max(1, tiles)];
				fixed (ulong* p = tileOut) {
					Check(Native.cvx_shard_plan_tile_out(plan, sendArea, displayArea, p));
					Check(Native.cvx_draw_segments_placed(ctx, frameCount, segments, cameras, screenWidth, screenHeight, vanishingPoints, tiles, p, 1));
				}
				Check(Native.cvx_exchange(ctx, plan, comm, IntPtr.Zero, sendArea, displayArea));
				Check(Native.cvx_synchronize(ctx));
			} finally {
				Native.cvx_shard_plan_destroy(plan);
			}
		}

		public void Dispose()
		{
			if (ctx != IntPtr.Zero) { Native.cvx_destroy(ctx); ctx = IntPtr.Zero; }
		}
	}
}
