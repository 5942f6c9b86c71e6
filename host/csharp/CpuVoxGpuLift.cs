// CpuVoxGpuLift.cs -- P/Invoke binding of the lift entry points of libcpuvox_gpu.so (include/cpuvox_gpu_lift.h), beside CpuVoxGpu.cs
// (include/cpuvox_gpu.h) and under the same terms: not compiled in this repository's image, dependency-free, kept honest by parsing
// (tests/test_world_lift_cpu.py compares every DllImport with the header's declaration and the structs' sizes with the header's).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvx_lifted_piece: a floating piece as cvx_world_pieces reports it (the first 48 bytes are cvx_piece's), where its box lies in the
	/// pools, and the integer sums of its voxels' coordinates relative to min, modulo 2^64.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxLiftedPiece // 128 bytes
	{
		public fixed int min[3];  // cvx_piece: bounding box in LOD-0 voxels, inclusive
		public fixed int max[3];  // exclusive
		public fixed int seed[3]; // the piece's first voxel in cvx_world_pieces' order
		public int pad_;
		public long voxels;
		public long offset;          // first element of its box in the pools; -1: listed but not stored
		public fixed ulong sum[3];    // sum of p_x, p_y, p_z over its voxels, p = v - min
		public fixed ulong moment[6]; // sums of p_x^2, p_y^2, p_z^2, p_x p_y, p_y p_z, p_z p_x
	}

	[StructLayout(LayoutKind.Sequential)]
	public struct CvxLiftSummary // 64 bytes
	{
		public long floatingPieces, floatingVoxels, anchoredPieces, anchoredVoxels; // cvx_pieces_summary
		public long storedPieces, storedVoxels; // pool elements used = sum of the stored boxes' volumes
		public long neededVoxels;               // sum of the box volumes of ALL floating pieces
		public long pad_;
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_lift.h.  A stored piece is a ready cvx_model: size = max - min, the
	/// pools advanced by offset elements.</summary>
	public static unsafe class NativeLift
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		public const int CVX_LIFT_COPY = 0;
		public const int CVX_LIFT_REMOVE = 1;
		// the floating pieces of cvx_world_pieces(REPORT) for the same box and anchors: the first min(pieceCapacity, m) listed with their sums, the
		// longest prefix whose box volumes fit voxelCapacity stored in the pools (either may be null); REMOVE turns the stored ones into air
		[DllImport(Lib)] public static extern int cvx_world_lift_pieces(IntPtr ctx, int* boxMin, int* boxMax, int anchors, int op, int levelCount,
		                                                                CvxLiftedPiece* pieces, int pieceCapacity, uint* argb, byte* solid, long voxelCapacity,
		                                                                CvxLiftSummary* summary, out float outDeviceMs);
		// the pools are device pointers; the list and the summary still come to the host
		[DllImport(Lib)] public static extern int cvx_world_lift_pieces_device(IntPtr ctx, int* boxMin, int* boxMax, int anchors, int op, int levelCount,
		                                                                       CvxLiftedPiece* pieces, int pieceCapacity, IntPtr argbDevice, IntPtr solidDevice,
		                                                                       long voxelCapacity, CvxLiftSummary* summary, out float outDeviceMs);
		// pure host: centre of mass (3 doubles) and inertia (Ixx, Iyy, Izz, Ixy, Iyz, Izx) about it for unit cubes of unit mass; either may be null
		[DllImport(Lib)] public static extern int cvx_lifted_piece_mass(CvxLiftedPiece* p, double* centre, double* inertia);
	}
}
