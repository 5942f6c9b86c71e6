// CpuVoxGpuSpread.cs -- P/Invoke binding of the travel-distance entry points of libcpuvox_gpu.so (include/cpuvox_gpu_spread.h), beside
// CpuVoxGpu.cs (include/cpuvox_gpu.h) and under the same terms: not compiled in this repository's image, dependency-free, kept honest by
// parsing (tests/test_world_spread_cpu.py compares every DllImport with the header's declaration and the structs' sizes with the header's).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvx_spread_params: the box, the medium, the directions a step may go and the cut.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxSpreadParams // 40 bytes
	{
		public fixed int boxMin[3];
		public fixed int boxMax[3]; // LOD-0 voxels, [min, max)
		public int medium;          // CVX_SPREAD_AIR, CVX_SPREAD_SOLID
		public int stepFaces;       // bits 0..5 = -X,+X,-Y,+Y,-Z,+Z: 0x3F all, 0x37 water (no +Y), 0x3B smoke (no -Y)
		public int maxSteps;        // 1 .. CVX_SPREAD_MAX_STEPS
		public int pad_;
	}

	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxSpreadSeed // 16 bytes
	{
		public fixed int voxel[3];
		public int start; // 0 .. maxSteps: the distance the seed itself has
	}

	[StructLayout(LayoutKind.Sequential)]
	public struct CvxSpreadSummary // 40 bytes
	{
		public long passable, reached;
		public int largestDistance; // -1: nothing reached
		public int seedsUsed;       // entries on a passable voxel, duplicates included
		public int launches, pad_;  // informative
		public long tileVisits;     // informative
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_spread.h.</summary>
	public static unsafe class NativeSpread
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		public const int CVX_SPREAD_AIR = 0, CVX_SPREAD_SOLID = 1;
		public const int CVX_SPREAD_UNREACHED = -1;
		public const int CVX_SPREAD_BLOCKED = -2;
		public const int CVX_SPREAD_MAX_SEEDS = 4096;
		public const int CVX_SPREAD_MAX_STEPS = 65534;
		// the travel distance from the seeds to every voxel of the box through the medium, in steps between passable face neighbours, as an
		// (X, Z, Y) int array, y fastest: the distance, CVX_SPREAD_UNREACHED or CVX_SPREAD_BLOCKED.  seeds is host memory in both calls; the
		// device call leaves the field in device memory.  summary may be null.
		[DllImport(Lib)] public static extern int cvx_world_spread(IntPtr ctx, CvxSpreadParams* parameters, CvxSpreadSeed* seeds, int seedCount, int* output,
		                                                           CvxSpreadSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_spread_device(IntPtr ctx, CvxSpreadParams* parameters, CvxSpreadSeed* seeds, int seedCount,
		                                                                  IntPtr outDevice, CvxSpreadSummary* summary, out float outDeviceMs);
	}
}
