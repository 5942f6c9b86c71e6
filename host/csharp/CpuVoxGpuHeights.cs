// CpuVoxGpuHeights.cs -- P/Invoke binding of the height-map entry points of libcpuvox_gpu.so (include/cpuvox_gpu_heights.h), beside
// CpuVoxGpu.cs (include/cpuvox_gpu.h) and under the same terms: not compiled in this repository's image, dependency-free, kept honest by
// parsing (tests/test_world_heights_cpu.py compares every DllImport with the header's declaration).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_heights.h.</summary>
	public static unsafe class NativeHeights
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		// terrain as height maps: (X, Z) arrays, z fastest, over the footprint of [boxMin, boxMax) and the window [boxMin.y, boxMax.y).  Read: 1 + the y of the
		// highest solid voxel in the window (boxMin.y: none), its colour word, how far down the solid goes (any may be null, not all).  Write:
		// cvx_world_write_voxels of the terrain the heights stand for -- thickness 0: solid down to the window's bottom, t: a crust; argb the top voxel's
		// colour, sideArgb (may be null) that of the voxels below; flags: CVX_HEIGHTS_WALLED, the rim is a wall down to the window's bottom
		public const int CVX_HEIGHTS_WALLED = 1;
		[DllImport(Lib)] public static extern int cvx_world_read_heights(IntPtr ctx, int* boxMin, int* boxMax, int* heights, uint* argb, int* bottoms, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_read_heights_device(IntPtr ctx, int* boxMin, int* boxMax, IntPtr heightsDevice, IntPtr argbDevice,
		                                                                        IntPtr bottomsDevice, IntPtr hipStream);
		[DllImport(Lib)] public static extern int cvx_world_write_heights(IntPtr ctx, int* boxMin, int* boxMax, int* heights, uint* argb, uint* sideArgb, int thickness,
		                                                                  int flags, int op, int levelCount, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_write_heights_device(IntPtr ctx, int* boxMin, int* boxMax, IntPtr heightsDevice, IntPtr argbDevice,
		                                                                         IntPtr sideArgbDevice, int thickness, int flags, int op, int levelCount, out float outDeviceMs);
	}
}
