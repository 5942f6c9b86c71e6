// CpuVoxGpuSurfaceRects.cs -- P/Invoke binding of the merged-surface entry points of libcpuvox_gpu.so (include/cpuvox_gpu_surface_rects.h),
// beside CpuVoxGpu.cs (include/cpuvox_gpu.h) and under the same terms: not compiled in this repository's image, dependency-free, kept honest by
// parsing (tests/test_world_surface_rects_cpu.py compares every DllImport with the header's declaration and the structs' sizes with the header's).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvx_surface_rect: one rectangle of exposed voxel faces.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxSurfaceRect // 32 bytes
	{
		public fixed int voxel[3]; // the rectangle's lowest voxel (min x, min y, min z)
		public fixed int size[3];  // extent in voxels per axis; 1 along the face's normal axis
		public int face;           // 0..5 = -X,+X,-Y,+Y,-Z,+Z
		public uint argb;          // the colour word of the rectangle's first strip
	}

	/// <summary>cvx_surface_rects_summary: the totals, whatever the capacity.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxSurfaceRectsSummary // 72 bytes
	{
		public long rects;     // total rectangles
		public long strips;    // cvx_world_surface's quads for the same call
		public long unitFaces; // the exposed voxel faces
		public fixed long rectsPerFace[6];
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_surface_rects.h.</summary>
	public static unsafe class NativeSurfaceRects
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		// cvx_world_surface's quads for the same box, solidOutside and flags (Native.CVX_SURFACE_*) merged into rectangles: walls along z or x,
		// floors and ceilings into rows along x that stack along z; in (x, z, face, descending top) order of their lowest voxel.  Capacity 0 with no
		// list asks for the count; the device call leaves the rectangles in device memory; summary may be null.
		[DllImport(Lib)] public static extern int cvx_world_surface_rects(IntPtr ctx, int* boxMin, int* boxMax, int solidOutside, int flags, CvxSurfaceRect* rects,
		                                                                  long rectCapacity, CvxSurfaceRectsSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_surface_rects_device(IntPtr ctx, int* boxMin, int* boxMax, int solidOutside, int flags, IntPtr rectsDevice,
		                                                                         long rectCapacity, CvxSurfaceRectsSummary* summary, out float outDeviceMs);
		// host only: 4 vertices and 6 indices per rectangle, wound outward (a merged mesh has T-junctions)
		[DllImport(Lib)] public static extern int cvx_surface_rect_triangles(CvxSurfaceRect* rects, long rectCount, MeshVertex* vertices, int* indices);
	}
}
