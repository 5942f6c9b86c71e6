// CpuVoxGpuContacts.cs -- P/Invoke binding of the contact entry points of libcpuvox_gpu.so (include/cpuvox_gpu_contacts.h), beside CpuVoxGpu.cs
// (include/cpuvox_gpu.h) and CpuVoxGpuModels.cs (whose CvxModel and CvxModelInstance the calls take) and under the same terms: not compiled in
// this repository's image, dependency-free, kept honest by parsing (tests/test_abi_contacts.py compares every DllImport with the header's
// declaration and every struct with the header's, field by field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxc_contact_result: where one instance touches the world.  overlap counts the voxels a FILL of the instance would write that are
	/// already solid; normal sums their open faces and points out of the world's solid.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxcContactResult // 120 bytes
	{
		public long voxels;           // the voxels a FILL of the instance would write
		public long overlap;          // those of them that are solid already
		public long points;           // its entries in the full list, whatever the capacity
		public long firstPoint;       // sum of `points` of the instances before it
		public fixed ulong sum[3];    // sum over the overlap of (d - boxMin), modulo 2^64
		public fixed long normal[3];  // sum over the overlap's open faces of their unit steps
		public fixed int origin[3];   // the instance's boxMin
		public fixed int min[3];      // bounding box of the overlap, inclusive
		public fixed int max[3];      // exclusive; all 0 without overlap
		public int pad_;
	}

	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxcContactPoint // 24 bytes
	{
		public fixed int voxel[3];
		public int instance;
		public int faces; // bit f: the neighbour through face f (0..5 = -X,+X,-Y,+Y,-Z,+Z) is not solid
		public uint argb; // the arena's colour word of the world voxel, 0 outside the world
	}

	[StructLayout(LayoutKind.Sequential)]
	public struct CvxcContactsSummary // 32 bytes
	{
		public long touching;                // instances with overlap > 0
		public long overlap, points, voxels; // totals, whatever the capacity
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_contacts.h.</summary>
	public static unsafe class NativeContacts
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		// one result per instance, the first min(pointCapacity, summary.points) contact points in (instance, x, z, descending y) order (points may be
		// null with capacity 0); the instances' op is not read
		[DllImport(Lib)] public static extern int cvxc_world_contacts(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                              int solidOutside, CvxcContactResult* results, CvxcContactPoint* points, long pointCapacity,
		                                                              CvxcContactsSummary* summary, out float outDeviceMs);
		// the models' arrays, the results and the points are device pointers; descriptors, instances and summary are host memory
		[DllImport(Lib)] public static extern int cvxc_world_contacts_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                     int solidOutside, IntPtr resultsDevice, IntPtr pointsDevice, long pointCapacity,
		                                                                     CvxcContactsSummary* summary, out float outDeviceMs);
		// pure host: the overlap's centre (3 doubles), the unit normal (3 doubles) and depth = overlap / |normal|; any may be null
		[DllImport(Lib)] public static extern int cvxc_contact_response(CvxcContactResult* r, double* centre, double* normal, double* depth);
	}
}
