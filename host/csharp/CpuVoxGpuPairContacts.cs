// CpuVoxGpuPairContacts.cs -- P/Invoke binding of the pair-contact entry points of libcpuvox_gpu.so (include/cpuvox_gpu_pair_contacts.h), beside
// CpuVoxGpuContacts.cs (bodies against the world) and CpuVoxGpuModels.cs (whose CvxModel and CvxModelInstance the calls take) and under the same
// terms: not compiled in this repository's image, dependency-free, kept honest by parsing (tests/test_abi_pair_contacts.py compares every
// DllImport with the header's declaration and every struct with the header's, field by field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxp_pair_result: where the two bodies of one pair overlap.  pushA sums the open faces of body b over the overlap and is the way
	/// to move body a; pushB the open faces of body a, the way to move body b.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxpPairResult // 144 bytes
	{
		public long overlap;          // the voxels in both bodies
		public long points;           // its entries in the full list, whatever the capacity
		public long firstPoint;       // sum of `points` of the pairs before it
		public fixed ulong sum[3];    // sum over the overlap of (d - origin), modulo 2^64
		public fixed long pushA[3];   // sum over the overlap's faces open in b of their unit steps
		public fixed long pushB[3];   // ... open in a
		public fixed int origin[3];   // the per-axis maximum of the two boxMin
		public fixed int min[3];      // bounding box of the overlap, inclusive
		public fixed int max[3];      // exclusive; all 0 without overlap
		public int a, b;              // the pair, as given
		public int pad_;
	}

	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxpPairPoint // 32 bytes
	{
		public fixed int voxel[3];
		public int pair;         // its index in the pairs array
		public int facesA;       // bit f: the neighbour through face f (0..5 = -X,+X,-Y,+Y,-Z,+Z) is not in body a
		public int facesB;       // ... not in body b
		public uint argbA, argbB; // each model's colour word of the voxel's image, 0 for a model without argb
	}

	[StructLayout(LayoutKind.Sequential)]
	public struct CvxpPairsSummary // 32 bytes
	{
		public long touching;        // pairs with overlap > 0
		public long overlap, points; // totals, whatever the capacity
		public long jobs;            // the (pair, column of the common box) pairs walked
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_pair_contacts.h.</summary>
	public static unsafe class NativePairContacts
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so
		public const int CVXP_MAX_PAIRS = 65536; // cvxp_model_contacts: pairCount

		// one result per pair (pairs: pairCount x 2 indices into instances), the first min(pointCapacity, summary.points) contact points in (pair, x, z,
		// descending y) order (points may be null with capacity 0); no world is read and none need be uploaded
		[DllImport(Lib)] public static extern int cvxp_model_contacts(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                              int* pairs, int pairCount, CvxpPairResult* results, CvxpPairPoint* points, long pointCapacity,
		                                                              CvxpPairsSummary* summary, out float outDeviceMs);
		// the models' arrays, the results and the points are device pointers; descriptors, instances, pairs and summary are host memory
		[DllImport(Lib)] public static extern int cvxp_model_contacts_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                     int* pairs, int pairCount, IntPtr resultsDevice, IntPtr pointsDevice, long pointCapacity,
		                                                                     CvxpPairsSummary* summary, out float outDeviceMs);
		// pure host: every (a, b), a < b, whose boxes widened by margin intersect, in lexicographic order; found receives their number
		[DllImport(Lib)] public static extern int cvxp_box_pairs(CvxModelInstance* instances, int instanceCount, int margin, int* pairs, long pairCapacity, out long found);
		// pure host: the overlap's centre (3 doubles), the unit vector of pushA (which = 0) or pushB (1) and depth = overlap / |push|; any may be null
		[DllImport(Lib)] public static extern int cvxp_pair_response(CvxpPairResult* r, int which, double* centre, double* normal, double* depth);
	}
}
