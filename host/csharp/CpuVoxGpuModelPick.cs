// CpuVoxGpuModelPick.cs -- P/Invoke binding of the model-pick entry points of libcpuvox_gpu.so (include/cpuvox_gpu_model_pick.h), beside
// CpuVoxGpuContacts.cs (bodies against the world), CpuVoxGpuPairContacts.cs (bodies against bodies), CpuVoxGpuModels.cs (whose CvxModel and
// CvxModelInstance the calls take) and CpuVoxGpu.cs (whose PickRay they read), and under the same terms: not compiled in this repository's image,
// dependency-free, kept honest by parsing (tests/test_abi_model_pick.py compares every DllImport with the header's declaration and the struct
// with the header's, field by field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxq_model_hit: the first voxel of any placed instance along a ray.  A miss has voxel and modelVoxel -1, face -1, argb 0,
	/// t = the ray's maxT and instance -1.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxqModelHit // 48 bytes
	{
		public fixed int voxel[3];      // the world voxel that was hit
		public int face;                // 0..5 = -X,+X,-Y,+Y,-Z,+Z as cvx_world_pick; 6: the ray starts inside the voxel; -1: miss
		public uint argb;               // the model's colour word of modelVoxel; 0 for a model without argb
		public float t;                 // along the ray, in the direction's units
		public int instance;            // index into the call's instances
		public fixed int modelVoxel[3]; // the voxel of the model to carve or paint
		public fixed int pad_[2];
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_model_pick.h.</summary>
	public static unsafe class NativeModelPick
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so
		public const int CVXQ_PICK_MAX_RAYS = 65536; // cvxq_model_pick: rayCount

		// one hit per ray: the nearest of the instances' first voxels along it; no world is read and none need be uploaded.  For the first of world
		// or bodies pass cvx_world_pick's t as the ray's maxT
		[DllImport(Lib)] public static extern int cvxq_model_pick(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                          PickRay* rays, int rayCount, CvxqModelHit* hits, out float outDeviceMs);
		// the models' arrays, the rays and the hits are device pointers; descriptors and instances are host memory
		[DllImport(Lib)] public static extern int cvxq_model_pick_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                 IntPtr raysDevice, int rayCount, IntPtr hitsDevice, out float outDeviceMs);
	}
}
