// CpuVoxGpuModelBrush.cs -- P/Invoke binding of the model-brush entry points of libcpuvox_gpu.so (include/cpuvox_gpu_model_brush.h), beside
// CpuVoxGpu.cs (whose BrushStroke the calls take) and CpuVoxGpuModels.cs (whose CvxModel and CvxModelInstance they take), and under the same
// terms: not compiled in this repository's image, dependency-free, kept honest by parsing (tests/test_abi_model_brush.py compares every
// DllImport with the header's declaration and the structs with the header's, field by field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxd_model_result: one model after the call, touched or not.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxdModelResult // 128 bytes
	{
		public long voxels;            // set voxels after the call
		public long carved;            // voxels unset by this call
		public long painted;           // set voxels after the call that a PAINT touched; 0 for a model without argb
		public fixed ulong sum[3];     // sums of p_x, p_y, p_z over the set voxels, p the model voxel, modulo 2^64
		public fixed ulong moment[6];  // p_x^2, p_y^2, p_z^2, p_x p_y, p_y p_z, p_z p_x
		public fixed int min[3];       // the tight box of the set voxels in model coordinates, inclusive
		public fixed int max[3];       // exclusive; all 0 when none is left
		public fixed int pad_[2];
	}

	/// <summary>cvxd_instance_result: whether a body was hit, counted over its voxels before the call.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxdInstanceResult // 16 bytes
	{
		public long carved;  // body voxels inside at least one CARVE stroke
		public long painted; // of the others, those inside at least one PAINT stroke; 0 for a model without argb
	}

	/// <summary>cvxd_brush_summary: totals of one call.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxdBrushSummary // 32 bytes
	{
		public long carved;  // the sum of the models' carved
		public long painted; // the sum of the models' painted
		public long models;  // models with carved + painted > 0
		public long jobs;    // (instance, column) jobs of the call
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_model_brush.h.</summary>
	public static unsafe class NativeModelBrush
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		// CARVE and PAINT strokes in world coordinates applied to the models through their instances; the models' host arrays are written in
		// place; instanceResults and summary may be null
		[DllImport(Lib)] public static extern int cvxd_models_brush(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                            BrushStroke* strokes, int strokeCount, CvxdModelResult* modelResults,
		                                                            CvxdInstanceResult* instanceResults, CvxdBrushSummary* summary, out float outDeviceMs);
		// the models' arrays are device pointers, written in place; descriptors, instances, strokes and all results are host memory
		[DllImport(Lib)] public static extern int cvxd_models_brush_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                   BrushStroke* strokes, int strokeCount, CvxdModelResult* modelResults,
		                                                                   CvxdInstanceResult* instanceResults, CvxdBrushSummary* summary, out float outDeviceMs);
		// centre of mass and inertia in model coordinates from a model result (pure host code); either output may be null
		[DllImport(Lib)] public static extern int cvxd_model_mass(CvxdModelResult* r, double* centre, double* inertia);
	}
}
