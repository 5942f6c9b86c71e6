// CpuVoxGpuModels.cs -- P/Invoke binding of the model-placement entry points of libcpuvox_gpu.so (include/cpuvox_gpu_models.h), beside
// CpuVoxGpu.cs (include/cpuvox_gpu.h) and under the same terms: not compiled in this repository's image, dependency-free, kept honest by
// parsing (tests/test_world_models_cpu.py compares every DllImport with the header's declaration and the structs' sizes with the header's).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvx_model_map: image_i = (m[3 i] (2 v0 + 1) + m[3 i + 1] (2 v1 + 1) + m[3 i + 2] (2 v2 + 1) + 2 t[i]) >> 17; m and t in units of 2^-16.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxModelMap // 64 bytes
	{
		public fixed int m[9]; // row-major 3 x 3
		public int pad_;
		public fixed long t[3];
	}

	/// <summary>cvx_model: dense (X, Z, Y) arrays, y fastest; host memory for cvx_world_place_models, device memory for cvx_world_place_models_device.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxModel // 32 bytes
	{
		public fixed int size[3]; // (sx, sy, sz)
		public int pad_;
		public IntPtr argb;       // uint per voxel, may be null for a model only CARVE instances use
		public IntPtr solid;      // byte per voxel, may be null: the voxels with argb != 0 are set
	}

	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxModelInstance // 96 bytes
	{
		public CvxModelMap toModel; // world voxel -> model voxel
		public fixed int boxMin[3];
		public fixed int boxMax[3]; // the world voxels the instance may touch, [min, max)
		public int model;           // index into the call's models
		public int op;              // CVX_COPY_REPLACE, CVX_BRUSH_FILL, CVX_BRUSH_CARVE, CVX_BRUSH_PAINT
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_models.h.</summary>
	public static unsafe class NativeModels
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		public const int CVX_MODELS_MAX_MODELS = 256;
		public const int CVX_MODELS_MAX_INSTANCES = 4096;
		// voxel models at any orientation and scale: the instances are applied in order, each visiting the world voxels of its box, mapping them into its
		// model (int64 fixed point, nearest voxel) and applying its op; LOD 1 .. levelCount are rebuilt over the boxes.  The read samples the world at
		// toWorld(model voxel) into (X, Z, Y) arrays (either may be null).  cvx_model_instance_from_matrix: a row-major 3 x 4 double matrix, model
		// coordinates to world voxel coordinates -> the instance (rounded inverse and a conservative box); pure host
		[DllImport(Lib)] public static extern int cvx_world_place_models(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                 int levelCount, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_place_models_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances,
		                                                                        int instanceCount, int levelCount, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_read_model(IntPtr ctx, int* size, CvxModelMap* toWorld, uint* argb, byte* solid, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_read_model_device(IntPtr ctx, int* size, CvxModelMap* toWorld, IntPtr argbDevice, IntPtr solidDevice,
		                                                                      IntPtr hipStream);
		[DllImport(Lib)] public static extern int cvx_model_instance_from_matrix(double* forward, int* size, int model, int op, CvxModelInstance* output);
	}
}
