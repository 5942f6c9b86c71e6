// CpuVoxGpuModelDraw.cs -- P/Invoke binding of the model-draw entry points of libcpuvox_gpu.so (include/cpuvox_gpu_model_draw.h), beside
// CpuVoxGpuModelPick.cs (rays against bodies), CpuVoxGpuModels.cs (whose CvxModel and CvxModelInstance the calls take) and CpuVoxGpu.cs (whose
// CameraData and PickRay they read and write), and under the same terms: not compiled in this repository's image, dependency-free, kept honest
// by parsing (tests/test_abi_model_draw.py compares every DllImport with the header's declaration and the structs with the header's, field by
// field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxv_view: the rays of a view.  Pixel (x, y), row 0 the bottom row, looks from origin along dir0 + x * dirX + y * dirY.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxvView // 96 bytes
	{
		public fixed float origin[3]; // the eye, in PickRay's space
		public float maxT;            // far limit of every pixel's ray, >= 0, +inf allowed
		public fixed double dir0[3];  // un-normalised direction through the centre of pixel (0, 0)
		public fixed double dirX[3];  // added per pixel step in x
		public fixed double dirY[3];  // added per pixel step in y
		public int width;
		public int height;
	}

	/// <summary>cvxv_draw_summary: pixel counts of one draw.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxvDrawSummary // 32 bytes
	{
		public long pixelsDrawn;    // a body shows
		public long pixelsOccluded; // a body was hit but the world lies in front
		public long jobs;           // (pixel, instance) pairs whose box the ray crosses
		public long pad_;
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_model_draw.h.</summary>
	public static unsafe class NativeModelDraw
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so
		public const int CVXV_DRAW_WORLD = 1, CVXV_DRAW_DEPTH_TEST = 2; // flags
		public const int CVXV_MAX_SIZE = 8192;                          // cvxv_view: width and height

		// the view of a camera at width x height; a host with its own camera fills CvxvView itself
		[DllImport(Lib)] public static extern int cvxv_view_from_camera(CameraData* camera, int width, int height, float maxT, CvxvView* view);
		// the rays the draw gives the pixels [x0, x0 + w) x [y0, y0 + h), row-major in that window
		[DllImport(Lib)] public static extern int cvxv_view_rays(CvxvView* view, int x0, int y0, int w, int h, PickRay* rays);
		// the nearest body of every pixel into host arrays of width * height elements; any of the three may be null, not all
		[DllImport(Lib)] public static extern int cvxv_models_draw(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                           CvxvView* view, uint flags, uint* image, float* depth, int* ids, out CvxvDrawSummary summary,
		                                                           out float outDeviceMs);
		// the models' arrays, image, depth and ids are device pointers (image: what cvx_screen_device_ptr returns after cvx_blit_segments(ctx, b, null))
		[DllImport(Lib)] public static extern int cvxv_models_draw_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                  CvxvView* view, uint flags, IntPtr imageDevice, IntPtr depthDevice, IntPtr idsDevice,
		                                                                  out CvxvDrawSummary summary, out float outDeviceMs);
	}
}
