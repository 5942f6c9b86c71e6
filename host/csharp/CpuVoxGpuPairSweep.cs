// CpuVoxGpuPairSweep.cs -- P/Invoke binding of the pair-sweep entry points of libcpuvox_gpu.so (include/cpuvox_gpu_pair_sweep.h), beside
// CpuVoxGpuSweep.cs (whose CvxsSweepResult every result begins with), CpuVoxGpuPairContacts.cs (whose CvxpPairResult the calls write) and
// CpuVoxGpuModels.cs (whose CvxModel and CvxModelInstance they take), and under the same terms: not compiled in this repository's image,
// dependency-free, kept honest by parsing (tests/test_abi_pair_sweep.py compares every DllImport with the header's declaration and the structs
// with the header's, field by field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxm_pair_sweep_result: how far body a of one pair gets along its motion relative to body b.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxmPairSweepResult // 56 bytes
	{
		public CvxsSweepResult sweep; // of a relative to b, as cvxs_world_sweep fills it
		public int a;                 // the pair, as given
		public int b;
	}

	/// <summary>cvxm_pair_sweeps_summary: totals of one call.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxmPairSweepsSummary // 32 bytes
	{
		public long hits;        // pairs with hit >= 0
		public long startsSolid; // pairs with hit == 0
		public long jobs;        // (pair, column) jobs of the first phase
		public long pad_;
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_pair_sweep.h.</summary>
	public static unsafe class NativePairSweep
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		// one sweep per pair (pairs: two ints each; motions: three ints each, of a relative to b); contacts (may be null) receives
		// cvxp_model_contacts' results with body a of every pair moved to `at`
		[DllImport(Lib)] public static extern int cvxm_pair_sweep(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                          int* pairs, int* motions, int pairCount, CvxmPairSweepResult* sweeps, CvxpPairResult* contacts,
		                                                          CvxmPairSweepsSummary* summary, out float outDeviceMs);
		// the models' arrays and the contacts are device pointers; descriptors, instances, pairs, motions, sweeps and summary are host memory
		[DllImport(Lib)] public static extern int cvxm_pair_sweep_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                 int* pairs, int* motions, int pairCount, CvxmPairSweepResult* sweeps, IntPtr contactsDevice,
		                                                                 CvxmPairSweepsSummary* summary, out float outDeviceMs);
	}
}
