// CpuVoxGpuSweep.cs -- P/Invoke binding of the sweep entry points of libcpuvox_gpu.so (include/cpuvox_gpu_sweep.h), beside CpuVoxGpuContacts.cs
// (whose CvxcContactResult and CvxcContactPoint the calls write) and CpuVoxGpuModels.cs (whose CvxModel and CvxModelInstance they take), and under
// the same terms: not compiled in this repository's image, dependency-free, kept honest by parsing (tests/test_abi_sweep.py compares every
// DllImport with the header's declaration and the structs with the header's, field by field).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvxs_sweep_result: how far one instance gets along its motion's lattice path.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxsSweepResult // 48 bytes
	{
		public int steps;         // n = |vx| + |vy| + |vz|
		public int hit;           // the first touching step, or -1
		public int axis;          // the axis of step `hit`; -1 when hit <= 0
		public int sign;          // the sign of v on that axis; 0 when hit <= 0
		public fixed int free[3]; // o_(hit - 1); 0 when hit == 0; v when hit == -1
		public fixed int at[3];   // o_hit; v when hit == -1
		public fixed int pad_[2];
	}

	/// <summary>cvxs_sweeps_summary: totals of one call.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxsSweepsSummary // 32 bytes
	{
		public long hits;        // instances with hit >= 0
		public long startsSolid; // instances with hit == 0
		public long jobs;        // (instance, column, station) jobs of the first phase
		public long points;      // contact points of the moved instances, whatever the capacity
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_sweep.h.</summary>
	public static unsafe class NativeSweep
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so
		public const int CVXS_MAX_MOTION = 4096; // every component of a motion

		// one sweep per instance (motions: three ints each); contacts (may be null, then pointCapacity is 0) receives cvxc_world_contacts' results
		// for the instances moved to `at`, points the first min(pointCapacity, summary.points) contact points of those
		[DllImport(Lib)] public static extern int cvxs_world_sweep(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                           int* motions, int solidOutside, CvxsSweepResult* sweeps, CvxcContactResult* contacts,
		                                                           CvxcContactPoint* points, long pointCapacity, CvxsSweepsSummary* summary, out float outDeviceMs);
		// the models' arrays, the contacts and the points are device pointers; descriptors, instances, motions, sweeps and summary are host memory
		[DllImport(Lib)] public static extern int cvxs_world_sweep_device(IntPtr ctx, CvxModel* models, int modelCount, CvxModelInstance* instances, int instanceCount,
		                                                                  int* motions, int solidOutside, CvxsSweepResult* sweeps, IntPtr contactsDevice,
		                                                                  IntPtr pointsDevice, long pointCapacity, CvxsSweepsSummary* summary, out float outDeviceMs);
		// pure host: o_j (three ints) and the axis of step j of the motion's path (-1 for j = 0)
		[DllImport(Lib)] public static extern int cvxs_sweep_offset(int* motion, int j, int* offset, int* axis);
		// pure host: the instance whose body is `instance`'s shifted by the integer offset
		[DllImport(Lib)] public static extern int cvxs_instance_moved(CvxModelInstance* instance, int* offset, CvxModelInstance* moved);
	}
}
