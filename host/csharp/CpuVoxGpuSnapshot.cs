// CpuVoxGpuSnapshot.cs -- P/Invoke binding of the snapshot entry points of libcpuvox_gpu.so (include/cpuvox_gpu_snapshot.h), beside
// CpuVoxGpu.cs (include/cpuvox_gpu.h) and under the same terms: not compiled in this repository's image, dependency-free, kept honest by
// parsing (tests/test_world_snapshot_cpu.py compares every DllImport with the header's declaration and the structs' sizes with the header's).
using System;
using System.Runtime.InteropServices;

namespace CpuVox.Gpu
{
	/// <summary>cvx_snapshot_info: the rectangle and the levels a snapshot holds, and what it takes on the device.</summary>
	[StructLayout(LayoutKind.Sequential)]
	public struct CvxSnapshotInfo // 48 bytes
	{
		public int x0, z0, sizeX, sizeZ; // the rectangle actually held, LOD-0 columns (rounded, clipped)
		public int levelCount;           // levels 0 .. levelCount are held
		public int dimX, dimY, dimZ;     // the world it was taken from
		public long deviceBytes;
		public long elements;            // blob elements, all levels together
	}

	[StructLayout(LayoutKind.Sequential)]
	public struct CvxSnapshotChange // 16 bytes
	{
		public int x, z;       // LOD-0 column
		public int yMin, yMax; // its differing voxels lie in [yMin, yMax), both ends tight
	}

	[StructLayout(LayoutKind.Sequential)]
	public unsafe struct CvxSnapshotDiffSummary // 48 bytes
	{
		public long changedColumns, changedVoxels;
		public fixed int min[3];
		public fixed int max[3]; // bounding box of the differing voxels, incl / excl; all 0 when nothing differs
		public fixed int pad_[2];
	}

	/// <summary>Raw entry points, one per declaration of include/cpuvox_gpu_snapshot.h.  A snapshot is an IntPtr that belongs to ONE context:
	/// destroy it (cvx_snapshot_destroy) before that context.</summary>
	public static unsafe class NativeSnapshot
	{
		const string Lib = "cpuvox_gpu"; // libcpuvox_gpu.so

		public const int CVX_SNAPSHOT_IGNORE_COLOUR = 1;
		// captures the rectangle (rounded outward to 2^levelCount, clipped) at LOD 0 .. levelCount into device memory the snapshot owns
		[DllImport(Lib)] public static extern int cvx_world_snapshot(IntPtr ctx, int x0, int z0, int sizeX, int sizeZ, int levelCount, out IntPtr snapshot,
		                                                             out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_snapshot_info_get(IntPtr snap, CvxSnapshotInfo* info);
		// every held level back over its rectangle: cvx_world_read_region of it returns the bytes it returned at the capture
		[DllImport(Lib)] public static extern int cvx_world_snapshot_restore(IntPtr ctx, IntPtr snap, out float outDeviceMs);
		// the changed columns of LOD 0 against the snapshot, x ascending then z; changes receives min(changeCapacity, changedColumns) entries and may
		// be null iff the capacity is 0; summary may be null.  The device call leaves the list in device memory.
		[DllImport(Lib)] public static extern int cvx_world_snapshot_diff(IntPtr ctx, IntPtr snap, int flags, CvxSnapshotChange* changes, long changeCapacity,
		                                                                  CvxSnapshotDiffSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern int cvx_world_snapshot_diff_device(IntPtr ctx, IntPtr snap, int flags, IntPtr changesDevice, long changeCapacity,
		                                                                         CvxSnapshotDiffSummary* summary, out float outDeviceMs);
		[DllImport(Lib)] public static extern void cvx_snapshot_destroy(IntPtr snap);
	}
}
