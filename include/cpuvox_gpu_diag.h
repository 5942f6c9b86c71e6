/* cpuvox_gpu_diag.h -- diagnostics of the EXPERIMENT and PROFILING builds of libcpuvox_gpu (libcpuvox_gpu_exp.so: `make gpu-exp`,
 * -DCVX_EXPERIMENTS; libcpuvox_gpu_prof.so / _count.so: -DCVX_PROFILE_SECTIONS).  NOT part of the drop-in boundary: the product
 * library (libcpuvox_gpu.so, include/cpuvox_gpu.h) neither declares nor exports any of these; the tests of the device arithmetic
 * and the profiling tools load the experiment build for them. */
#ifndef CPUVOX_GPU_DIAG_H
#define CPUVOX_GPU_DIAG_H

#include "cpuvox_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Resident render-kernel workgroups (= waves) per CU the runtime predicts for a given dynamic LDS size. */
int cvx_debug_occupancy(cvx_context *ctx, int64_t ldsBytes, int *blocksPerCU);

/* Experiment build only (make gpu-exp): the shape of the last draw's launch as DrawBatch chose it.  out[0] the kernel instance (0 the counting
 * render_kernel<true>, 1 the batch kernel render_kernel<false>, 2 lone_kernel<false>, 3 lone_kernel<true>), [1] tiles of the draw, [2] waves
 * (workgroups) launched, [3] / [4] the least / most distinct rays a wave holds (lanes beyond them duplicate its rays; the latency kernel: 1),
 * [5] the largest dupShift (2^dupShift lanes per ray), [6] the split factor of the launch (0: latency kernel), [7] LDS words (x 4 bytes) per
 * wave.  CVX_ERR_NOT_READY before the first draw and in the other builds. */
int cvx_debug_last_launch(cvx_context *ctx, int64_t out[8]);

/* cvx_world_settle's last call in this process (tools/settle_bench.py): outMs (may be NULL) = device ms of the analysis, of gap + relax, of the
 * edit; outCounts (may be NULL) = solid runs in the box (-1: no call yet), relax sweeps, relax launches, 1 if one workgroup relaxed the box.
 * oneSweepPerLaunch 1 / 0: later calls relax with one sweep per launch and a host round trip between / as the product does; -1: leave it. */
int cvx_debug_settle(cvx_context *ctx, int oneSweepPerLaunch, float outMs[3], int64_t outCounts[4]);

/* cvx_world_cavities' last call in this process (tools/cavity_bench.py): outMs (may be NULL) = device ms of the analysis and of the edit (0: a
 * REPORT, or nothing selected); outCounts (may be NULL) = air intervals in the box (-1: no call yet), hook / flatten rounds. */
int cvx_debug_cavities(cvx_context *ctx, float outMs[2], int64_t outCounts[2]);

/* Diagnostic build only (make gpu-prof, -DCVX_PROFILE_SECTIONS): wave cycles spent per code section of the
 * render kernel (s_memtime stamps), accumulated over all launches.  Sections: 0 prologue/epilogue, 1 phase A
 * (DDA step + header + cull), 2 frustum clip, 3 element walk, 4 side-face setup, 5 side-face pixels,
 * 6 top/bottom setup, 7 top/bottom pixels, 8 skybox pass.  The regular build returns CVX_ERR_NOT_READY. */
int cvx_debug_section_cycles(cvx_context *ctx, uint64_t out[32], int reset); /* [16+i] = cycles/16 * active lanes of section i */
/* Counting diagnostic build only (make gpu-count): how many lanes were active each time a wave executed section i:
 * out[i * 8 + b] = executions with 8b+1 .. 8b+8 active lanes. */
int cvx_debug_section_histogram(cvx_context *ctx, uint64_t out[128], int reset);
/* Counting diagnostic build only: census of the batch kernel's frustum clip outside its all-straddle instance, per wave execution, accumulated over
 * all launches.  A lane's class at one end (Last / Next intersection) from the four compares of GetWorldBoundsClippingCamSpace: 0 straddle,
 * 1 foot below / top inside the window, 2 foot inside / top above, 3 both inside, 4 entirely outside, 5 inverted straddle (foot above, top below),
 * 6 the inverted rest.  out[7 cl + cn] = executions whose clipping lanes all have class cl at Last and cn at Next, out[49] = executions whose lanes
 * differ, out[50] = all executions.  out[51 + 3 k + j]: wave-uniform predicate k (a1 / a2 = foot / top above the window, b1 / b2 = below it, at both
 * ends; k = 0: !a1 && !b2, 1: ... && !a2, 2: ... && !b1, 3: !b1 && !a2, 4: ... && !b2, 5: ... && !a1, 6: a1 && !a2 && b2, the inverted straddle);
 * j = 0 executions in which every lane satisfies it, 1 in which some but not all do, 2 the lanes that do in the executions of j = 1.
 * out[72] = executions of the inverted-straddle instance, out[73] = of the general instance, out[74] = of the general instance with at least one
 * inverted-straddling lane in it, out[75] = those lanes.  (Prefix cvxd_: diagnostics added after the list of cvx_debug_ entry points was closed; bound by
 * cpuvox_amd.gpu wherever a library exports it.) */
int cvxd_clip_census(cvx_context *ctx, uint64_t out[96], int reset);

/* Arithmetic self-test hook used by tests: evaluates op on n float pairs on
 * the device.  op: 0 a/b, 1 sqrt(a), 2 1/sqrt(a), 3 a*b+c style lerp a+b*(b-a),
 * 4 floor, 5 ceil, 6 round-half-even, 7 (int)a with the x86 rule. */
int cvx_selftest_math(cvx_context *ctx, int op, int n, const float *a, const float *b, float *out);

/* The device prefix sum behind cvx_world_downsample (three launches, cvx_downsample.h) on a caller's array: values[0 .. n) are
 * replaced by their exclusive prefix sums (modulo 2^32), *total receives the 64-bit sum.  For tests of the tail / multi-chunk paths. */
int cvx_selftest_scan(cvx_context *ctx, int n, uint32_t *values, uint64_t *total);

/* The two inline-assembly primitives of the latency kernel (csrc/cvx_lone.h) on a caller's values, one wavefront per case:
 * op 0: the DDA's crossing chains -- out[128 w + n] = a[w] + n additions of b[w], out[128 w + 64 + n] = a[w] + n additions of -b[w] (n = 0 .. 63; a, b: `waves` floats);
 * op 1: v_writelane -- out[64 w + n] = a[64 w + n], except out[64 w + (w % 64)] = b[w] (a: 64 x waves floats, b: waves). */
int cvx_selftest_lone(cvx_context *ctx, int op, int waves, const float *a, const float *b, float *out);

#ifdef __cplusplus
}
#endif
#endif
