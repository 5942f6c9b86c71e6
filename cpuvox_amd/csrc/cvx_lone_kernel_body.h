// cvx_lone_kernel_body.h -- the latency kernel (grid = 64 x tiles, block = 64: one wave per ray; see cvx_lone.h), included twice by cvx_lone.h inside
// namespace cvxk: as lone_kernel<HI> (CVX_LONE_REPEAT false: the bounded world) and as lone_repeat_kernel<HI> (true: a world that repeats in X and Z,
// cvx_set_world_repeat).  Written out rather than inlined from a shared device function for the reason given in cvx_render_kernel_body.h.
// Expects CVX_LONE_KERNEL (the kernel's name) and CVX_LONE_REPEAT; undefines both.  (No include guard: included once per instance.)
template <bool HI>
__global__ __launch_bounds__(CVX_WAVE, CVX_LONE_WAVES_PER_SIMD) void CVX_LONE_KERNEL(const DevFrame *__restrict__ frames, const DevTile *__restrict__ tiles, const DevWorld *__restrict__ world)
{
	extern __shared__ uint32_t lds[]; // [0, 64): the DDA's crossings in merged order (lone_trace_ray); [64, 64 + omax - omin]: the ray's pixel row
	uint32_t *merged = lds;
#ifdef CVX_LONE_STATS
	const unsigned long long waveStart_ = __builtin_amdgcn_s_memtime();
#endif
	const DevTile tile = tiles[blockIdx.x >> 6];
	const DevFrame &F = frames[tile.frame];
	const DevSegment &S = F.seg[tile.seg];
	const int firstLane = (int)(blockIdx.x & 63u);
	const int planeRayIndex = tile.tileInSeg * CVX_WAVE + firstLane; // RaySetupJob (:19-39)
	if (planeRayIndex >= S.rayCount) { return; }
#ifdef CVX_LONE_PRIO
	if ((int)blockIdx.x < CVX_LONE_PRIO) { __builtin_amdgcn_s_setprio(3); } // (experiment: the longest rays of the launch first in their SIMD's issue arbitration)
#endif
	const int omin = S.omin, omax = S.omax;
	LoneSeen seen;
	seen.w0 = seen.w1 = 0u; // stackalloc is zero-initialised, :208
	seen.wordBase = omin >> 5;
	seen.lane = (int)threadIdx.x;
	const gptr_tile tileOut = (gptr_tile)tile.out;
	const uint32_t laneByteOff = (uint32_t)firstLane * 4u;
	// The ray's pixel row [omin, omax] is staged in LDS and written out once, at the end: gfx9 counts loads and stores in ONE counter (vmcnt), so a
	// pixel store in the column loop would make every later wait for a colour load also wait for the store's acknowledgement from memory.  Staged, the
	// loop's only vector-memory operations are loads, and the row's stores are issued back to back with nothing waiting for them.  Every pixel starts
	// as the skybox colour (WriteSkybox / WriteSkyboxFull, :699-716: whatever is not written by a run).
	uint32_t *pix = lds + CVX_WAVE - omin;
	for (int y = omin + seen.lane; y <= omax; y += CVX_WAVE) { pix[y] = CVX_SKYBOX_ARGB; }
#ifdef CVX_LONE_STATS
	unsigned int stat_[48];
	for (int i = 0; i < 48; i++) { stat_[i] = 0u; }
	stat_[30] = (unsigned int)__builtin_amdgcn_s_memtime();
#else
	unsigned int *stat_ = nullptr;
#endif
	if (F.inverse) { // RenderJob.Execute :174-178
		lone_trace_ray<-1, HI, CVX_LONE_REPEAT>(F, S, world, planeRayIndex, seen, merged, stat_);
	} else {
		lone_trace_ray<1, HI, CVX_LONE_REPEAT>(F, S, world, planeRayIndex, seen, merged, stat_);
	}
#ifdef CVX_LONE_STATS
	stat_[16]++;
	CVX_LSEC(0);
	if (threadIdx.x == 0) {
		const unsigned long long life_ = __builtin_amdgcn_s_memtime() - waveStart_;
		for (int i = 0; i < 48; i++) { if (i != 18 && i != 19 && i != 20) { atomicAdd(&g_loneStats[i], (unsigned long long)stat_[i]); } }
		atomicAdd(&g_loneStats[18], life_);                 // sum of the waves' lives (clock ticks)
		atomicMax(&g_loneStats[19], life_);                 // the longest
		if (life_ == atomicMax(&g_loneStats[19], 0ull)) { // (the counters of the longest wave so far: racy, diagnostic only)
			g_loneStats[20] = stat_[1];
			for (int i = 0; i < 48; i++) { g_loneLongest[i] = stat_[i]; }
		}
	}
#endif
	// the row goes out: pixel y of this ray at tile row y (256 bytes per row, cvx_device.h); first every colour still on its way into the row has to be there
	__builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0) (gfx9 encoding, see cvx_kernels.h)
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	CVX_LSEC(11);
	for (int y = omin + seen.lane; y <= omax; y += CVX_WAVE) { st_pixel(tileOut, laneByteOff, y, pix[y]); }
}

#undef CVX_LONE_KERNEL
#undef CVX_LONE_REPEAT
