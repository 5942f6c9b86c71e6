// cvx_render_kernel_body.h -- the render kernel (grid = tiles, block = 64: one wave; LDS: words*64 uint32), included twice by cvx_kernels.h inside
// namespace cvxk: as render_kernel<COUNT> (CVX_RENDER_REPEAT false: the bounded world) and as render_repeat_kernel<COUNT> (true: a world that repeats in
// X and Z, cvx_set_world_repeat).  One source for both; the kernel is written out here rather than inlined from a shared device function because the
// wrapper changed the bounded instances' code (register allocation, a spill in the counting build), and those must stay what they were.
// Expects CVX_RENDER_KERNEL (the kernel's name) and CVX_RENDER_REPEAT; undefines both.  (No include guard: included once per instance.)
template <bool COUNT>
__global__ __launch_bounds__(CVX_WAVE, CVX_WAVES_PER_SIMD) void CVX_RENDER_KERNEL(const DevFrame *__restrict__ frames, const DevTile *__restrict__ tiles,
                                                          const DevWorld *__restrict__ world, DevCounters *__restrict__ counters)
{
	extern __shared__ uint32_t lds[];
	const int lane = threadIdx.x;
#ifdef CVX_TILE_TIMES
	const unsigned long long tileStart_ = __builtin_amdgcn_s_memtime();
#endif
	const DevTile tile = tiles[blockIdx.x];
	const DevFrame &F = frames[tile.frame];
	const DevSegment &S = F.seg[tile.seg];

	// The mask only covers the words that hold pixels [omin, omax]; `seen` is biased so that the
	// absolute word index w of a pixel addresses seen[w * 64].
	const int omin = S.omin, omax = S.omax;
	const int wordBase = omin >> 5;
	const int words = (omax >> 5) - wordBase + 1;
	// RaySetupJob (:19-39): tile -> (segment, planeRayIndex)
	const int firstLane = tile.lanes & 0xFF, laneCount = tile.lanes ? (tile.lanes >> 8) & 0xFF : CVX_WAVE;
	const int sshift = 31 - __clz(laneCount); // laneCount is a power of two
	// 2^dupShift physical lanes per ray of a narrow sub-tile (cvx_gpu.hip DrawBatch: a wave with <= 8 active lanes issues ~3.6 x slower); the lanes of a
	// group hold the same values all the way, read and write the same mask words and store the same pixels
	const int dupShift = (tile.lanes >> 16) & 7;
	const int vlane = lane >> dupShift;
	const bool leader = (lane & ((1 << dupShift) - 1)) == 0; // one lane per ray writes the skybox pixels below (64 stores to one address are not free)
	const int planeRayIndex = tile.tileInSeg * CVX_WAVE + firstLane + vlane;
	const bool active = vlane < laneCount && planeRayIndex < S.rayCount;
	if (vlane < laneCount) {
		for (int w = 0; w < words; w++) {
			lds[(w << sshift) + vlane] = 0u; // stackalloc is zero-initialised, :208
		}
	}
	const gptr_tile tileOut = (gptr_tile)tile.out;
	const uint32_t laneByteOff = (uint32_t)(firstLane + vlane) * 4u;
	uint32_t *seen = lds + vlane - (wordBase << sshift);
	ProfLane prof;
#ifdef CVX_PROFILE_SECTIONS
	for (int i = 0; i < CVX_NSEC; i++) { prof.acc[i] = 0u; }
#ifdef CVX_PROFILE_COUNTS
	for (int i = 0; i < CVX_NSEC; i++) { prof.lanes[i] = 0u; }
#endif
	CVX_BEGIN();
#endif

	LaneCounters cnt;
	if (COUNT) {
		cnt.S = cnt.E = cnt.C = cnt.P = 0;
		for (int i = 0; i < 6; i++) { cnt.lod[i] = 0; }
	}

	if (active) {
		// RenderJob.Execute :174-178: the iteration direction is a per-frame (wave-uniform) constant
		if (F.inverse) {
			trace_ray<-1, COUNT, CVX_RENDER_REPEAT>(F, S, world, planeRayIndex, seen, sshift, tileOut, laneByteOff, cnt, prof);
		} else {
			trace_ray<1, COUNT, CVX_RENDER_REPEAT>(F, S, world, planeRayIndex, seen, sshift, tileOut, laneByteOff, cnt, prof);
		}
	}

	// WriteSkybox / WriteSkyboxFull (:699-716) for the whole wave: every pixel
	// of [omin, omax] not marked seen gets the skybox colour.
	CVX_BEGIN();
	unsigned int skyPixels = 0;
	for (int w = omin >> 5; w <= (omax >> 5); w++) {
		uint32_t todo = 0u;
		if (active && leader) { todo = ~seen[w << sshift] & range_mask(w, omin, omax); }
		const int base = w << 5;
		if (!COUNT && __ballot(todo != 0u) == 0ull) { continue; } // (a word every ray of the tile has filled -- the ground half of a frame: 3 instructions instead of 32 bit tests; round 5: -0.5 %)
#pragma unroll 4
		for (int b = 0; b < 32; b++) {
			if ((todo >> b) & 1u) {
				st_pixel_stream(tileOut, laneByteOff, base + b, CVX_SKYBOX_ARGB);
			}
		}
		if (COUNT) { skyPixels += (unsigned int)__popc(todo); }
	}

#ifdef CVX_PROFILE_SECTIONS
	CVX_END(8);
	for (int i = 0; i < CVX_NSEC; i++) {
#ifdef CVX_PROFILE_COUNTS
		unsigned long long tot = prof.acc[i], act = prof.lanes[i];
		for (int o = 32; o > 0; o >>= 1) { tot += (unsigned long long)__shfl_xor((long long)tot, o); act += (unsigned long long)__shfl_xor((long long)act, o); }
		if (lane == 0) { atomicAdd(&g_sectionCycles[i], tot); atomicAdd(&g_sectionCycles[16 + i], act); }
#else
		unsigned int mx = prof.acc[i], sum = prof.acc[i] >> 6;
		for (int o = 32; o > 0; o >>= 1) {
			mx = max(mx, (unsigned int)__shfl_xor((int)mx, o));
			sum += (unsigned int)__shfl_xor((int)sum, o);
		}
		if (lane == 0) {
			atomicAdd(&g_sectionCycles[i], (unsigned long long)mx);
			atomicAdd(&g_sectionCycles[16 + i], (unsigned long long)sum);
		}
#endif
	}
#endif
#ifdef CVX_TILE_TIMES
	if (!COUNT && lane == 0 && g_tileTimes) { g_tileTimes[blockIdx.x] = __builtin_amdgcn_s_memtime() - tileStart_; }
#endif
	if (COUNT) {
		cnt.P += skyPixels;
		atomicAdd(&counters->S, (unsigned long long)cnt.S);
		atomicAdd(&counters->E, (unsigned long long)cnt.E);
		atomicAdd(&counters->C, (unsigned long long)cnt.C);
		atomicAdd(&counters->P, (unsigned long long)cnt.P);
		atomicAdd(&counters->R, active ? 1ull : 0ull);
		for (int i = 0; i < 6; i++) {
			atomicAdd(&counters->lodVisits[i], (unsigned long long)cnt.lod[i]);
		}
	}
}

#undef CVX_RENDER_KERNEL
#undef CVX_RENDER_REPEAT
