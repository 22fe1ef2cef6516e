// cfnerf_comp_fwd_body.h - the body of composite_kernel (cfnerf_fwd.hip, CFN_COMP_SPARSE 0) and of composite_sparse_kernel (cfnerf_cull.hip,
// CFN_COMP_SPARSE 1), included ONCE PER KERNEL between the braces of the kernel.  raw2outputs (RUN:411-454), one wave per ray, lane = sample:
// the culled render has the bits of the dense one because the two kernels are this one text.
// Shared as TEXT, like cfnerf_tail_body.h and for its reason: as __forceinline__ pieces (the ray as a struct, a latent group's step as a
// function) the same statements cost composite_sparse_kernel<8, true> 7 vector registers (62 -> 69: a wave per SIMD by the allocation table)
// and 1.5 % of its time, and composite_kernel<8, false> a spill until the fetch's offsets were taken out of the struct again.  As text the
// preprocessor leaves each kernel the statements it had, and the compiler emits the code it emitted (tools/isa_same.py, profiles/r16_kernel_regs.txt).
// CFN_COMP_SPARSE 1: `raw_c` holds the rows of the kept samples only (`slot`, `ray_start`); a chunk's staged block starts at its first kept
// row, a kept lane reads the row of its rank, a culled lane is OFF - alpha = 0, colour terms gated (its row is not its own).  No weights
// turn-around there (the path is about doing less network work).
#if CFN_COMP_SPARSE
#define CFN_COMP_ON keep
#else
#define CFN_COMP_ON valid
#endif
    using M = Num<FAST>;
    using St = CompStage<KG>;
#if !CFN_COMP_SPARSE
    constexpr int U = (KG == 8) ? 4 : 1;                     // groups per round of the weights turn-around (32 latents = one 128-byte line per sample)
#endif
    __shared__ __attribute__((aligned(16))) float stage_all[kWaves][St::kQuads * 4];
    __shared__ float sums_all[kWaves][6][kCompKB];           // [0] transmittance entering the next chunk, [1..5] rgb / depth / acc sums
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * kWaves + wave;
    if (ray >= N) return;                                    // (no workgroup barrier below: a wave leaves alone)
    float* stage = stage_all[wave];
    float (*sums)[kCompKB] = sums_all[wave];
    const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)(__attribute__((address_space(3))) float*)stage);
    const float* d = rays_d + ray * 3;
    const float dnorm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const float* zr = z_vals + ray * (int64_t)S;
#if CFN_COMP_SPARSE
    const int32_t* sr = slot + ray * (int64_t)S;
    // the ray's block of raw_c, clamped to [0, P'] and to S rows: a descriptor of exactly its bytes (S * K * 16 < 2 GiB is checked by the host)
    const int64_t total = max(ray_start[N], (int64_t)0);
    const int64_t r0 = min(max(ray_start[ray], (int64_t)0), total);
    const int64_t rows = raw_c == nullptr ? 0 : min(max(ray_start[ray + 1] - r0, (int64_t)0), min((int64_t)S, total - r0));      // (no raw: P' = 0)
    const i32x4 rsrc = ds_rsrc(raw_c + r0 * (int64_t)K * 4, (int)rows * K * 16);
#else
    const i32x4 rsrc = ds_rsrc(raw + ray * (int64_t)S * K * 4, S * K * 16);      // samples past S arrive as zeros (bounds check)
#endif
    const int nch = (S + 63) / 64;
    const bool vec_w = weights != nullptr && (K & 3) == 0;   // a lane's KG weights of a sample as 16-byte stores
    unsigned voff[KG];
#pragma unroll
    for (int j = 0; j < KG; ++j) voff[j] = St::piece_voff(lane, j, K);
#if !CFN_COMP_SPARSE
    const int my_q0 = lane * KG, my_swz = St::swz(lane);
#endif
    // Chunk-major: all latents of a chunk before the next chunk, so that raw streams through once front to back and the KG-float
    // pieces a group adds to a sample's row of `weights` complete their cache lines while these are still in L2.
    for (int kb = 0; kb < K; kb += kCompKB) {                // (K above kCompKB takes a second pass)
        const int kn = min(K - kb, kCompKB);
        sums[0][lane] = 1.f;
#pragma unroll
        for (int c = 1; c < 6; ++c) sums[c][lane] = 0.f;
#if CFN_COMP_SPARSE
        int row_ch = 0;                                      // kept rows of the chunks in front of this one
#endif
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool valid = s < S;
            float zv = 0.f, dist = 0.f;
#if CFN_COMP_SPARSE
            bool keep = false;
#endif
            if (valid) {
                zv = zr[s];
                const float dz = (s == S - 1) ? 1e1f : zr[s + 1] - zv;
                dist = dz * dnorm;
#if CFN_COMP_SPARSE
                keep = sr[s] >= 0;
#endif
            }
#if CFN_COMP_SPARSE
            const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
            const int cnt = __popcll(mask);
            if (cnt == 0 && weights == nullptr) continue;    // (uniform) an empty chunk multiplies every carry by 1.0f and adds 0.0f to every sum
            const int rank = __popcll(mask & ((1ull << lane) - 1ull));
            const int my_q0 = rank * KG, my_swz = St::swz(rank);
            for (int gi = 0; gi < kn; gi += KG) {
                const int g0 = kb + gi;
                // St::fetch with the chunk's first KEPT row in place of its first sample
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                wave_lds_turn();
                const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane((row_ch * K + g0) * 16);
#pragma unroll
                for (int j = 0; j < KG; ++j) ds_dma16(rsrc, lds0 + j * 1024, voff[j], soff);
#else
            for (int gf = 0; gf < kn; gf += KG * U) {
                float wrow_keep[KG * U];                     // (U > 1) this sample's weights of up to 32 latents, for full-line stores
#pragma unroll
                for (int i = 0; i < KG * U; ++i) wrow_keep[i] = 0.f;
#pragma unroll
                for (int gq = 0; gq < U; ++gq) {
                const int gi = gf + gq * KG;
                if (gi >= kn) continue;                      // (uniform)
                const int g0 = kb + gi;
                St::fetch(rsrc, lds0, voff, ch, g0, K);
#endif
                // lane q < KG: latent g0 + q
                const int sl = gi + (lane < KG ? lane : 0);
                float carv = sums[0][sl], acc0 = sums[1][sl], acc1 = sums[2][sl], acc2 = sums[3][sl], accd = sums[4][sl], acca = sums[5][sl];
                St::landed();
                float wv[KG];
#pragma unroll
                for (int q = 0; q < KG; ++q) {
                    wv[q] = 0.f;
                    if (gi + q < kn) {                       // (uniform)
                        const f32x4 rv = *reinterpret_cast<const f32x4*>(stage + (my_q0 + (q ^ my_swz)) * 4);
                        const float car = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(carv), q));
                        const float alpha = CFN_COMP_ON ? 1.f - M::exp(-M::softplus(rv[3]) * dist) : 0.f;
                        const float xk = (1.f - alpha) + 1e-10f;
                        float incl, excl;
                        comp_scan_mul(xk, incl, excl);
                        const float wgt = alpha * (car * excl);
                        wv[q] = wgt;
#if CFN_COMP_SPARSE
                        const float c0 = keep ? wgt * M::sigmoid(rv[0]) : 0.f, c1 = keep ? wgt * M::sigmoid(rv[1]) : 0.f,
                                    c2 = keep ? wgt * M::sigmoid(rv[2]) : 0.f;
                        const float s0 = comp_sum(c0), s1 = comp_sum(c1), s2 = comp_sum(c2);                  // RUN:431,444
#else
                        const float s0 = comp_sum(wgt * M::sigmoid(rv[0])), s1 = comp_sum(wgt * M::sigmoid(rv[1])), s2 = comp_sum(wgt * M::sigmoid(rv[2]));
#endif
                        const float sd = comp_sum(wgt * zv), sa = comp_sum(wgt);                              // RUN:447,449
                        const float carn = car * comp_last(incl);
                        if (lane == q) { acc0 += s0; acc1 += s1; acc2 += s2; accd += sd; acca += sa; carv = carn; }   // (chunk by chunk like the fused kernel)
                    }
                }
                if (lane < KG) { sums[0][sl] = carv; sums[1][sl] = acc0; sums[2][sl] = acc1; sums[3][sl] = acc2; sums[4][sl] = accd; sums[5][sl] = acca; }
#if !CFN_COMP_SPARSE
                if (U > 1 && vec_w) {
#pragma unroll
                    for (int q = 0; q < KG; ++q) wrow_keep[gq * KG + q] = wv[q];
                } else
#endif
                if (weights != nullptr && valid) {
                    float* wrow = weights + (ray * S + s) * (int64_t)K + g0;
                    if (vec_w) {                             // (K <= 4: a sample's row is one 16-byte store, rows adjacent)
#pragma unroll
                        for (int q = 0; q < KG; q += 4)
                            if (gi + q < kn) { f32x4 o; o[0] = wv[q]; o[1] = wv[q + 1]; o[2] = wv[q + 2]; o[3] = wv[q + 3]; *reinterpret_cast<f32x4*>(wrow + q) = o; }
                    } else {
#pragma unroll
                        for (int q = 0; q < KG; ++q)
                            if (gi + q < kn) wrow[q] = wv[q];
                    }
                }
#if CFN_COMP_SPARSE
            }
            row_ch += cnt;
#else
                }
                if (U > 1 && vec_w) {
                    // Up to 32 latents = 128 bytes per sample: turned around in the (now free) LDS block so that 8 lanes write one sample's
                    // full line - a lane's own 16- or 32-byte pieces at a pitch of 4 K bytes took 414 instead of ~290 us at K = 32
                    // (a timing-only build with a contiguous layout).  Quad kq of sample sl sits at sl * 8 + (kq ^ swz(sl)).
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    wave_lds_turn();
#pragma unroll
                    for (int kq = 0; kq < 8; ++kq) {
                        f32x4 o; o[0] = wrow_keep[kq * 4]; o[1] = wrow_keep[kq * 4 + 1]; o[2] = wrow_keep[kq * 4 + 2]; o[3] = wrow_keep[kq * 4 + 3];
                        *reinterpret_cast<f32x4*>(stage + (lane * 8 + (kq ^ my_swz)) * 4) = o;
                    }
                    wave_lds_turn();
                    float* wblk = weights + (ray * S + (int64_t)ch * 64) * K + kb + gf;
                    f32x4 ov[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int sl = j * 8 + (lane >> 3), kq = lane & 7;
                        ov[j] = *reinterpret_cast<const f32x4*>(stage + (sl * 8 + (kq ^ St::swz(sl))) * 4);
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int sl = j * 8 + (lane >> 3), kq = lane & 7;
                        if (ch * 64 + sl < S && gf + kq * 4 < kn) *reinterpret_cast<f32x4*>(wblk + (int64_t)sl * K + kq * 4) = ov[j];
                    }
                }
            }
#endif
        }
        wave_lds_turn();
        if (lane < kn) {                                     // lane l: latent kb + l
            const int k = kb + lane;
            float r0c = sums[1][lane], r1c = sums[2][lane], r2c = sums[3][lane];
            const float rd = sums[4][lane], ra = sums[5][lane];
            if (white_bkgd) { r0c = r0c + (1.f - ra); r1c = r1c + (1.f - ra); r2c = r2c + (1.f - ra); }
            float* o = rgb_map + ray * 3 * (int64_t)K;
            o[0 * K + k] = r0c; o[1 * K + k] = r1c; o[2 * K + k] = r2c;
            disp_map[ray * (int64_t)K + k] = 1.f / fmaxf(1e-10f + 1e-10f, rd / (ra + 1e-10f) + 1e-10f);
            depth_map[ray * (int64_t)K + k] = rd;
        }
        wave_lds_turn();
    }
#undef CFN_COMP_ON
