// cfnerf_comp_bwd_body.h - the body of composite_bwd_kernel (CFN_COMP_SEAM 0: d_raw) and of comp_seam_zgrad_kernel (CFN_COMP_SEAM 1: d_z_vals,
// d_rays_d) in cfnerf_bwd.hip, included ONCE PER KERNEL between the braces of the kernel.  The adjoint of raw2outputs (RUN:411-454), one wave per
// ray, lane = sample: the forward pass, the K split, the staging and the back-to-front walk up to d loss / d alpha are this one text; the two
// kernels differ in what they take out of the walk.  Shared as TEXT, like cfnerf_comp_fwd_body.h and for its reason: the preprocessor leaves
// each kernel the statements it had - among them which products the vectoriser pairs before the contraction below can fuse them, i.e. d_raw's bits.
//   d loss / d w_s = sum_c G_c c_s + Gd' z_s + Ga + Gw_s     with  Gd' = Gd + Gdisp d disp / d depth,
//   Ga = Gdisp d disp / d acc - [white_bkgd] sum_c G_c       (disp = 1 / max(2e-10, depth / (acc + 1e-10) + 1e-10), RUN:448)
// CFN_COMP_SEAM 1:
//   d dist_s = sum_k dalpha_k e_k softplus(raw_k[3]),   d z_s = sum_k Gd'_k w_{s,k} - flow_s + flow_{s-1},   flow_s = d dist_s |d|
// (flow of the last sample is 0: its interval is the constant 1e1) and d |d| = sum_s d dist_s dz_s.  No atomics: a ray belongs to one
// wave, the latent groups are summed in their order into the wave's own d_z row (the first group overwrites, later groups add; every
// element is written and read back by the SAME lane), d |d| in a register per lane: bit-reproducible.  d_z or d_rays_d may be null.
#pragma clang fp contract(fast)      // (like the fused tail kernel: the two must agree to rounding, see tests/test_hip_unfused_seam.py)
    using M = Num<FAST>;
    using St = CompStage<KG>;
    __shared__ __attribute__((aligned(16))) float stage_all[kWaves][St::kQuads * 4];
    __shared__ float carryT[kWaves][KG][kCompMaxChunks];
    const int lane = lane_id_opaque(), wave = wave_id();
    const int64_t ray = (int64_t)blockIdx.x * kWaves + wave;
    if (ray >= N) return;
    float* stage = stage_all[wave];
    const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)(__attribute__((address_space(3))) float*)stage);
    const float* d = rays_d + ray * 3;
    const float dnorm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const float* zr = z_vals + ray * (int64_t)S;
    const i32x4 rsrc = ds_rsrc(raw + ray * (int64_t)S * K * 4, S * K * 16);
#if CFN_COMP_SEAM
    float* dzr = d_z != nullptr ? d_z + ray * (int64_t)S : nullptr;
#else
    float* drow = d_raw + ray * (int64_t)S * K * 4;
#endif
    const int nch = (S + 63) / 64;
    const bool vec_w = d_weights != nullptr && (K & 3) == 0;
    unsigned voff[KG];
#pragma unroll
    for (int j = 0; j < KG; ++j) voff[j] = St::piece_voff(lane, j, K);
    const int my_q0 = lane * KG, my_swz = St::swz(lane);
    auto fetch = [&](int ch, int g0) { St::fetch(rsrc, lds0, voff, ch, g0, K); };
    auto landed = [&]() { St::landed(); };
#if CFN_COMP_SEAM
    float dn_acc = 0.f;                                      // this lane's part of d loss / d |d|, over every group and chunk
#endif
    for (int g0 = 0; g0 < K; g0 += KG) {
        // ---- forward sums of the group's latents (depth, acc) and the transmittance entering every chunk
        float car[KG];
        float accd = 0.f, acca = 0.f;                        // lane q: latent g0 + q
#pragma unroll
        for (int q = 0; q < KG; ++q) car[q] = 1.f;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool valid = s < S;
            fetch(ch, g0);
            float zv = 0.f, dist = 0.f;
            if (valid) {
                zv = zr[s];
                const float dz = (s == S - 1) ? 1e1f : zr[s + 1] - zv;
                dist = dz * dnorm;
            }
            landed();
#pragma unroll
            for (int q = 0; q < KG; ++q) {
                if (g0 + q < K) {
                    const float r3 = stage[(my_q0 + (q ^ my_swz)) * 4 + 3];
                    const float alpha = valid ? 1.f - M::exp(-M::softplus(r3) * dist) : 0.f;
                    float incl, excl;
                    comp_scan_mul((1.f - alpha) + 1e-10f, incl, excl);
                    if (lane == 0) carryT[wave][q][ch] = car[q];
                    const float wgt = alpha * (car[q] * excl);
                    const float sd = comp_sum(wgt * zv), sa = comp_sum(wgt);
                    if (lane == q) { accd += sd; acca += sa; }
                    car[q] *= comp_last(incl);
                }
            }
        }
        // ---- cotangents of the group's latents, lane q: latent g0 + q
        float G0v = 0.f, G1v = 0.f, G2v = 0.f, Gdv = 0.f, Gav = 0.f;
        {
            const int k = g0 + lane;
            if (lane < KG && k < K) {
                G0v = d_rgb[ray * 3 * (int64_t)K + 0 * K + k]; G1v = d_rgb[ray * 3 * (int64_t)K + 1 * K + k]; G2v = d_rgb[ray * 3 * (int64_t)K + 2 * K + k];
                Gdv = (d_depth != nullptr) ? d_depth[ray * (int64_t)K + k] : 0.f;
                Gav = white_bkgd ? -(G0v + G1v + G2v) : 0.f;
                if (d_disp != nullptr) {
                    const float qq = accd / (acca + 1e-10f) + 1e-10f;
                    if (qq > 1e-10f + 1e-10f) {                                    // torch.max routes the gradient to the larger argument
                        const float gq = -d_disp[ray * (int64_t)K + k] / (qq * qq);
                        Gdv += gq / (acca + 1e-10f);
                        Gav += gq * (-accd / ((acca + 1e-10f) * (acca + 1e-10f)));
                    }
                }
            }
        }
        // ---- back to front: the transmittance adjoint as a reverse affine wave scan + a carry (see tail_bwd_kernel, comp_adjoint_D)
        float cg[KG], cx[KG], cD[KG];                        // (g, x, D) of the first sample of the chunk behind (comp_adjoint_D, cfnerf_device.h)
#pragma unroll
        for (int q = 0; q < KG; ++q) { cg[q] = 0.f; cx[q] = 0.f; cD[q] = 0.f; }
#if CFN_COMP_SEAM
        float pend = 0.f;                                    // this group's d_z of the first sample of the chunk behind, without its flow_{s-1}
#endif
        for (int ch = nch - 1; ch >= 0; --ch) {
            const int s = ch * 64 + lane;
            const bool valid = s < S;
            fetch(ch, g0);
            float zv = 0.f, dz = 0.f, dist = 0.f;       // (dz: the interval itself, for d |d| of CFN_COMP_SEAM)
            float dwv[KG];
#pragma unroll
            for (int q = 0; q < KG; ++q) dwv[q] = 0.f;
            if (valid) {
                zv = zr[s];
                dz = (s == S - 1) ? 1e1f : zr[s + 1] - zv;
                dist = dz * dnorm;
                if (d_weights != nullptr) {
                    const float* wrow = d_weights + (ray * S + s) * (int64_t)K + g0;
                    if (vec_w) {
#pragma unroll
                        for (int q = 0; q < KG; q += 4)
                            if (g0 + q < K) { const f32x4 v = *reinterpret_cast<const f32x4*>(wrow + q); dwv[q] = v[0]; dwv[q + 1] = v[1]; dwv[q + 2] = v[2]; dwv[q + 3] = v[3]; }
                    } else {
#pragma unroll
                        for (int q = 0; q < KG; ++q)
                            if (g0 + q < K) dwv[q] = wrow[q];
                    }
                }
            }
            landed();
#if CFN_COMP_SEAM
            float dd = 0.f, dzs = 0.f;                       // d loss / d dist_s, the explicit-z term of d loss / d z_s: this group's latents
#endif
#pragma unroll
            for (int q = 0; q < KG; ++q) {
                if (g0 + q < K) {
                    float* slot = stage + (my_q0 + (q ^ my_swz)) * 4;
                    const f32x4 rv = *reinterpret_cast<const f32x4*>(slot);
                    const float G0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(G0v), q)), G1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(G1v), q)),
                                G2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(G2v), q)), Gd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Gdv), q)),
                                Ga = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Gav), q));
#if CFN_COMP_SEAM                                            // (one value, in each kernel's own words: their code follows the token stream)
                    const float sp = M::softplus(rv[3]);
                    const float ea = valid ? M::exp(-sp * dist) : 1.f;
#else
                    const float ea = valid ? M::exp(-M::softplus(rv[3]) * dist) : 1.f;
#endif
                    const float alpha = 1.f - ea;
                    const float xk = (1.f - alpha) + 1e-10f;
                    float incl_m, excl_m;
                    comp_scan_mul(xk, incl_m, excl_m);
                    const float Tt = carryT[wave][q][ch] * excl_m;
                    const float c0 = t_sigmoid(rv[0]), c1 = t_sigmoid(rv[1]), c2 = t_sigmoid(rv[2]);
                    const float w = alpha * Tt;
                    float g = (G0 * c0 + G1 * c1 + G2 * c2) + Gd * zv;
                    g += Ga;
                    g += dwv[q];
                    const float dalpha = Tt * comp_adjoint_D(valid ? g : 0.f, xk, cg[q], cx[q], cD[q]);      // = g T - suffix / x, carried as the cancelled quantity
#if CFN_COMP_SEAM
                    if (valid) {
                        dd += dalpha * ea * sp;                                        // d alpha / d dist = softplus e
                        dzs += Gd * w;
                    }
#else
                    const float sg = t_sigmoid(rv[3]);                                 // softplus'
                    f32x4 o;
                    o[0] = G0 * w * c0 * (1.f - c0); o[1] = G1 * w * c1 * (1.f - c1); o[2] = G2 * w * c2 * (1.f - c2);
                    o[3] = dalpha * ea * dist * sg;                                    // d alpha / d softplus = dist e, from the exponential itself (tail_bwd_kernel)
                    *reinterpret_cast<f32x4*>(slot) = o;                               // in place: the block leaves the way it came
#endif
                }
            }
#if CFN_COMP_SEAM
            dn_acc += dd * dz;                                                         // (the last sample's dz = 1e1 included)
            const float flow = (valid && s < S - 1) ? dd * dnorm : 0.f;                // what d dist_s moves from z_s to z_{s+1}
            const float mine = dzs - flow + wave_prev_dpp(flow, 0.f);
            if (dzr != nullptr) {
                // the chunk's first sample lacks flow_{s-1}, which the chunk in front holds in its lane 63: that lane writes it, one turn later
                if (valid && (lane != 0 || ch == 0)) dzr[s] = (g0 == 0) ? mine : dzr[s] + mine;
                if (lane == 63 && ch + 1 < nch) dzr[s + 1] = (g0 == 0) ? pend + flow : dzr[s + 1] + (pend + flow);      // (a chunk in front of another is full: s + 1 < S)
            }
            pend = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mine)));
#else
            wave_lds_turn();
#pragma unroll
            for (int j = 0; j < KG; ++j) {
                const int p = j * 64 + lane, sl = p / KG, kk = (p % KG) ^ St::swz(sl);
                const int sj = ch * 64 + sl, k = g0 + kk;
                if (sj < S && k < K)
                    *reinterpret_cast<f32x4*>(drow + ((int64_t)sj * K + k) * 4) = *reinterpret_cast<const f32x4*>(stage + p * 4);
            }
#endif
        }
    }
#if CFN_COMP_SEAM
    if (d_rays_d != nullptr) {
        const float dn = comp_sum(dn_acc);
        if (lane < 3) d_rays_d[ray * 3 + lane] = dnorm > 0.f ? dn * (d[lane] / dnorm) : 0.f;      // torch.norm's subgradient at 0 is 0
    }
#endif
