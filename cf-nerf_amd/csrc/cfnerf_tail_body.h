// cfnerf_tail_body.h - the body of tail_bwd_kernel, tail_cot_kernel and tail_eps_kernel (cfnerf_tail.hip), included ONCE PER KERNEL between
// the braces of the kernel, with CFN_TAIL_COT 0 / 1 and CFN_TAIL_EPS 0 / 1: `A` is the kernel's TailArgs, with CFN_TAIL_COT `C` its TailCot and
// with CFN_TAIL_EPS `E` its TailEps.
// Shared as TEXT, not as a __forceinline__ template on a bool: tail_bwd_kernel lives at the register limit, and its code generation follows the
// token stream - handed to a function template (by reference, by value or field by field) the kernel allocated its scalar registers and
// scheduled its scalar code differently from the build before (5 instead of 7 SGPRs in VGPR lanes at best, profiles/r12_kernel_regs.txt).
// With CFN_TAIL_COT 0 the preprocessor leaves exactly the kernel of before, and the compiler emits exactly its code.
// CFN_TAIL_COT 1 (CFNERF_F_COTANGENTS with a cotangent for disp_map, weights or raw; each may be null):
//   disp = 1 / max(2e-10, depth / (acc + 1e-10) + 1e-10) (RUN:448) is a function of the ray's two sums depth_k = sum_s w_s z_s and acc_k = sum_s w_s:
//   a PRE-PASS of the same wave over the ray's chunks re-forms them from the stashed (e, T) stream (w = (1 - e) T, one wave_sum per latent and
//   chunk) and leaves Gd' = d_disp d disp / d depth and Ga = d_disp d disp / d acc per latent in LDS (composite_bwd_kernel's arithmetic, clamp
//   branch included); the walk then adds Gd' to Gd and Ga to g, as the white-background term enters g.  d_weights is added to g, d_raw to
//   (gz, ga) where they are formed.  The three operands are loaded at their point of use through bounded buffer descriptors, not in the
//   one-latent-ahead prefetch: the kernel lives at the register limit.
// CFN_TAIL_EPS 1 (CFNERF_F_EPS_GRAD, on top of CFN_TAIL_COT 1 - a null TailCot costs a few scalar branches, and one variant serves stashes with and
// without cotangents): d loss / d eps of this ray's [K,4] latent row, and NOTHING else - the kernel runs BESIDE tail_bwd_kernel / tail_cot_kernel,
// which write g_theta and the base-Gaussian partials as ever.  (One kernel for both was tried first: the compiler contracts the shared adjoint's
// multiply-adds differently in a different kernel - v_fma in one, v_mul + v_add in the other for the same source line - and the parameter gradient
// of a stash with the flag moved by one unit in the last place at a few entries.  "Nothing else moves" is a contract, so the launches that write
// what already existed stay the ones of before, and this variant drops their stores: the 84 g_theta accumulators, the k-part merge and its
// barriers are dead code here.)  flows_adjoint ends in d loss / d z0 per (sample, latent) and folds it over k into the base-Gaussian sums; handed
// a zeroed 8-vector in place of `gms`, it leaves this lane's d z0 there (entries 0 and 2..4).  Four wave_sums per (chunk, latent) add the lanes,
// an LDS row per latent adds the chunks (written by lane 0, as `carry` is), and at the end the wave writes rows k in [k_lo, k_hi) of its ray:
// a wave owns its (ray, k-part), so the parts never meet.  With CFN_TAIL_EPS 0 the preprocessor leaves the two kernels of before.
#pragma clang fp contract(fast)
    __shared__ float carry[kWaves][kMaxK][3];              // per latent: (g, x, D) of the first sample of the chunk behind (comp_adjoint_D)
    // merge (ksplit 2 or 4, so a ray's parts are waves of ONE workgroup): the parts past the first publish their 84 partial sums per
    // sample here and the first adds them before it writes the row - one g_theta part leaves the kernel, and backward-data neither reads
    // a second [P,128] array nor writes the sum back (K = 64: +60 MB read, +65 MB written, +4.9 % of that kernel by counters).
    __shared__ float gsh[kWaves - 1][84][64];
    const int lane = lane_id_opaque(), wave = wave_id();
    GReg gth;
    // one wave per (ray, k-part): a ray's K latent samples are independent up to the sums over k, which are left to the
    // consumers (bwd_data adds the partial g_theta's while loading them, reduce_gms adds the rows), so small batches and
    // large K still fill the chip (this kernel runs one wave per SIMD: ~360 registers)
    const int64_t unit = (int64_t)blockIdx.x * kWaves + wave;
    const int64_t ray_u = unit / A.ksplit;
    const int part = (int)(unit - ray_u * A.ksplit);
    static_assert(kWaves % kTailParts == 0 && (kTailParts & (kTailParts - 1)) == 0, "a ray's k-parts must be waves of one workgroup");
    const bool merge = A.ksplit > 1;                       // (tail_parts: 1, 2 or 4 - the divisors of the workgroup's 4 waves)
    const bool live = ray_u < A.N;
#if CFN_TAIL_EPS
    if (!live) return;                                     // (no merge, hence no barrier in this variant: a wave past the last ray just leaves)
#else
    if (!live && !merge) return;                           // (merge: every wave of the workgroup keeps step with the barriers below)
#endif
    const int64_t ray = live ? ray_u : 0;                  // (a wave past the last ray addresses ray 0 and touches nothing)
    const int S = A.S, K = A.K;
    const int Kp = (K + A.ksplit - 1) / A.ksplit, k_lo = part * Kp, k_hi = min(K, k_lo + Kp);
    const float* rr = A.rays + ray * 11;
    // CFNERF_F_EPS_ROWS: this ray's [K,4] latent row (one ray per wave: a uniform, scalar address)
    const float* const eps_ray = (A.flags & CFNERF_F_EPS_ROWS) ? A.eps + (int64_t)__builtin_amdgcn_readfirstlane((int)ray) * (K * 4) : A.eps;
    const float dnorm = sqrtf((rr[3] * rr[3] + rr[4] * rr[4]) + rr[5] * rr[5]);
    const float cE = -((A.d_ent != nullptr) ? A.d_ent[0] : 0.f) / (float)((double)A.P * (double)K);
    const bool wb = (A.flags & CFNERF_F_WHITE_BKGD) != 0;
    const float a_mean = A.flat[0], a_std = A.flat[1];
    const float r_mean[3] = {A.flat[2], A.flat[3], A.flat[4]};
    const float r_std[3] = {A.flat[5], A.flat[6], A.flat[7]};
    for (int k = lane; k < K; k += 64) { carry[wave][k][0] = 0.f; carry[wave][k][1] = 0.f; carry[wave][k][2] = 0.f; }
    float gms[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gms[i] = 0.f;

    const int nch = (S + 63) / 64;
#if CFN_TAIL_EPS
    __shared__ float epsg[kWaves][kMaxK][4];               // per latent: sum over the ray's samples of d loss / d z0 (rgb, alpha)
    for (int k = lane; k < K; k += 64) { epsg[wave][k][0] = 0.f; epsg[wave][k][1] = 0.f; epsg[wave][k][2] = 0.f; epsg[wave][k][3] = 0.f; }
#endif
#if CFN_TAIL_COT
    // pre-pass: depth_k = sum_s w_s z_s and acc_k = sum_s w_s of this wave's latents from the stashed (e, T) stream, then (Gd', Ga) per latent
    __shared__ float cot[kWaves][kMaxK][2];
    for (int k = lane; k < K; k += 64) { cot[wave][k][0] = 0.f; cot[wave][k][1] = 0.f; }
    wave_lds_turn();
    if (live && C.d_disp != nullptr) {
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool valid = s < S;
            const float zv = A.z[ray * (int64_t)S + (valid ? s : 0)];
            const int tile_s = __builtin_amdgcn_readfirstlane((int)(ray * nch + ch));
            const __amdgpu_buffer_rsrc_t at_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.at + (size_t)tile_s * K * 128), 0, K * 512, 0x00020000);
            for (int k = k_lo; k < k_hi; ++k) {
                const f32x2 at = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(at_rs, lane * 8, k * 512, /*nt*/ 0));
                const float w = valid ? (1.f - at[0]) * at[1] : 0.f;
                const float sd = wave_sum(w * zv), sa = wave_sum(w);
                if (lane == 0) { cot[wave][k][0] += sd; cot[wave][k][1] += sa; }
            }
        }
        wave_lds_turn();
        for (int k = k_lo + lane; k < k_hi; k += 64) {
            const float accd = cot[wave][k][0], acca = cot[wave][k][1];
            float Gdx = 0.f, Gax = 0.f;
            const float qq = accd / (acca + 1e-10f) + 1e-10f;
            if (qq > 1e-10f + 1e-10f) {                                        // torch.max routes the gradient to the larger argument
                const float gq = -C.d_disp[ray * (int64_t)K + k] / (qq * qq);
                Gdx = gq / (acca + 1e-10f);
                Gax = gq * (-accd / ((acca + 1e-10f) * (acca + 1e-10f)));
            }
            cot[wave][k][0] = Gdx; cot[wave][k][1] = Gax;
        }
        wave_lds_turn();
    }
#endif
    for (int ch = nch - 1; ch >= 0; --ch) {
#if !CFN_TAIL_EPS
        if (!live) { __syncthreads(); __syncthreads(); continue; }      // (merge only: a wave past the last ray)
#endif
        const int s = ch * 64 + lane;
        const bool valid = s < S;
        const int64_t p = ray * (int64_t)S + (valid ? s : 0);
        // this chunk's tile of the transposed stash pieces (cfnerf_kernels.h): [k][64 rows][4] / [k][64 rows][2], lane = row
        const int tile_s = __builtin_amdgcn_readfirstlane((int)(ray * nch + ch));       // (scalar: the tile base stays in SGPRs, a lane keeps one 32-bit offset)
        const __amdgpu_buffer_rsrc_t raw_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.raw + (size_t)tile_s * K * 256), 0, K * 1024, 0x00020000);
        const __amdgpu_buffer_rsrc_t at_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.at + (size_t)tile_s * K * 128), 0, K * 512, 0x00020000);
        float th[84];
        {
            const f32x4* tp = reinterpret_cast<const f32x4*>(A.theta + p * kThetaAll);
#pragma unroll
            for (int q = 0; q < 18; ++q) { const f32x4 v = tp[q]; th[q * 4] = v[0]; th[q * 4 + 1] = v[1]; th[q * 4 + 2] = v[2]; th[q * 4 + 3] = v[3]; }
#pragma unroll
            for (int q = 0; q < 3; ++q) { const f32x4 v = tp[kThetaRgb / 4 + q]; th[72 + q * 4] = v[0]; th[73 + q * 4] = v[1]; th[74 + q * 4] = v[2]; th[75 + q * 4] = v[3]; }
        }
        gth.clear();
        const float zv = A.z[p];
        const float dz = (s >= S - 1) ? 1e1f : A.z[p + 1] - zv;
        const float dist = dz * dnorm;

        // this kernel runs ONE wave per SIMD (nothing else covers a load's latency): the inputs of latent k + 1 are fetched
        // while latent k is processed
        struct KIn { f32x4 rv; f32x2 at; f32x4 e; float G0, G1, G2, Gd; };
        auto fetch = [&](int k) {
            KIn q;
            // touch-once and coalesced (1 KB / 512 B per wave instruction), through ONE buffer descriptor per array: the tile base and the
            // latent are scalar offsets, a lane keeps lane * 16 / lane * 8 (no 64-bit vector addresses in a kernel that lives at 256 registers)
            q.rv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(raw_rs, lane * 16, k * 1024, /*nt*/ 2));
            q.at = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(at_rs, lane * 8, k * 512, /*nt*/ 2));
            q.e = *reinterpret_cast<const f32x4*>(eps_ray + k * 4);
            q.G0 = A.d_rgb[ray * 3 * (int64_t)K + 0 * K + k]; q.G1 = A.d_rgb[ray * 3 * (int64_t)K + 1 * K + k];
            q.G2 = A.d_rgb[ray * 3 * (int64_t)K + 2 * K + k];
            q.Gd = (A.d_depth != nullptr) ? A.d_depth[ray * (int64_t)K + k] : 0.f;
            return q;
        };
        KIn nx = fetch(min(k_lo, K - 1));                  // (K not a multiple of the parts: a last part may be empty - its prefetch stays in range)
        for (int k = k_lo; k < k_hi; ++k) {
            const KIn cur = nx;
            if (k + 1 < k_hi) nx = fetch(k + 1);
            const f32x4 rv = cur.rv;
            // the forward stashed e = exp(-softplus(a) dist) and T: alpha = 1 - e is the forward's own number again (one exact subtraction),
            // and d alpha / d softplus = dist * e comes from the exponential ITSELF like torch's exp backward.  Rounds 1-4 stashed alpha and
            // multiplied by (1 - alpha): for an opaque sample - above all a ray's LAST one, whose 1e1 interval (RUN:427) makes it the largest
            // entry of the density gradient - that subtraction keeps e only to eps / e (alpha = 0.99925: 8e-5), and a single ray's
            // density-path gradient sat 10-30 x further from fp64 than torch's own fp32 autograd (tests/tools/k2_grad_diag.py, round 5)
            const float ea = cur.at[0], Tt = cur.at[1];
            const float alpha = 1.f - ea;
#if CFN_TAIL_COT
            const float G0 = cur.G0, G1 = cur.G1, G2 = cur.G2, Gd = cur.Gd + cot[wave][k][0];      // + d_disp d disp / d depth
#else
            const float G0 = cur.G0, G1 = cur.G1, G2 = cur.G2, Gd = cur.Gd;
#endif
            const float c0 = t_sigmoid(rv[0]), c1 = t_sigmoid(rv[1]), c2 = t_sigmoid(rv[2]);
            const float w = alpha * Tt;
            float g = (G0 * c0 + G1 * c1 + G2 * c2) + Gd * zv;                 // d loss / d w_s
            if (wb) g -= (G0 + G1 + G2);                                       // rgb_map += 1 - acc  (RUN:452)
#if CFN_TAIL_COT
            g += cot[wave][k][1];                                              // + d_disp d disp / d acc
            // this ray's [S,K] rows of the caller's d_weights (row-major, lane = sample at a stride of 4 K bytes) through a descriptor bounded by
            // the ray's own extent; a lane past S addresses sample 0 and its g is dropped below
            if (C.d_weights != nullptr) {
                const __amdgpu_buffer_rsrc_t dw_rs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float*>(C.d_weights + (int64_t)__builtin_amdgcn_readfirstlane((int)ray) * S * K), 0, S * K * 4, 0x00020000);
                g += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dw_rs, ((valid ? s : 0) * K + k) * 4, 0, 0));
            }
#endif
            // d loss / d alpha = T D with D = g_s - (what the samples behind s render for g), carried by its own recurrence (comp_adjoint_D,
            // cfnerf_device.h: rounds 1-5 formed g T - suffix / x from the forward's T and lost 1-2 digits per ray to the product scan's noise)
            const float xk = (1.f - alpha) + 1e-10f;                           // cumprod factor of RUN:443
            float cg = carry[wave][k][0], cx = carry[wave][k][1], cD = carry[wave][k][2];
            const float Dv = comp_adjoint_D(valid ? g : 0.f, xk, cg, cx, cD);
            if (lane == 0) { carry[wave][k][0] = cg; carry[wave][k][1] = cx; carry[wave][k][2] = cD; }
            const float dalpha = Tt * Dv;
            const float sg = t_sigmoid(rv[3]);                                 // softplus'
            float ga = dalpha * ea * dist * sg + cE * (1.f - sg);              // + d(-mean(a - softplus a))  MOD:263
            float gz[3] = {G0 * w * c0 * (1.f - c0) + cE * (1.f - 2.f * c0),   // + d(-mean(c - 2 softplus c)) MOD:278
                           G1 * w * c1 * (1.f - c1) + cE * (1.f - 2.f * c1),
                           G2 * w * c2 * (1.f - c2) + cE * (1.f - 2.f * c2)};
#if CFN_TAIL_COT
            if (C.d_raw != nullptr) {                                          // + d loss / d raw of the caller (as flows_bwd_kernel adds it)
                // ([S,K,4] rows, a stride of 16 K bytes; bounded and addressed as d_weights above, and dropped with the lane below)
                const __amdgpu_buffer_rsrc_t dr_rs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float*>(C.d_raw + (int64_t)__builtin_amdgcn_readfirstlane((int)ray) * S * K * 4), 0, S * K * 16, 0x00020000);
                const f32x4 dr = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dr_rs, ((valid ? s : 0) * K + k) * 16, 0, 0));
                gz[0] += dr[0]; gz[1] += dr[1]; gz[2] += dr[2]; ga += dr[3];
            }
#endif
            if (!valid) { ga = 0.f; gz[0] = gz[1] = gz[2] = 0.f; }

#if CFN_TAIL_EPS
            float gl[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) gl[i] = 0.f;
            flows_adjoint(th, gth, gl, cur.e, a_mean, a_std, r_mean, r_std, ga, gz, cE, valid);
            // (gl[0] = d z0 of the density latent, gl[2..4] of the colour latents)
            const float e0 = wave_sum(gl[2]), e1 = wave_sum(gl[3]), e2 = wave_sum(gl[4]), e3 = wave_sum(gl[0]);     // (lanes past S hold zeros)
            if (lane == 0) { epsg[wave][k][0] += e0; epsg[wave][k][1] += e1; epsg[wave][k][2] += e2; epsg[wave][k][3] += e3; }
#else
            flows_adjoint(th, gth, gms, cur.e, a_mean, a_std, r_mean, r_std, ga, gz, cE, valid);
#endif
        }
#if !CFN_TAIL_EPS
        if (merge) {
            if (part != 0) {
#pragma unroll
                for (int i = 0; i < 84; ++i) gsh[wave - 1][i][lane] = gth.get(i);
            }
            __syncthreads();
            if (part == 0) {
                for (int pp = 1; pp < A.ksplit; ++pp) {    // fixed order: part 0 + part 1 (+ part 2 + part 3)
#pragma unroll
                    for (int i = 0; i < 84; ++i) gth.add(i, gsh[wave + pp - 1][i][lane]);
                }
            }
            __syncthreads();                               // (the rows are free again)
            if (part == 0 && valid) store_gtheta_row(A.g_theta + p * kThetaAll, th, gth);
        } else if (valid) {
            store_gtheta_row(A.g_theta + p * kThetaAll, th, gth);
        }
#endif
    }
    if (!live) return;
#if CFN_TAIL_EPS
    // this ray's rows k in [k_lo, k_hi) of d_eps_rows [N,K,4] (an empty last part writes nothing): the chain through z0 = eps std + mean, plus
    // the ray's share of the base log-normal's direct term (MOD:268,283,286: -d_entropy eps / (K N), a colour latent a third of it)
    wave_lds_turn();
    {
        const float cB = -((A.d_ent != nullptr) ? A.d_ent[0] : 0.f) / (float)((double)A.N * (double)K);
        for (int k = k_lo + lane; k < k_hi; k += 64) {
            const f32x4 ev = *reinterpret_cast<const f32x4*>(eps_ray + k * 4);
            f32x4 o;
            o[0] = epsg[wave][k][0] * r_std[0] + cB * (1.f / 3.f) * ev[0];
            o[1] = epsg[wave][k][1] * r_std[1] + cB * (1.f / 3.f) * ev[1];
            o[2] = epsg[wave][k][2] * r_std[2] + cB * (1.f / 3.f) * ev[2];
            o[3] = epsg[wave][k][3] * a_std + cB * ev[3];
            *reinterpret_cast<f32x4*>(E.rows + (ray * K + k) * 4) = o;
        }
    }
#else
#pragma unroll
    for (int i = 0; i < 8; ++i) gms[i] = wave_sum(gms[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) A.gms_partials[unit * 8 + i] = gms[i];
    }
#endif
