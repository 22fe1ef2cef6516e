// cfnerf_fwd_trunk_body.h - phases 1-3 of a tile of fused_fwd_kernel (CFN_FWD_GEOM 0) and of geom_fwd_kernel (CFN_FWD_GEOM 1), both in
// cfnerf_fwd.hip: sampling along the ray, the positional encoding and its parking for the skip layer, the trunk.  Included ONCE PER KERNEL
// at the top of the tile loop; it leaves `tl_cur`, the operand entry fetched for the phase behind the trunk.  The geometry-only launch has the
// bits of the unflagged one because the two kernels run this one text (tests/test_hip_geometry.py).
// Shared as TEXT, like cfnerf_comp_fwd_body.h and for its reason: the h_alpha sum as a __forceinline__ function changed the code of all 24
// kernels of a width.  As text the preprocessor leaves each kernel the statements it had (tools/isa_same.py, profiles/r17_forward_refactor.txt).
// The including kernel supplies the constants the text branches on - kGeom = CFN_FWD_GEOM, and in the geometry kernel TRAIN = Q4 = false -
// so what the geometry kernel lacks is a folded condition here, not a second copy:
//   (a) no stash: destinations and mask bits are null constants                 (b) behind the trunk comes T.ha, not T.ft, and no bias prefetch
//   (c) kParkRegs: there is no train variant                                    (d) explicit depths: the sample table is not read
//   (e) the lists of scalars fetched together differ: the one #if below
            // global point index of row 0 and number of valid rows of this tile
            const int64_t p0 = (MODE == 0) ? unit * (int64_t)S + (int64_t)chunk * kTileM : unit * (int64_t)kTileM;
            const int rows_valid = (MODE == 0) ? min(kTileM, S - chunk * kTileM) : (int)min((int64_t)kTileM, A.P - p0);
            [[maybe_unused]] const int64_t tile_idx = (MODE == 0) ? unit * chunks_per_ray + chunk : unit;
            [[maybe_unused]] constexpr int kMbStride = (W / 32) * 64;        // mask words per (layer, tile)

            // ---- 1. sampling along the ray (RUN:510-534): z for rows 0..64, pts for rows 0..63
            if (MODE == 0) {
                const float* const a_zin = A.z_in;
                const float* const a_tv = A.t_vals;
                const float* const a_tr = A.t_rand;
                float* const a_pts = A.pts;
                float* const a_stz = kGeom ? nullptr : A.st_z;
                const int a_flags = A.flags;
#if CFN_FWD_GEOM        // an asm operand per scalar: a null constant in the list would cost the geometry kernel a register
                fetched_together(a_zin, a_tv, a_tr, a_pts, a_flags);
#else
                fetched_together(a_zin, a_tv, a_tr, a_pts, a_stz, a_flags);
#endif
                if (tid <= kTileM) {
                    const int s = chunk * kTileM + tid;
                    float zv = 0.f, px = 0.f, py = 0.f, pz = 0.f;
                    if (s < S) {
                        // every input of this sample is requested before the first is used (round 4): written as nested conditionals the
                        // loads sat behind one another, each with its own full wait - four serialised memory round trips at every tile
                        // start, with 191 of the workgroup's 256 threads waiting at the barrier below.  Same arithmetic.
                        const int64_t si = unit * (int64_t)S + s;
                        // geometry kernel, explicit depths: the sample table is NOT read (it may be NULL or shorter than S, include/cfnerf.h) - the
                        // condition is wave-uniform and taken once around the three loads, which still leave together in front of one wait
                        float tv0 = 0.f, tvp = 0.f, tvm = 0.f;
                        if (!kGeom || a_zin == nullptr) { tv0 = a_tv[s]; tvp = a_tv[min(s + 1, S - 1)]; tvm = a_tv[max(s - 1, 0)]; }
                        float trv = 0.f, zin = 0.f;
                        if (a_tr != nullptr) trv = a_tr[si];
                        if (a_zin != nullptr) zin = a_zin[si];
                        if (a_zin != nullptr) {
                            zv = zin;                                                              // explicit depths (extension)
                        } else {
                            const bool lind = (a_flags & CFNERF_F_LINDISP) != 0;
                            const float zc = zlin_f(tv0, nearv, farv, lind);
                            zv = zc;
                            if (a_tr != nullptr) zv = strat_jitter(zc, tvp, tvm, trv, s == 0, s == S - 1, nearv, farv, lind);      // RUN:518-532
                        }
                        px = ro[0] + rd[0] * zv; py = ro[1] + rd[1] * zv; pz = ro[2] + rd[2] * zv;  // RUN:534
                        if (tid < kTileM) {
                            if (a_pts != nullptr) {
                                float* o = a_pts + (unit * (int64_t)S + s) * 3;
                                o[0] = px; o[1] = py; o[2] = pz;
                            }
                            if (a_stz != nullptr) a_stz[unit * (int64_t)S + s] = zv;
                        }
                    }
                    float* ri = rowinfo + tid * 4;
                    ri[0] = px; ri[1] = py; ri[2] = pz; ri[3] = zv;
                }
                __syncthreads();
            }
            // Biases are fetched ONE PHASE AHEAD of the accumulator initialisation that needs them (the accumulators must
            // hold them before a layer's first MFMA, so a fetch at the top of the layer is an exposed L2 round trip per layer):
            // layer 0's rides under the encoding, layer l+1's under layer l's MFMAs, and so on down the heads.
            float bias_n[C::NTW];
            // Operand-table entries travel ONE PHASE AHEAD as well (16 bytes = one s_load_dwordx4 each, cfnerf_device.h: kload): a trunk layer
            // runs on the entry fetched two layers earlier, prefetches the next layer's bias with the entry fetched one layer earlier, and
            // fetches the one after - so no layer starts by waiting for the constant cache in front of its first weight loads.
            // Behind the last trunk layer comes the feature head (T.ft) - in the geometry kernel the h_alpha head (T.ha).
            SubL tl_cur = kload(T.trunk[0]);
            SubL tl_nxt = kload((1 < Dn) ? T.trunk[1] : (kGeom ? T.ha : T.ft));
            const SubL tl_skip = kload(T.skipseg);
            // ... and so do the stash destinations of the layer epilogues: this tile's rows of layer 0 + a per-layer stride, fetched here
            // (four constant-cache round trips per layer when each field is loaded at its first use behind the epilogue's barrier)
            [[maybe_unused]] float* const te_st0 = (!kGeom && A.st_h != nullptr) ? A.st_h + (size_t)p0 * W : nullptr;
            [[maybe_unused]] uint32_t* const te_mb0 = (!kGeom && A.st_mbits != nullptr) ? A.st_mbits + (size_t)tile_idx * kMbStride : nullptr;
            [[maybe_unused]] const size_t te_st_step = (size_t)A.P * W, te_mb_step = (size_t)A.n_tiles * kMbStride;
            load_bias<C::NTW>(tl_cur, wave, kWv, wp, bias_n);
            // ---- 2. positional encoding of the tile into act[:, 0:64)   (HLP:42-51, RUN:70-71)
            encode_tile<MODE, LD, PREC, kThr>(act, rowinfo, A.x, p0, rows_valid, ic, icv);
            // gamma(p) is needed again at the skip layer, five layers later, when the in-place tile has long been overwritten.
            // Re-evaluating it there cost ~800 vector instructions per wave and tile (30 correctly rounded sincosf per point);
            // instead the tile is parked as 16 KB of row-major fp32 - in the activation stash when there is one (the backward
            // wants it there anyway), else in this workgroup's slot of a small L2-resident scratch - and fetched back with
            // four 16-byte loads per thread.
            // The EVAL variants of the exact-fp32 path keep it in REGISTERS instead (16 per thread with 4 waves, 8 with 8): the scratch
            // slot was rewritten every tile and every one of those writes went through L2 to memory - 33 MB of WRITE_SIZE per C2
            // launch against 82 KB of outputs (profiles/r02_traffic.json).  (The split-bf16 eval kernel has no registers to spare and the
            // train variants want the tile in the stash anyway: they park it in memory as before.)
            constexpr bool kParkRegs = MODE == 0 && !TRAIN && PREC == PREC_F32;
            constexpr int kParkN = kTileM * 16 / kThr;
            f32x4 park[kParkRegs ? kParkN : 1];
            float* enc_park = (MODE == 0 && !kParkRegs) ? ((!kGeom && A.st_enc != nullptr) ? A.st_enc + p0 * 64 : A.enc_scratch + (size_t)blockIdx.x * (kTileM * 64)) : nullptr;
            if (kParkRegs) {
                __syncthreads();
#pragma unroll
                for (int i = 0; i < kParkN; ++i) {
                    const int idx = tid + i * kThr, row = idx >> 4, q = idx & 15;
                    park[i] = *reinterpret_cast<const f32x4*>(act + row * LD + 4 * q);
                }
            } else if (MODE == 0 || (!kGeom && A.st_enc != nullptr)) {
                __syncthreads();
                float* dst = (MODE == 0) ? enc_park : A.st_enc + p0 * 64;
                for (int idx = tid; idx < kTileM * 16; idx += kThr) {
                    const int row = idx >> 4, q = idx & 15;
                    if (row < rows_valid) {
                        f32x4 v;
                        const float* src = act + row * LD;
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = act_load<PREC>(src, LD, 4 * q + c);
                        if (!kGeom && A.st_enc != nullptr) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + row * 64 + 4 * q));
                        else *reinterpret_cast<f32x4*>(dst + row * 64 + 4 * q) = v;
                    }
                }
            }
            __syncthreads();
            // ---- 3. trunk: D x (Linear + ReLU), skip concat after layer D/2   (MOD:168-172)
            for (int l = 0; l < Dn; ++l) {
                CFN_PHASE_ARGS;
                f32x16 acc[2][C::NTW];
                const SubL tl_nn = kload((l + 2 < Dn) ? T.trunk[l + 2] : (kGeom ? T.ha : T.ft));   // (in flight under this layer's MFMAs)
                acc_init(acc, bias_n);
                // the accumulators take the bias fetched a layer ago (its wait also drains the previous layer's stash stores: one counter);
                // only THEN is the next layer's bias requested - hoisted above that wait it would expose an L2 round trip per layer
                asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[0][C::NTW - 1][0]) : "memory");
                // next layer's / the feature head's (the h_alpha head adds its bias after the k-split sum: nothing to fetch behind the last layer)
                if (!kGeom || l + 1 < Dn) load_bias<C::NTW>(tl_nxt, wave, kWv, wp, bias_n);
                mma_any<C::NTW, PREC, 2>(acc, tl_cur, wave, kWv, wp, wp16, act, LD);
                // (all four dwords of the prefetched entry stay live to here: the fp32 kernels never read w16_off, and a dead destination
                // register of an s_load in flight gets reused at once - a write-after-write wait on the load that was meant to be hidden)
                asm volatile("" :: "s"(tl_nn.w16_off));
                if (l >= 1 && l - 1 == skip_l) {
                    __syncthreads();                 // every wave is done reading h_{l-1}
                    if (kParkRegs) {                 // act[:, 0:64) <- gamma(p) again, from the registers it was kept in
#pragma unroll
                        for (int i = 0; i < kParkN; ++i) {
                            const int idx = tid + i * kThr, row = idx >> 4, q = idx & 15;
                            *reinterpret_cast<f32x4*>(act + row * LD + 4 * q) = park[i];
                        }
                    } else if (MODE == 0) {          // ... or from where the tile was parked
                        for (int idx = tid; idx < kTileM * 16; idx += kThr) {
                            const int row = idx >> 4, q = idx & 15;
                            f32x4 v; v[0] = v[1] = v[2] = v[3] = 0.f;           // rows past a ragged tile: finite filler
                            // nt load: served by L2, never by this CU's L1 (the scratch slot is rewritten every tile)
                            if (row < rows_valid) v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(enc_park + row * 64 + 4 * q));
                            float* dstl = act + row * LD;
#pragma unroll
                            for (int c = 0; c < 4; ++c) act_store<PREC>(dstl, LD, 4 * q + c, v[c]);
                        }
                    } else {
                        encode_tile<MODE, LD, PREC, kThr>(act, rowinfo, A.x, p0, rows_valid, ic, icv);
                    }
                    __syncthreads();
                    mma_any<C::NTW, PREC, 2>(acc, tl_skip, wave, kWv, wp, wp16, act, LD);
                }
                __syncthreads();
                float* st = (te_st0 != nullptr) ? te_st0 + (size_t)l * te_st_step : nullptr;
                uint32_t* mb = (te_mb0 != nullptr) ? te_mb0 + (size_t)l * te_mb_step : nullptr;
                constexpr bool kRows = TRAIN && PREC == PREC_F32 && kStashFromLds && !Q4;      // stash by rows out of LDS (see stash_rows) ...
                store_tiles<C::NTW, ACT_RELU, PREC, TRAIN, TRAIN && !kRows, true, Q4>(acc, tl_cur, wave, kWv, wp, act, LD, 0, st, W, rows_valid, mb);      // ... or (Q4) as pieces from the registers
                __syncthreads();
                if (kRows && st != nullptr) stash_rows<W, kThr>(act, LD, st, rows_valid);
                tl_cur = tl_nxt; tl_nxt = tl_nn;
            }
