// cfnerf_fwd_halpha_body.h - the k-split partial sum of the h_alpha head (MOD:175) in fused_fwd_kernel (CFN_FWD_GEOM 0) and geom_fwd_kernel
// (CFN_FWD_GEOM 1), included ONCE PER KERNEL behind the head's MFMAs; text for the reason given in cfnerf_fwd_trunk_body.h.  h_alpha is only
// 1-2 n-tiles wide: its K is split over the waves (mma_ksplit) and each wave arrives here with its raw fp32 partial tile in accA.  The
// partial tiles go through act[] once h is dead and are summed in ONE order - pp[0], q = 1 .. nparts-1, then the bias - into hs.
// Reads accA, s_ha and st_ha, the head's stash stream: a null constant in the geometry kernel, which has no stash.
                __syncthreads();                     // every wave is done reading h
                {
                    const int lo = lane_id_opaque();
                    float* lp = act + (4 * (lo >> 5)) * LD + 32 * wave + (lo & 31);      // raw fp32 partial of wave w: act[:, 32w..32w+32)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) lp[(i * 32 + (r & 3) + 8 * (r >> 2)) * LD] = accA[i][0][r];
                }
                __syncthreads();
                {
                    const int ntc = (int)s_ha.nt, nparts = kWv / ntc;
                    if (kThr % HA == 0) {
                        // (round 4) every thread owns ONE column (the thread count is a multiple of h_alpha_size: 32, 64, 128): its bias is
                        // fetched once, in front of the loop.  Element by element - `wp[b_off + c]` inside the loop - the compiler emitted
                        // global_load, s_waitcnt vmcnt(0), add, ds_write, store per element: a serialised L2 round trip (which also drains the
                        // previous element's stash store) 8 ... 32 times per tile, plus an integer division by the run-time HA each.
                        // Same element -> thread map, same order of the partial sums.
                        const int c = tid % HA, rstep = kThr / HA;
                        const float bc = wp[s_ha.b_off + c];
                        const float* pp0 = act + 32 * (c >> 5) + (c & 31);                   // wave w = part * ntc + n-tile
                        for (int row = tid / HA; row < kTileM; row += rstep) {
                            const float* pp = pp0 + row * LD;
                            float v = pp[0];
                            for (int q = 1; q < nparts; ++q) v += pp[32 * ntc * q];
                            v += bc;
                            act_store<PREC>(hs + row * HLD, HLD, c, v);
                            if (st_ha != nullptr && row < rows_valid) st_stream(st_ha + (p0 + row) * HA + c, v);
                        }
                    } else {
                        for (int idx = tid; idx < kTileM * HA; idx += kThr) {
                            const int row = idx / HA, c = idx - row * HA;
                            const float* pp = act + row * LD + 32 * (c >> 5) + (c & 31);
                            float v = pp[0];
                            for (int q = 1; q < nparts; ++q) v += pp[32 * ntc * q];
                            v += wp[s_ha.b_off + c];
                            act_store<PREC>(hs + row * HLD, HLD, c, v);
                            if (st_ha != nullptr && row < rows_valid) st_stream(st_ha + (p0 + row) * HA + c, v);
                        }
                    }
                }
                __syncthreads();
