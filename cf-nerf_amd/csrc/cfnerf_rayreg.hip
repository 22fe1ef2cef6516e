// cfnerf_rayreg.hip - ray_reg_kernel: the two ray regularisers of few-view training, as ONE stateless launch over the composite's
// weights [N,S,K] (CFNERF_F_RAY_REG in the white_bkgd argument of cfnerf_composite_fwd, include/cfnerf.h):
//   the distortion loss of mip-NeRF 360   D = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i
//   the ray entropy of InfoNeRF           H = - sum_i p_i log(p_i + 1e-10),  p = w / (sum w + 1e-10),  on rays with sum w > acc_min
// with their gradient in the weights (scaled: a cotangent for the composite's backward as it stands) and, optionally, the direct
// gradient in z_vals.  O(S) per (ray, latent): prefix sums along the ray.
//
// The distortion is evaluated in the Q/R form, sums of NON-NEGATIVE terms only:
//   Q_i = sum_{j<i}  W_{<=j} (m_{j+1} - m_j) = sum_{j<i} w_j (m_i - m_j)         a prefix scan of a prefix scan, front to back
//   R_i = sum_{j>=i} W_{>j}  (m_{j+1} - m_j) = sum_{j>i} w_j (m_j - m_i)         a suffix scan of a suffix scan, back to front
//   D = 2 sum_i w_i Q_i + 1/3 sum_i w_i^2 delta_i,     dD/dw_i = 2 (Q_i + R_i) + 2/3 w_i delta_i
// The textbook m_i W_{<i} - sum_{j<i} w_j m_j is a cancelling difference of two running sums, and a wave scan gives every lane its own
// summation tree: the lesson of comp_adjoint_D (cfnerf_device.h).  W_{>j} comes from its own suffix scan, not from A - W_{<=j}.
//
// One wave walks one ray, lane = sample, 64-sample chunks with the running sums of every latent carried in LDS (entry = latent).  A
// chunk's [64][K] block of weights is ONE contiguous span of memory: it is staged through LDS kRegKT latents at a time, read and
// written by consecutive lanes at consecutive addresses, and read transposed (lane = sample, pitch kRegKT + 1: conflict-free).
// Inside the walk of a tile's latents no fence is needed: a lane reads and writes its own slots of the tile, and entry k of the carries is
// read before it is written; the fences sit where lanes exchange data - around the staging and between chunks.
// A ray is walked up to three times (its block is L2-resident after the first):
//   1. front to back: A = sum w; Q, D; the Q half of dD/dw parked in d_weights
//   2. front to back (entropy or d_z wanted): H and sum_j p_j g_j, which need A; dD/dm, dD/ddelta summed over the latents -> d_z
//   3. back to front: R; d_weights = (parked half + R half) + the entropy's gradient
// A lambda of 0 skips that term's arithmetic (and pass 2 altogether when there is no d_z either).  Each product that enters the final sum
// is rounded on its own (no contraction), so a call with one lambda at 0 has the bits of the other term's gradient alone.
// The three loss sums leave as 64-bit fixed-point integer atomics (order-free: two runs give the same bits), like loss_partial_kernel;
// the workgroup that draws the last ticket turns them into {reg, dist, ent, frac}.
#include <hip/hip_runtime.h>

#include "cfnerf_device.h"
#include "cfnerf_kernels.h"

namespace cfnerf {

constexpr int kRegKT = 16;                    // latents of one staged tile (a sample's 64-byte segment)
constexpr int kRegPitch = kRegKT + 1;
constexpr int kRegMaxK = 128;
constexpr double kRegFix = 1099511627776.0;   // 2^40: resolution 9e-13 per workgroup partial, |sum| < 2^21 (checked: NaN beyond)
constexpr int kRegTicketShift = 44;           // accumulator 2: masked (ray, latent) pairs in the low 44 bits, workgroup tickets above
constexpr int kRegMaxGrid = 32768;

// stage rows [ch*64, ch*64+64) x latents [t0, t0+kt) of a ray's [S,K] block: consecutive lanes, consecutive addresses; rows past S are zeros.
// All of a lane's loads are issued before the first LDS write: with one wave per ray a tile costs one memory latency, not kt of them.
__device__ __forceinline__ void reg_stage_in(float* tile, const float* __restrict__ src, int ch, int t0, int kt, int S, int K, int lane) {
    if (kt == kRegKT) {                       // piece j: rows 4 j + lane / 16 of the chunk, latent t0 + lane % 16 - one base per lane, a uniform step per piece
        float v[kRegKT];
        const int sl0 = lane / kRegKT, q = lane % kRegKT, s0 = ch * 64 + sl0;
        const unsigned off = (unsigned)(s0 * K + t0 + q), step = (unsigned)(4 * K);      // (S K <= 2^19 floats per ray)
#pragma unroll
        for (int j = 0; j < kRegKT; ++j) v[j] = s0 + 4 * j < S ? src[off + j * step] : 0.f;
#pragma unroll
        for (int j = 0; j < kRegKT; ++j) tile[(sl0 + 4 * j) * kRegPitch + q] = v[j];
    } else {                                  // a narrower tile (K < 16, or the last of a K that is no multiple of 16): four pieces of 64 elements at a time
        for (int j0 = 0; j0 < kt; j0 += 4) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = (j0 + j) * 64 + lane, sl = e / kt, q = e - sl * kt, s = ch * 64 + sl;
                v[j] = (j0 + j < kt && s < S) ? src[(unsigned)(s * K + t0 + q)] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = (j0 + j) * 64 + lane, sl = e / kt;
                if (j0 + j < kt) tile[sl * kRegPitch + (e - sl * kt)] = v[j];
            }
        }
    }
}
__device__ __forceinline__ void reg_stage_out(const float* tile, float* __restrict__ dst, int ch, int t0, int kt, int S, int K, int lane) {
    if (kt == kRegKT) {
        const int sl0 = lane / kRegKT, q = lane % kRegKT, s0 = ch * 64 + sl0;
        const unsigned off = (unsigned)(s0 * K + t0 + q), step = (unsigned)(4 * K);
#pragma unroll
        for (int j = 0; j < kRegKT; ++j)
            if (s0 + 4 * j < S) dst[off + j * step] = tile[(sl0 + 4 * j) * kRegPitch + q];
    } else {
        for (int e = lane; e < 64 * kt; e += 64) {
            const int sl = e / kt, q = e - sl * kt, s = ch * 64 + sl;
            if (s < S) dst[(unsigned)(s * K + t0 + q)] = tile[sl * kRegPitch + q];
        }
    }
}

__global__ __launch_bounds__(kThreads)
void ray_reg_kernel(const RayRegArgs a) {
    __shared__ float tile_all[kWaves][2][64 * kRegPitch];
    __shared__ float car_all[kWaves][4][kRegMaxK];      // [0] A  [1], [2] running sums of the pass  [3] sum_j p_j g_j
    __shared__ double red_d[kWaves][2];
    __shared__ unsigned long long red_m[kWaves];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    float* tA = tile_all[wave][0];
    float* tB = tile_all[wave][1];
    float* cA = car_all[wave][0];
    float* c1 = car_all[wave][1];
    float* c2 = car_all[wave][2];
    float* cG = car_all[wave][3];
    const int S = a.S, K = a.K;
    const int nch = (S + 63) / 64;
    const bool do_d = a.cd != 0.f, do_e = a.ce != 0.f, want_z = a.dz != nullptr;
    double dsum = 0.0, hsum = 0.0;                       // this wave's rays: sum_k D, sum_k mask H
    unsigned long long msum = 0;                         // ... and masked (ray, latent) pairs

    for (int64_t ray = (int64_t)blockIdx.x * kWaves + wave; ray < a.N; ray += (int64_t)gridDim.x * kWaves) {
        const float* wr = a.w + ray * (int64_t)S * K;
        float* gr = a.dw + ray * (int64_t)S * K;
        const float* zr = a.z + ray * (int64_t)S;
        float nearv = 0.f, span = 1.f;
        if (a.rays != nullptr) { nearv = a.rays[ray * 11 + 6]; span = a.rays[ray * 11 + 7] - nearv; }
        // the geometry of this lane's sample in chunk ch: s, the interval's midpoint and width, the step to the next midpoint
        auto geometry = [&](int ch, float& m, float& dl, float& dmn) {
            const int s = ch * 64 + lane;
            m = 0.f; dl = 0.f; dmn = 0.f;
            if (s < S) {
                const float s0 = a.rays != nullptr ? (zr[s] - nearv) / span : zr[s];
                if (s == S - 1) { m = s0; }
                else {
                    const float s1 = a.rays != nullptr ? (zr[s + 1] - nearv) / span : zr[s + 1];
                    m = (s0 + s1) / 2.f; dl = s1 - s0;
                    float m1 = s1;
                    if (s + 1 < S - 1) { const float s2 = a.rays != nullptr ? (zr[s + 2] - nearv) / span : zr[s + 2]; m1 = (s1 + s2) / 2.f; }
                    dmn = m1 - m;
                }
            }
        };
        for (int k = lane; k < K; k += 64) { c1[k] = 0.f; c2[k] = 0.f; }
        wave_lds_turn();

        // ---- pass 1, front to back: A; Q and D; the Q half of the gradient parked in d_weights
        for (int ch = 0; ch < nch; ++ch) {
            float m, dl, dmn;
            geometry(ch, m, dl, dmn);
            for (int t0 = 0; t0 < K; t0 += kRegKT) {
                const int kt = min(K - t0, kRegKT);
                reg_stage_in(tA, wr, ch, t0, kt, S, K, lane);
                wave_lds_turn();
                for (int q = 0; q < kt; ++q) {
                    const int k = t0 + q;
                    const float w = tA[lane * kRegPitch + q];
                    const float Wi = wave_scan_add_dpp(w) + c1[k];           // W_{<=i}
                    float carQ = 0.f;
                    if (do_d) {
                        const float Ti = wave_scan_add_dpp(Wi * dmn);
                        carQ = c2[k];
                        const float Q = wave_prev_dpp(Ti, 0.f) + carQ;
                        dsum += (double)comp_sum(2.f * (w * Q) + (w * w) * dl / 3.f);
                        tA[lane * kRegPitch + q] = a.cd * (2.f * Q + (2.f / 3.f) * (w * dl));
                        carQ += wave_last(Ti);
                    }
                    const float carW = wave_last(Wi);
                    if (lane == 0) { c1[k] = carW; c2[k] = carQ; }
                }
                wave_lds_turn();
                if (do_d) reg_stage_out(tA, gr, ch, t0, kt, S, K, lane);
                wave_lds_turn();
            }
        }
        for (int k = lane; k < K; k += 64) {
            const float A = c1[k];
            cA[k] = A; c1[k] = 0.f; c2[k] = 0.f; cG[k] = 0.f;
            if (A > a.acc_min) ++msum;                    // (per lane: summed over the wave at the end)
        }
        wave_lds_turn();

        // ---- pass 2, front to back: the entropy's two sums (they need A); the direct gradient in the depths
        if (do_e || want_z) {
            float zcar = 0.f;                            // what the chunk in front hands this chunk's first sample
            for (int ch = 0; ch < nch; ++ch) {
                float m, dl, dmn;
                geometry(ch, m, dl, dmn);
                float dm = 0.f, dd = 0.f;                // dD/dm_i, dD/ddelta_i summed over the latents
                for (int t0 = 0; t0 < K; t0 += kRegKT) {
                    const int kt = min(K - t0, kRegKT);
                    reg_stage_in(tA, wr, ch, t0, kt, S, K, lane);
                    wave_lds_turn();
                    for (int q = 0; q < kt; ++q) {
                        const int k = t0 + q;
                        const float w = tA[lane * kRegPitch + q];
                        const float A = cA[k];
                        float carW = 0.f, carG = 0.f;
                        if (do_e) {
                            const float p = w / (A + 1e-10f);
                            const float lg = logf(p + 1e-10f);
                            const float g = -lg - p / (p + 1e-10f);
                            const float h = comp_sum(-(p * lg));
                            carG = cG[k] + comp_sum(p * g);
                            if (A > a.acc_min) hsum += (double)h;
                        }
                        if (want_z && do_d) {
                            const float Wi = wave_scan_add_dpp(w);
                            carW = c1[k];
                            const float Wlt = wave_prev_dpp(Wi, 0.f) + carW;           // W_{<i}
                            const float Wgt = A - (Wi + carW);                         // W_{>i}
                            dm += 2.f * w * (Wlt - Wgt);
                            dd += w * w / 3.f;
                            carW += wave_last(Wi);
                        }
                        if (lane == 0) { c1[k] = carW; cG[k] = carG; }
                    }
                    wave_lds_turn();
                }
                if (want_z) {
                    const int s = ch * 64 + lane;
                    const bool inner = s < S - 1;
                    const float own = inner ? dm / 2.f - dd : dm;                      // (the last sample is the point m = s)
                    const float next = inner ? dm / 2.f + dd : 0.f;
                    const float prev = wave_prev_dpp(next, zcar);
                    zcar = wave_last(next);
                    if (s < S) a.dz[ray * (int64_t)S + s] = do_d ? a.cd * ((own + prev) / span) : 0.f;
                }
            }
            for (int k = lane; k < K; k += 64) { c1[k] = 0.f; c2[k] = 0.f; }
            wave_lds_turn();
        }

        // ---- pass 3, back to front, lanes reversed (lane r holds sample 63 - r of the chunk): R; the gradient
        for (int ch = nch - 1; ch >= 0; --ch) {
            float m, dl, dmn;
            geometry(ch, m, dl, dmn);
            const float rdmn = __int_as_float(__builtin_amdgcn_ds_bpermute((63 - lane) * 4, __float_as_int(dmn)));
            const int rl = 63 - lane;
            for (int t0 = 0; t0 < K; t0 += kRegKT) {
                const int kt = min(K - t0, kRegKT);
                reg_stage_in(tA, wr, ch, t0, kt, S, K, lane);
                if (do_d) reg_stage_in(tB, gr, ch, t0, kt, S, K, lane);
                wave_lds_turn();
                for (int q = 0; q < kt; ++q) {
                    const int k = t0 + q;
                    const float w = tA[rl * kRegPitch + q];
                    float out = 0.f, carW = 0.f, carR = 0.f;
                    if (do_d) {
                        const float Si = wave_scan_add_dpp(w);
                        carW = c1[k];
                        const float Wgt = wave_prev_dpp(Si, 0.f) + carW;               // W_{>i}: the samples behind, later chunks included
                        const float Ri = wave_scan_add_dpp(Wgt * rdmn) + c2[k];
                        out = tB[rl * kRegPitch + q] + a.cd * (2.f * Ri);
                        carW += wave_last(Si);
                        carR = wave_last(Ri);
                    }
                    if (do_e) {
                        const float A = cA[k];
                        if (A > a.acc_min) {
                            const float p = w / (A + 1e-10f);
                            const float g = -logf(p + 1e-10f) - p / (p + 1e-10f);
                            out = out + a.ce * ((g - cG[k]) / (A + 1e-10f));
                        }
                    }
                    tB[rl * kRegPitch + q] = out;
                    if (lane == 0) { c1[k] = carW; c2[k] = carR; }
                }
                wave_lds_turn();
                reg_stage_out(tB, gr, ch, t0, kt, S, K, lane);
                wave_lds_turn();
            }
        }
    }

    // ---- the loss sums: wave -> workgroup -> 64-bit fixed-point atomics; the last ticket finalises
    for (int d = 32; d >= 1; d >>= 1) msum += __shfl_xor(msum, d, 64);
    if (lane == 0) { red_d[wave][0] = dsum; red_d[wave][1] = hsum; red_m[wave] = msum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double d0 = 0.0, d1 = 0.0;
        unsigned long long mm = 0;
        for (int i = 0; i < kWaves; ++i) { d0 += red_d[i][0]; d1 += red_d[i][1]; mm += red_m[i]; }
        // a NaN / inf / out-of-range partial must surface as NaN in the result, not as integer garbage: flag it in bit 62
        const bool bad0 = !(fabs(d0) < 2097152.0), bad1 = !(fabs(d1) < 2097152.0);
        unsigned long long* acc = a.acc;
        atomicAdd(acc + 0, bad0 ? (1ull << 62) : (unsigned long long)llrint(d0 * kRegFix));
        atomicAdd(acc + 1, bad1 ? (1ull << 62) : (unsigned long long)llrint(d1 * kRegFix));
        __threadfence();
        const unsigned long long old = atomicAdd(acc + 2, mm + (1ull << kRegTicketShift));
        if ((old >> kRegTicketShift) == (unsigned long long)gridDim.x - 1) {
            __threadfence();
            const long long a0 = (long long)atomicAdd(acc + 0, 0ull), a1 = (long long)atomicAdd(acc + 1, 0ull);
            const unsigned long long cnt = ((old + mm) & ((1ull << kRegTicketShift) - 1));
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            const double s0 = (a0 >= (1ll << 61) || a0 < -(1ll << 61)) ? nan : (double)a0 / kRegFix;
            const double s1 = (a1 >= (1ll << 61) || a1 < -(1ll << 61)) ? nan : (double)a1 / kRegFix;
            const double dist = s0 * a.inv, ent = s1 * a.inv, frac = (double)cnt * a.inv;
            float* o = a.scalars;                       // (the accumulators lie in bytes 8..31 of the same 32: read above, overwritten here)
            const float f_reg = (float)((double)a.lambda_dist * dist + (double)a.lambda_ent * ent);
            const float f_dist = (float)dist, f_ent = (float)ent, f_frac = (float)frac;
            o[0] = f_reg; o[1] = f_dist; o[2] = f_ent; o[3] = f_frac;
            o[4] = 0.f; o[5] = 0.f; o[6] = 0.f; o[7] = 0.f;
        }
    }
}

hipError_t launch_ray_reg(const RayRegArgs& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.scalars, 0, 8 * sizeof(float), st);
    if (e != hipSuccess || a.N == 0) return e;
    const int grid = (int)std::min<int64_t>((a.N + kWaves - 1) / kWaves, kRegMaxGrid);
    hipLaunchKernelGGL(ray_reg_kernel, dim3(grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace cfnerf
