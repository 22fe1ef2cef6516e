// cfnerf_kscores.hip - k_scores_kernel: the K latent samples of a row scored as an ENSEMBLE, as one stateless launch over samples [M,K]
// (CFNERF_F_KSCORES in the white_bkgd argument of cfnerf_composite_fwd, include/cfnerf.h): the row sorted ascending, its quantiles, and -
// against a target y - the rank of y among the samples (the PIT) and the CRPS of the ensemble.
//
// Lane layout.  KP = the next power of two >= K.  KP <= 64: one lane per sample and 64 / KP rows side by side in a wave (row r of the wave
// in lanes [r KP, (r + 1) KP)); KP = 128: one row per wave, two samples per lane (virtual positions lane and lane + 64).  The KP - K pad
// positions sit IN FRONT of the row and hold -inf: NaN has to order after +inf (torch.sort), so a +inf pad behind the row would come to lie
// between the real samples and a NaN; a -inf pad ties with a real -inf only, which has the same 32 bits, so whichever of the two ends up in
// front, the K positions behind the pads hold a permutation of the row's bit patterns.  Order statistic p is at virtual position pad + p.
//
// Sort: the bitonic network, partner = position ^ J.  J = 1, 2 are DPP quad_perm moves, J = 4, 8, 16 ds_swizzle in bit-mask mode (no LDS
// memory, within 32 lanes), J = 32 ds_bpermute, J = 64 is the lane's own second register.  The exchange is compare-and-select under
// less(a, b) = a < b, or b is NaN and a is not: no min / max arithmetic touches a value; on a tie both lanes keep their own.
//
// Scores.  #below / #equal are popcounts of a wave ballot masked to the row's lanes.  The two sums of the CRPS go through the xor butterfly
// of the same moves (a fixed tree of depth log2 KP whatever the row's place in the wave; pads add 0):
//   A = (1/K) sum_k |x_k - y|,   B = (1/K^2) sum_{g<K-1} (g+1)(K-1-g) (x_(g+1) - x_(g)),   crps = A - B
// B is 1/(2K^2) sum_kl |x_k - x_l| written over the sorted gaps: non-negative terms only (the textbook sum_i (2i-K+1) x_(i) cancels).
// Quantile level (lo, frac): x_(lo) + frac (x_(hi) - x_(lo)), hi = min(lo + 1, K - 1); frac == 0 gives the order statistic's bits.
// A row with a NaN sample or a NaN target gets NaN quantiles / crps / pit and rank_code -1.  No atomics, no LDS memory, no reduction
// across rows: every output of a row depends on that row alone.
#include <hip/hip_runtime.h>

#include "cfnerf_device.h"
#include "cfnerf_kernels.h"

namespace cfnerf {

constexpr int kScoresMaxGrid = 1 << 20;

__device__ __forceinline__ bool ks_less(float a, float b) { return a < b || (b != b && a == a); }

// the value held by lane ^ J
template <int J>
__device__ __forceinline__ float ks_xor(float v, int lane) {
    const int b = __float_as_int(v);
    if constexpr (J == 1) return __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0xB1, 0xf, 0xf, false));        // quad_perm:[1,0,3,2]
    else if constexpr (J == 2) return __int_as_float(__builtin_amdgcn_update_dpp(b, b, 0x4E, 0xf, 0xf, false));   // quad_perm:[2,3,0,1]
    else if constexpr (J < 32) return __int_as_float(__builtin_amdgcn_ds_swizzle(b, (J << 10) | 0x1F));            // and 0x1f, or 0, xor J
    else return __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, b));
}

// one compare-exchange of the network at distance J < 64 inside merge size MS; `pos` = the element's virtual position in its row
template <int J, int MS>
__device__ __forceinline__ float ks_cx(float v, int pos, int lane) {
    const float o = ks_xor<J>(v, lane);
    const bool take_min = ((pos & J) == 0) == ((pos & MS) == 0);
    const bool sw = take_min ? ks_less(o, v) : ks_less(v, o);
    return sw ? o : v;
}

template <int KP, int MS, int J>
__device__ __forceinline__ void ks_merge(float (&v)[KP > 64 ? 2 : 1], int pos0, int lane) {
    if constexpr (J == 64) {                  // (MS = 128: ascending) the lane's own pair
        const float a = v[0], b = v[1];
        const bool sw = ks_less(b, a);
        v[0] = sw ? b : a;
        v[1] = sw ? a : b;
    } else {
        v[0] = ks_cx<J, MS>(v[0], pos0, lane);
        if constexpr (KP > 64) v[1] = ks_cx<J, MS>(v[1], pos0 + 64, lane);
    }
    if constexpr (J > 1) ks_merge<KP, MS, J / 2>(v, pos0, lane);
}
template <int KP, int MS>
__device__ __forceinline__ void ks_sort(float (&v)[KP > 64 ? 2 : 1], int pos0, int lane) {
    if constexpr (MS <= KP) {
        ks_merge<KP, MS, MS / 2>(v, pos0, lane);
        ks_sort<KP, MS * 2>(v, pos0, lane);
    }
}
// the sum over the LP lanes of a row, the same bits in each of them
template <int LP, int J = 1>
__device__ __forceinline__ float ks_row_sum(float v, int lane) {
    if constexpr (J < LP) {
        v = v + ks_xor<J>(v, lane);
        return ks_row_sum<LP, J * 2>(v, lane);
    } else {
        return v;
    }
}

template <int KP>
__global__ __launch_bounds__(kThreads)
void k_scores_kernel(const KScoresArgs a) {
    constexpr int E = KP > 64 ? 2 : 1;        // samples per lane
    constexpr int LP = KP > 64 ? 64 : KP;     // lanes per row
    constexpr int R = 64 / LP;                // rows per wave
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int K = a.K, pad = KP - K;
    const int r = lane / LP, j = lane % LP;   // row of the wave, virtual position of v[0]
    const int p0 = j - pad;                   // order statistic held after the sort (v[1]: p0 + 64); < 0: a pad
    const unsigned long long rmask = (LP == 64 ? ~0ull : ((1ull << LP) - 1ull)) << (r * LP);
    const float ninf = __int_as_float(0xff800000), qnan = __int_as_float(0x7fc00000);
    const int64_t nwaves = (a.M + R - 1) / R;

    for (int64_t w = (int64_t)blockIdx.x * kWaves + wave; w < nwaves; w += (int64_t)gridDim.x * kWaves) {      // (wave-uniform)
        const int64_t row = w * R + r;
        const bool live = row < a.M;
        const float* xr = a.samples + row * K;
        float v[E];
        v[0] = (live && p0 >= 0) ? xr[p0] : ninf;
        if constexpr (E == 2) v[1] = live ? xr[p0 + 64] : ninf;                  // (K >= 65: pad <= 63, the second register is never a pad)
        float y = 0.f;
        if (a.target != nullptr && live) y = a.target[row];

        // scores that need no order: before the sort
        bool bad = false;
        int code = 0;
        float sumA = 0.f;
        if (a.target != nullptr) {
            const bool ok0 = live && p0 >= 0;
            unsigned long long nn = __ballot(ok0 && v[0] != v[0]), lt = __ballot(ok0 && v[0] < y), eq = __ballot(ok0 && v[0] == y);
            int below = __popcll(lt & rmask), equal = __popcll(eq & rmask);
            float t = ok0 ? fabsf(v[0] - y) : 0.f;
            if constexpr (E == 2) {
                nn |= __ballot(live && v[1] != v[1]);
                below += __popcll(__ballot(live && v[1] < y));
                equal += __popcll(__ballot(live && v[1] == y));
                t = t + (live ? fabsf(v[1] - y) : 0.f);
            }
            bad = (nn & rmask) != 0 || y != y;
            code = bad ? -1 : 2 * below + equal;
            sumA = ks_row_sum<LP>(t, lane);
        } else {
            unsigned long long nn = __ballot(v[0] != v[0]);
            if constexpr (E == 2) nn |= __ballot(v[1] != v[1]);
            bad = (nn & rmask) != 0;
        }

        ks_sort<KP, 2>(v, j, lane);

        if (a.sorted != nullptr && live) {
            float* sr = a.sorted + row * K;
            if (p0 >= 0) sr[p0] = v[0];
            if constexpr (E == 2) sr[p0 + 64] = v[1];
        }

        if (a.quantiles != nullptr) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                if (t < a.Q) {                                                   // (uniform)
                    const int lo = a.level_lo[t], hi = min(lo + 1, K - 1);
                    const float fr = a.level_frac[t];
                    const int ilo = pad + lo, ihi = pad + hi;                    // virtual positions in the row
                    float xa, xb;
                    if constexpr (E == 1) {
                        xa = __int_as_float(__builtin_amdgcn_ds_bpermute((r * LP + ilo) << 2, __float_as_int(v[0])));
                        xb = __int_as_float(__builtin_amdgcn_ds_bpermute((r * LP + ihi) << 2, __float_as_int(v[0])));
                    } else {
                        const float a0 = __int_as_float(__builtin_amdgcn_ds_bpermute((ilo & 63) << 2, __float_as_int(v[0])));
                        const float a1 = __int_as_float(__builtin_amdgcn_ds_bpermute((ilo & 63) << 2, __float_as_int(v[1])));
                        const float b0 = __int_as_float(__builtin_amdgcn_ds_bpermute((ihi & 63) << 2, __float_as_int(v[0])));
                        const float b1 = __int_as_float(__builtin_amdgcn_ds_bpermute((ihi & 63) << 2, __float_as_int(v[1])));
                        xa = ilo < 64 ? a0 : a1;
                        xb = ihi < 64 ? b0 : b1;
                    }
                    float q = fr == 0.f ? xa : xa + fr * (xb - xa);
                    if (bad) q = qnan;
                    if (live && j == 0) a.quantiles[row * a.Q + t] = q;
                }
            }
        }

        if (a.target != nullptr) {
            if (a.crps != nullptr) {
                // the gap above this lane's order statistic, weighted: (p + 1)(K - 1 - p) (x_(p+1) - x_(p)), p in [0, K-2]
                const int nl = ((lane + 1) & 63) << 2;
                const float n0 = __int_as_float(__builtin_amdgcn_ds_bpermute(nl, __float_as_int(v[0])));
                float g;
                if constexpr (E == 1) {
                    g = (p0 >= 0 && p0 <= K - 2) ? (float)((p0 + 1) * (K - 1 - p0)) * (n0 - v[0]) : 0.f;
                } else {
                    const float n1 = __int_as_float(__builtin_amdgcn_ds_bpermute(nl, __float_as_int(v[1])));      // (lane 63 reads lane 0's)
                    const float up0 = lane == 63 ? n1 : n0;
                    const int p1 = p0 + 64;
                    g = (p0 >= 0 && p0 <= K - 2) ? (float)((p0 + 1) * (K - 1 - p0)) * (up0 - v[0]) : 0.f;
                    g = g + (p1 <= K - 2 ? (float)((p1 + 1) * (K - 1 - p1)) * (n1 - v[1]) : 0.f);
                }
                const float sumB = ks_row_sum<LP>(g, lane);
                const float fk = (float)K;
                const float c = bad ? qnan : __fdiv_rn(sumA, fk) - __fdiv_rn(sumB, fk * fk);
                if (live && j == 0) a.crps[row] = c;
            }
            if (live && j == 0) {
                if (a.rank_code != nullptr) a.rank_code[row] = code;
                if (a.pit != nullptr) a.pit[row] = bad ? qnan : __fdiv_rn((float)code, (float)(2 * K));
            }
        }
    }
}

template <int KP>
static hipError_t ks_launch(const KScoresArgs& a, hipStream_t st) {
    const int R = KP > 64 ? 1 : 64 / KP;
    const int64_t nwaves = (a.M + R - 1) / R;
    const int grid = (int)std::min<int64_t>((nwaves + kWaves - 1) / kWaves, kScoresMaxGrid);
    hipLaunchKernelGGL(k_scores_kernel<KP>, dim3(grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_k_scores(const KScoresArgs& a, hipStream_t st) {
    if (a.M == 0) return hipSuccess;
    const int K = a.K;
    if (K <= 1) return ks_launch<1>(a, st);
    if (K <= 2) return ks_launch<2>(a, st);
    if (K <= 4) return ks_launch<4>(a, st);
    if (K <= 8) return ks_launch<8>(a, st);
    if (K <= 16) return ks_launch<16>(a, st);
    if (K <= 32) return ks_launch<32>(a, st);
    if (K <= 64) return ks_launch<64>(a, st);
    return ks_launch<128>(a, st);
}

}  // namespace cfnerf
