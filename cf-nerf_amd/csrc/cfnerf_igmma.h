// cfnerf_igmma.h - the MFMA stage shared by input_grad_kernel (cfnerf_inputgrad.hip: d loss / d x of a points stash) and ray_grad_kernel
// (cfnerf_raygrad.hip: the same tile reduced to the ray).  One 64-point tile: d_x[:, :ic] = g_h[0] . W_pts0 + g_h[skip + 1] . W_skip[:, :ic] and
// d_x[:, ic:ic+icv] = g_v . W_views0[:, W:W+icv] on exact-fp32 v_mfma_f32_32x32x2_f32, left in LDS (Xs, row stride ic + icv).
#pragma once
#include <hip/hip_runtime.h>

#include "cfnerf_device.h"
#include "cfnerf_bwd.h"

namespace cfnerf {

constexpr int kIgKs = 32;               // k-slice of a stage: 32 units = ONE n-tile of a Q4 stream (cfnerf_device.h)
constexpr int kIgLdA = kIgKs + 4;       // A slice [64 rows][32 k]: +4 keeps the ds_read_b128 of 16 consecutive rows conflict-free (act_ld)
constexpr int kIgLdB = 64;              // B slice [32 k][64 input channels] (zero from ic / icv on)
constexpr int kIgMaxX = 64 + 32 - 6;    // ic + icv <= 63 + 27 (validate_cfg)

// slice s of a tile: [0, N0) layer 0, [N0, N0 + n1) the skip layer, then the views layer
struct IgSlice { const float* a; int C, nt, ld, ncols; uint32_t w; };

// the tile of points [p0, p0 + 64) (rows_valid of them exist) -> Xs; every thread of the workgroup calls it, Xs is readable on return
template <int W>
__device__ __forceinline__ void ig_tile_mma(const InputGradArgs& A, const int64_t p0, const int rows_valid, float* const As, float* const Bs, float* const Xs) {
    constexpr int N0 = W / 32, NV = W / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int half = lane >> 5, l31 = lane & 31;
    const int ic = A.ic, icv = A.icv, xs = ic + icv;
    const int n1 = A.g_h1 ? N0 : 0, n_pts = N0 + n1, n_slices = n_pts + NV;
    const bool q4 = A.q4 != 0;
    auto slice = [&](int s) {
        IgSlice r;
        if (s < N0)         { r.a = A.g_h0; r.C = W;     r.nt = s;         r.w = A.w0_off; r.ld = ic;     r.ncols = ic; }
        else if (s < n_pts) { r.a = A.g_h1; r.C = W;     r.nt = s - N0;    r.w = A.w1_off; r.ld = W + ic; r.ncols = ic; }
        else                { r.a = A.g_v;  r.C = W / 2; r.nt = s - n_pts; r.w = A.wv_off; r.ld = W + icv; r.ncols = icv; }
        return r;
    };
    f32x16 accP, accV;
#pragma unroll
    for (int r = 0; r < 16; ++r) accP[r] = accV[r] = 0.f;
    f32x4 ra[2];
    float rb[8];
    // global -> registers of slice s (issued one slice ahead of its use)
    auto fetch = [&](int s) {
        const IgSlice sl = slice(s);
        const float* const base = sl.a + p0 * sl.C;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (q4) {        // piece (half-tile j, n-tile nt, group g = wave): four consecutive rows of column l31 per lane
                ra[j] = *reinterpret_cast<const f32x4*>(base + ((j * (sl.C / 32) + sl.nt) * 4 + wave) * 256 + lane * 4);
            } else {
                const int idx = tid + j * kThreads, row = idx >> 3, kq = idx & 7;
                ra[j][0] = ra[j][1] = ra[j][2] = ra[j][3] = 0.f;      // rows past a ragged tile were never written
                if (row < rows_valid) ra[j] = *reinterpret_cast<const f32x4*>(base + (size_t)row * sl.C + sl.nt * kIgKs + kq * 4);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = tid + j * kThreads, k = idx >> 6, n = idx & 63;
            rb[j] = (n < sl.ncols) ? A.flat[(size_t)sl.w + (size_t)(sl.nt * kIgKs + k) * sl.ld + n] : 0.f;
        }
    };
    fetch(0);
#pragma unroll 1
    for (int s = 0; s < n_slices; ++s) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (q4) {
                const int row = 32 * j + 8 * wave + 4 * half;
#pragma unroll
                for (int e = 0; e < 4; ++e) As[(row + e) * kIgLdA + l31] = ra[j][e];
            } else {
                const int idx = tid + j * kThreads, row = idx >> 3, kq = idx & 7;
                *reinterpret_cast<f32x4*>(As + row * kIgLdA + kq * 4) = ra[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[tid + j * kThreads] = rb[j];          // (idx = k * 64 + n)
        __syncthreads();
        if (s + 1 < n_slices) fetch(s + 1);
        // d_pts: wave -> (row half wave >> 1, n-tile wave & 1); d_views: waves 0, 1 -> row half `wave`, the one n-tile
        auto mma = [&](f32x16& acc, int i, int ntc) {
#pragma unroll
            for (int k8 = 0; k8 < kIgKs / 8; ++k8) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(As + (32 * i + l31) * kIgLdA + k8 * 8 + 4 * half);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc = CFN_MFMA(a[c], Bs[(k8 * 8 + 4 * half + c) * kIgLdB + ntc * 32 + l31], acc);
            }
        };
        if (s < n_pts) mma(accP, wave >> 1, wave & 1);
        else if (wave < 2) mma(accV, wave, 0);
        __syncthreads();
    }
    // fragment element r of lane (l31, half): row (r & 3) + 8 (r >> 2) + 4 half of the 32-row half, column l31 of the n-tile
    {
        const int i = wave >> 1, col = (wave & 1) * 32 + l31;
        if (col < ic) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[(32 * i + (r & 3) + 8 * (r >> 2) + 4 * half) * xs + col] = accP[r];
        }
        if (wave < 2 && l31 < icv) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Xs[(32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half) * xs + ic + l31] = accV[r];
        }
    }
    __syncthreads();
}

}  // namespace cfnerf
