// cfnerf_inputgrad.hip - d loss / d x of a cfnerf_network_fwd stash (CFNERF_F_INPUT_GRAD), launched by cfnerf_network_bwd after
// backward-data, when the pre-activation gradients g_h / g_v in the workspace are final.
//
// With x = [gamma(p) | gamma(d)], ic = input_ch, icv = input_ch_views (MOD:166-177):
//   d_x[:, :ic]       = g_h[0] . W_pts0  +  g_h[skip + 1] . W_pts(skip+1)[:, :ic]       (layer 0, then the layer fed by cat([input_pts, h]))
//   d_x[:, ic:ic+icv] = g_v . W_views0[:, W:W+icv]                                      (views_linears.0 over cat([feature, input_views]))
// One 64-point tile of the forward's tiling per workgroup iteration: a 64 x 64 output (pad of ic <= 63) accumulated over W twice - layer
// 0 first, then the skip layer, always in that order - and a 64 x 32 output (pad of icv <= 27) over W / 2.  Exact-fp32
// v_mfma_f32_32x32x2_f32 in both precision modes (the narrow GEMMs stay exact fp32 under bf16x3, cfnerf.h), no atomics: every d_x element
// is ONE lane's accumulator, so the result is bit-reproducible.  The kernel only READS the stash and the caller's flat parameters (nn.Linear
// [out, in] row-major: B[k = out][n = in] is a row of the weight, no packed operand needed); the parameter gradient does not see it.
#include <hip/hip_runtime.h>

#include "cfnerf_kernels.h"
#include "cfnerf_device.h"
#include "cfnerf_bwd.h"

namespace cfnerf {

constexpr int kIgKs = 32;               // k-slice of a stage: 32 units = ONE n-tile of a Q4 stream (cfnerf_device.h)
constexpr int kIgLdA = kIgKs + 4;       // A slice [64 rows][32 k]: +4 keeps the ds_read_b128 of 16 consecutive rows conflict-free (act_ld)
constexpr int kIgLdB = 64;              // B slice [32 k][64 input channels] (zero from ic / icv on)
constexpr int kIgMaxX = 64 + 32 - 6;    // ic + icv <= 63 + 27 (validate_cfg)

// slice s of a tile: [0, N0) layer 0, [N0, N0 + n1) the skip layer, then the views layer
struct IgSlice { const float* a; int C, nt, ld, ncols; uint32_t w; };

template <int W>
__global__ __launch_bounds__(kThreads, 3)      // three workgroups per CU (168 registers, 3 x 40 KB of LDS; at four it spills): a streaming kernel lives on loads in flight
void input_grad_kernel(const InputGradArgs A) {
    __shared__ __attribute__((aligned(16))) float As[kTileM * kIgLdA];
    __shared__ __attribute__((aligned(16))) float Bs[kIgKs * kIgLdB];
    __shared__ __attribute__((aligned(16))) float Xs[kTileM * kIgMaxX];      // the tile's d_x rows as they lie in memory (row stride ic + icv)
    constexpr int N0 = W / 32, NV = W / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int half = lane >> 5, l31 = lane & 31;
    const int ic = A.ic, icv = A.icv, xs = ic + icv;
    const int n1 = A.g_h1 ? N0 : 0, n_pts = N0 + n1, n_slices = n_pts + NV;
    const bool q4 = A.q4 != 0;
    const int cpr = (A.S + kTileM - 1) / kTileM;                 // chunks per ray: the forward's tiling (points: ONE ray of S = P samples)

    auto slice = [&](int s) {
        IgSlice r;
        if (s < N0)         { r.a = A.g_h0; r.C = W;     r.nt = s;         r.w = A.w0_off; r.ld = ic;     r.ncols = ic; }
        else if (s < n_pts) { r.a = A.g_h1; r.C = W;     r.nt = s - N0;    r.w = A.w1_off; r.ld = W + ic; r.ncols = ic; }
        else                { r.a = A.g_v;  r.C = W / 2; r.nt = s - n_pts; r.w = A.wv_off; r.ld = W + icv; r.ncols = icv; }
        return r;
    };

    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const int64_t ray = tile / cpr;
        const int chunk = (int)(tile - ray * cpr);
        const int64_t p0 = ray * (int64_t)A.S + (int64_t)chunk * kTileM;
        const int rows_valid = min(kTileM, A.S - chunk * kTileM);
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
        // rows [p0, p0 + rows_valid) of d_x are ONE contiguous piece: nothing past column ic + icv, nothing past row P
        {
            float* const dst = A.d_x + p0 * xs;
            const int count = rows_valid * xs;
            const int nq = ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) ? (count >> 2) : 0;
            for (int q = tid; q < nq; q += kThreads) *reinterpret_cast<f32x4*>(dst + 4 * q) = *reinterpret_cast<const f32x4*>(Xs + 4 * q);
            for (int t = nq * 4 + tid; t < count; t += kThreads) dst[t] = Xs[t];
        }
        // (the next tile's first write into Xs sits behind the barriers of its slices)
    }
}

static const void* input_grad_fn(int W) {
    switch (W) {
#define CFN_W_CASE(w) case w: return reinterpret_cast<const void*>(input_grad_kernel<w>);
        CFN_FOR_EACH_WIDTH(CFN_W_CASE)
#undef CFN_W_CASE
    }
    return nullptr;
}

hipError_t launch_input_grad(const InputGradArgs& a, int W, int n_cu, hipStream_t st) {
    const void* fn = input_grad_fn(W);
    if (!fn) return hipErrorInvalidValue;
    if (a.ic + a.icv > kIgMaxX) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>(a.n_tiles, (int64_t)n_cu * 3);      // three resident workgroups per CU (launch bounds)
    void* args[] = {const_cast<InputGradArgs*>(&a)};
    return hipLaunchKernel(fn, dim3(grid), dim3(kThreads), args, 0, st);
}

}  // namespace cfnerf
