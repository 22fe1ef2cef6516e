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
#include "cfnerf_igmma.h"

namespace cfnerf {

template <int W>
__global__ __launch_bounds__(kThreads, 3)      // three workgroups per CU (168 registers, 3 x 40 KB of LDS; at four it spills): a streaming kernel lives on loads in flight
void input_grad_kernel(const InputGradArgs A) {
    __shared__ __attribute__((aligned(16))) float As[kTileM * kIgLdA];
    __shared__ __attribute__((aligned(16))) float Bs[kIgKs * kIgLdB];
    __shared__ __attribute__((aligned(16))) float Xs[kTileM * kIgMaxX];      // the tile's d_x rows as they lie in memory (row stride ic + icv)
    const int tid = threadIdx.x;
    const int xs = A.ic + A.icv;
    const int cpr = (A.S + kTileM - 1) / kTileM;                 // chunks per ray: the forward's tiling (points: ONE ray of S = P samples)

    for (int64_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const int64_t ray = tile / cpr;
        const int chunk = (int)(tile - ray * cpr);
        const int64_t p0 = ray * (int64_t)A.S + (int64_t)chunk * kTileM;
        const int rows_valid = min(kTileM, A.S - chunk * kTileM);
        ig_tile_mma<W>(A, p0, rows_valid, As, Bs, Xs);      // (cfnerf_igmma.h)
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
