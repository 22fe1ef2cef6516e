// cfnerf_tail.hip - the flow-adjoint kernels of the train step for gfx950, a translation unit of their own:
//   tail_bwd_kernel   (fused path)   adjoint of raw2outputs (RUN:424-452) + of the K conditional flows (FLW:225-268, MOD:263-286)
//   tail_cot_kernel   (fused path, CFNERF_F_COTANGENTS with a cotangent for disp_map, weights or raw) the same body (cfnerf_tail_body.h) + those three
//   flows_bwd_kernel  (unfused seam) adjoint of the K flows + entropy terms of NeRF_Flows.forward (MOD:225-291) given d loss / d raw
//   tail_eps_kernel, flows_eps_kernel, reduce_eps_kernel (CFNERF_F_EPS_GRAD) the two bodies + d loss / d eps per ray / point, and its sum
// Both are long straight-line scalar code (the unrolled adjoint of four 3 x 3 triangular flow steps per (sample, latent)) on one wave per
// SIMD.  This file is compiled with -fno-slp-vectorize (cf-nerf_amd/build.py): left on, the SLP vectoriser pairs the arithmetic into
// v_pk_mul / v_pk_add / v_pk_fma and then needs ~200 v_mov per (chunk, latent) to line the operands up in register pairs; that pushes the
// tail kernel to 367 ArchVGPRs + 111 AccVGPRs with another ~230 v_accvgpr moves between the two files (a vector instruction addresses
// only the first 256).  Without it: 255 VGPRs, no AccVGPR, 1 193 -> 1 103 vector instructions per (chunk, latent): -8.5 % at K = 64
// (0.280 -> 0.256 ms), -0.7 % at K = 4 (round 4, tools/ab_kernels.sh).  The rest of the backward keeps the vectoriser: switched off for
// the whole of cfnerf_bwd.hip the weight-gradient kernels ran 0.5 % slower.
#include "cfnerf_device.h"
#include "cfnerf_kernels.h"
#include "cfnerf_model.h"
#include "cfnerf_bwd.h"

namespace cfnerf {

// ================================================================================================
// 2. tail: adjoint of raw2outputs (RUN:424-452) and of the K flows (FLW:225-268, MOD:263-286).
//    One wave per ray, lane = sample, chunks of 64 samples walked back-to-front so the transmittance
//    adjoint (comp_adjoint_D, cfnerf_device.h) is a reverse wave scan + a per-k carry.
// Adjoint of the four conditional Sylvester flows (FLW:225-268, MOD:401-413) for ONE (point, latent sample): recomputes the
// forward keeping each step's input and tanh, then walks it backwards.  In: th = the point's flow parameters, e = the latent,
// ga / gz = d loss / d (alpha, rgb) flow outputs (activation and entropy-Jacobian terms already added), cE = the weight of the
// log-det terms (- d_entropy / (P K)).  Accumulates d loss / d theta into gth and the base-Gaussian terms into gms.  Shared by
// the fused tail kernel and the unfused flows_bwd_kernel, so both differentiate with the same arithmetic.
template <class GACC>
__device__ __forceinline__ void flows_adjoint(const float (&th)[84], GACC& gth, float (&gms)[8], const f32x4 e, const float a_mean,
                                              const float a_std, const float (&r_mean)[3], const float (&r_std)[3], float ga, float (&gz)[3],
                                              const float cE, const bool valid) {
#pragma clang fp contract(fast)      // gradient arithmetic: a*b + c may fuse (the library is built with -ffp-contract=off for the FORWARD's
                                     // parity with torch's separate ops; the backward has no such constraint and fused pairs halve its
                                     // multiply / add instruction count)
    // ---- recompute the flows, keeping each step's input and tanh
    float zin[4][3], tt[4][3], ain[4], ta[4];
    float z[3] = {e[0] * r_std[0] + r_mean[0], e[1] * r_std[1] + r_mean[1], e[2] * r_std[2] + r_mean[2]};
    float a = e[3] * a_std + a_mean;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const bool odd = f & 1;
        zin[f][0] = z[0]; zin[f][1] = z[1]; zin[f][2] = z[2]; ain[f] = a;
        const float zp0 = odd ? z[2] : z[0], zp1 = z[1], zp2 = odd ? z[0] : z[2];
        const float pre0 = ((th[48 + f] * zp0 + th[(1 * 3 + 0) * 4 + f] * zp1) + th[(2 * 3 + 0) * 4 + f] * zp2) + th[60 + f];
        const float pre1 = (th[52 + f] * zp1 + th[(2 * 3 + 1) * 4 + f] * zp2) + th[64 + f];
        const float pre2 = th[56 + f] * zp2 + th[68 + f];
        const float t0 = t_tanh(pre0), t1 = t_tanh(pre1), t2 = t_tanh(pre2);
        tt[f][0] = t0; tt[f][1] = t1; tt[f][2] = t2;
        const float u0 = (th[36 + f] * t0 + th[(0 * 3 + 1) * 4 + f] * t1) + th[(0 * 3 + 2) * 4 + f] * t2;
        const float u1 = th[40 + f] * t1 + th[(1 * 3 + 2) * 4 + f] * t2;
        const float u2 = th[44 + f] * t2;
        z[0] = (odd ? u2 : u0) + z[0]; z[1] = u1 + z[1]; z[2] = (odd ? u0 : u2) + z[2];
        ta[f] = t_tanh(th[76 + f] * a + th[80 + f]);
        a = th[72 + f] * ta[f] + a;
    }
    // ---- adjoint, last flow first
#pragma unroll
    for (int f = 3; f >= 0; --f) {
        const bool odd = f & 1;
        const float zp0 = odd ? zin[f][2] : zin[f][0], zp1 = zin[f][1], zp2 = odd ? zin[f][0] : zin[f][2];
        const float t0 = tt[f][0], t1 = tt[f][1], t2 = tt[f][2];
        const float d1_0 = th[36 + f], d1_1 = th[40 + f], d1_2 = th[44 + f];
        const float d2_0 = th[48 + f], d2_1 = th[52 + f], d2_2 = th[56 + f];
        const float gu0 = odd ? gz[2] : gz[0], gu1 = gz[1], gu2 = odd ? gz[0] : gz[2];   // u = flip(z-update)
        // u_i = sum_{j>=i} R1[i][j] t_j
        float gt0 = d1_0 * gu0;
        float gt1 = th[(0 * 3 + 1) * 4 + f] * gu0 + d1_1 * gu1;
        float gt2 = th[(0 * 3 + 2) * 4 + f] * gu0 + th[(1 * 3 + 2) * 4 + f] * gu1 + d1_2 * gu2;
        gth.add(36 + f, gu0 * t0); gth.add(40 + f, gu1 * t1); gth.add(44 + f, gu2 * t2);
        gth.add((0 * 3 + 1) * 4 + f, gu0 * t1); gth.add((0 * 3 + 2) * 4 + f, gu0 * t2); gth.add((1 * 3 + 2) * 4 + f, gu1 * t2);
        // log-det: ld_i = log(|q_i| + 1e-8), q_i = (1 - t_i^2) d1_i d2_i + 1     (FLW:251-259)
        if (cE != 0.f && valid) {
            // q = 1 + (1 - t^2) d1 d2 >= t^2 >= 0: the diagonals are tanh outputs (|d| <= 1, MOD:341-348), so |q| = q and sign(q) = +1 - the abs / copysign
            // of FLW:255 are the identity here (the forward keeps them: libm parity)
            const float q0 = (1.f - t0 * t0) * (d1_0 * d2_0) + 1.f, q1 = (1.f - t1 * t1) * (d1_1 * d2_1) + 1.f,
                        q2 = (1.f - t2 * t2) * (d1_2 * d2_2) + 1.f;
            const float gq0 = cE * t_rcp(q0 + 1e-08f), gq1 = cE * t_rcp(q1 + 1e-08f), gq2 = cE * t_rcp(q2 + 1e-08f);
            gt0 += gq0 * (-2.f * t0 * d1_0 * d2_0); gt1 += gq1 * (-2.f * t1 * d1_1 * d2_1); gt2 += gq2 * (-2.f * t2 * d1_2 * d2_2);
            gth.add(36 + f, gq0 * (1.f - t0 * t0) * d2_0); gth.add(40 + f, gq1 * (1.f - t1 * t1) * d2_1); gth.add(44 + f, gq2 * (1.f - t2 * t2) * d2_2);
            gth.add(48 + f, gq0 * (1.f - t0 * t0) * d1_0); gth.add(52 + f, gq1 * (1.f - t1 * t1) * d1_1); gth.add(56 + f, gq2 * (1.f - t2 * t2) * d1_2);
        }
        const float gp0 = gt0 * (1.f - t0 * t0), gp1 = gt1 * (1.f - t1 * t1), gp2 = gt2 * (1.f - t2 * t2);
        gth.add(60 + f, gp0); gth.add(64 + f, gp1); gth.add(68 + f, gp2);                         // b
        // pre_i = sum_{j>=i} R2[i][j] zp_j,  R2[i][i] = d2_i,  R2[i][j>i] = D[j][i]
        gth.add(48 + f, gp0 * zp0); gth.add(52 + f, gp1 * zp1); gth.add(56 + f, gp2 * zp2);
        gth.add((1 * 3 + 0) * 4 + f, gp0 * zp1); gth.add((2 * 3 + 0) * 4 + f, gp0 * zp2); gth.add((2 * 3 + 1) * 4 + f, gp1 * zp2);
        const float gzp0 = d2_0 * gp0;
        const float gzp1 = th[(1 * 3 + 0) * 4 + f] * gp0 + d2_1 * gp1;
        const float gzp2 = th[(2 * 3 + 0) * 4 + f] * gp0 + th[(2 * 3 + 1) * 4 + f] * gp1 + d2_2 * gp2;
        gz[0] += odd ? gzp2 : gzp0; gz[1] += gzp1; gz[2] += odd ? gzp0 : gzp2;
        // alpha: a' = a + d1 tanh(d2 a + b)
        {
            const float d1 = th[72 + f], d2 = th[76 + f], tav = ta[f], ai = ain[f];
            float gta = ga * d1;
            gth.add(72 + f, ga * tav);
            if (cE != 0.f && valid) {
                const float q = (1.f - tav * tav) * (d1 * d2) + 1.f;          // >= 0, see above
                const float gq = cE * t_rcp(q + 1e-08f);
                gta += gq * (-2.f * tav * d1 * d2);
                gth.add(72 + f, gq * (1.f - tav * tav) * d2);
                gth.add(76 + f, gq * (1.f - tav * tav) * d1);
            }
            const float gpa = gta * (1.f - tav * tav);
            gth.add(80 + f, gpa);
            gth.add(76 + f, gpa * ai);
            ga += gpa * d2;
        }
    }
    // base sample z0 = eps * std + mean  (MOD:239,251)
    gms[0] += ga; gms[1] += ga * e[3];
    gms[2] += gz[0]; gms[3] += gz[1]; gms[4] += gz[2];
    gms[5] += gz[0] * e[0]; gms[6] += gz[1] * e[1]; gms[7] += gz[2] * e[2];
}

// Where the adjoint accumulates d loss / d theta of the current point over the latent samples: 84 registers per lane.
// (Round 3 tried LDS instead - one float per (entry, wave, lane), accumulated with ds_add_f32, to take 84 registers and the ~500
// v_mov / v_accvgpr moves they cause per (chunk, latent) out of the fused tail kernel: the vector-instruction count fell from 1 329 to
// 1 011, and the kernel took 333 us instead of 64 - LDS atomics run at a fraction of the plain LDS rate.  Not kept.)
struct GReg {
    float g[84];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 84; ++i) g[i] = 0.f;
    }
    __device__ __forceinline__ void add(int i, float v) {
#pragma clang fp contract(fast)      // the add must carry the flag too, or `g[i] += a * b` of flows_adjoint stays a v_mul + v_add pair (round 4: it did)
        g[i] += v;
    }
    __device__ __forceinline__ float get(int i) const { return g[i]; }
};
// One row of d loss / d theta (the pre-activation outputs of the flow-parameter heads), in the [P,128] layout of theta:
// the diagonals were tanh-ed (MOD:341-348), the padding columns are written as zeros (the weight-gradient GEMM reads them).
template <class GACC>
__device__ __forceinline__ void store_gtheta_row(float* __restrict__ row, const float (&th)[84], const GACC& gth) {
    // element i of the row: the diagonals (36..59, 72..79) chain through their tanh
    auto val = [&](int i) { const float g = gth.get(i); return ((i >= 36 && i < 60) || (i >= 72 && i < 80)) ? g * (1.f - th[i] * th[i]) : g; };
    f32x4* gp = reinterpret_cast<f32x4*>(row);
#pragma unroll
    for (int q = 0; q < 18; ++q) { f32x4 v; v[0] = val(q * 4); v[1] = val(q * 4 + 1); v[2] = val(q * 4 + 2); v[3] = val(q * 4 + 3); gp[q] = v; }
    f32x4 zero; zero[0] = zero[1] = zero[2] = zero[3] = 0.f;
#pragma unroll
    for (int q = 18; q < 24; ++q) gp[q] = zero;
#pragma unroll
    for (int q = 0; q < 3; ++q) { f32x4 v; v[0] = val(72 + q * 4); v[1] = val(73 + q * 4); v[2] = val(74 + q * 4); v[3] = val(75 + q * 4); gp[24 + q] = v; }
#pragma unroll
    for (int q = 27; q < 32; ++q) gp[q] = zero;
}

// (two workgroups per CU = two waves per SIMD: tail_parts (cfnerf_model.h) counts on it for K >= 64; the kernel needs 255 registers
// without the SLP vectoriser - tests/test_abi_cpu.py checks the built code object for spills)
__global__ __launch_bounds__(kThreads, 2)
void tail_bwd_kernel(const TailArgs A) {
#define CFN_TAIL_COT 0
#define CFN_TAIL_EPS 0
#include "cfnerf_tail_body.h"
#undef CFN_TAIL_EPS
#undef CFN_TAIL_COT
}

// (the same two workgroups per CU: 74 752 B of LDS with the 4 KB of `cot`, and no more registers than the plain body - tools/kernel_regs.py)
__global__ __launch_bounds__(kThreads, 2)
void tail_cot_kernel(const TailArgs A, const TailCot C) {
#define CFN_TAIL_COT 1
#define CFN_TAIL_EPS 0
#include "cfnerf_tail_body.h"
#undef CFN_TAIL_EPS
#undef CFN_TAIL_COT
}

// CFNERF_F_EPS_GRAD: the cotangent body for this ray's rows of d loss / d eps alone, launched beside one of the two kernels above (an opt-in
// launch, not the train step's); the merge rows are dead here, so its LDS is carry + cot + the 8 KB of `epsg`; no scratch (tools/kernel_regs.py)
__global__ __launch_bounds__(kThreads, 2)
void tail_eps_kernel(const TailArgs A, const TailCot C, const TailEps E) {
#define CFN_TAIL_COT 1
#define CFN_TAIL_EPS 1
#include "cfnerf_tail_body.h"
#undef CFN_TAIL_EPS
#undef CFN_TAIL_COT
}

// ------------------------------------------------------------------------------------------------
// 2b. The UNFUSED seam (the reference's NeRF_Flows.forward and raw2outputs are separately differentiable, so a caller-supplied
//     network_query_fn trains): the tail kernel's two halves as standalone kernels with the same arithmetic.
//
// flows_bwd_kernel: adjoint of the K flows + the entropy terms of NeRF_Flows.forward (MOD:225-291) given d loss / d raw [P,K,4].
// lane = point; every latent of a point in one lane, so g_theta needs no partial sums.
__global__ __launch_bounds__(kThreads)
void flows_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ theta, const float* __restrict__ eps, int eps_rows,
                      const float* __restrict__ flat, const float* __restrict__ d_raw, const float* __restrict__ d_ent, int64_t P, int K,
                      float* __restrict__ g_theta, float* __restrict__ gms_partials) {
#define CFN_FLOWS_EPS 0
#include "cfnerf_flows_bwd_body.h"
#undef CFN_FLOWS_EPS
}

// CFNERF_F_EPS_GRAD of a points stash, launched beside flows_bwd_kernel: the same body for the point's [K,4] row of d loss / d eps alone, into
// eps_out [P,K,4] (16-byte stores, one per latent); g_theta / gms_partials are not written
__global__ __launch_bounds__(kThreads)
void flows_eps_kernel(const float* __restrict__ raw, const float* __restrict__ theta, const float* __restrict__ eps, int eps_rows,
                      const float* __restrict__ flat, const float* __restrict__ d_raw, const float* __restrict__ d_ent, int64_t P, int K,
                      float* __restrict__ g_theta, float* __restrict__ gms_partials, float* __restrict__ eps_out) {
#define CFN_FLOWS_EPS 1
#include "cfnerf_flows_bwd_body.h"
#undef CFN_FLOWS_EPS
}

// d_eps [K,4] = the sum of d_eps_rows [n,K,4] over its n rows (rays of a fused launch, points of a seam launch) in a fixed order: one
// workgroup per latent, double accumulators, rounded once - like reduce_gms_kernel.  The rows already hold the base log-normal's direct
// term (each its own share of it), so it enters the sum exactly once.
__global__ __launch_bounds__(256)
void reduce_eps_kernel(const float* __restrict__ rows, int64_t n, int K, float* __restrict__ d_eps) {
    __shared__ double sh[4][256];
    const int k = blockIdx.x;
    double s[4] = {0, 0, 0, 0};
    for (int64_t r = threadIdx.x; r < n; r += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(rows + (r * K + k) * 4);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    for (int i = 0; i < 4; ++i) sh[i][threadIdx.x] = s[i];
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) for (int i = 0; i < 4; ++i) sh[i][threadIdx.x] += sh[i][threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x < 4) d_eps[k * 4 + threadIdx.x] = (float)sh[threadIdx.x][0];
}


// ---- host launchers (cfnerf_bwd.h)
hipError_t launch_tail_bwd(const TailArgs& ta, const TailCot& cot, const TailEps& eg, int64_t n_rays, int ksplit, hipStream_t st) {
    const dim3 grid((unsigned)((n_rays * ksplit + kWaves - 1) / kWaves));
    if (eg.rows != nullptr) hipLaunchKernelGGL(tail_eps_kernel, grid, dim3(kThreads), 0, st, ta, cot, eg);      // (CFNERF_F_EPS_GRAD: beside the launch below, cotangents or not)
    if (cot.any()) hipLaunchKernelGGL(tail_cot_kernel, grid, dim3(kThreads), 0, st, ta, cot);
    else hipLaunchKernelGGL(tail_bwd_kernel, grid, dim3(kThreads), 0, st, ta);
    return hipGetLastError();
}

hipError_t launch_flows_bwd(const float* raw, const float* theta, const float* eps, int eps_rows, const float* flat, const float* d_raw,
                            const float* d_ent, int64_t P, int K, float* g_theta, float* gms_partials, float* eps_out, unsigned* grid_out,
                            hipStream_t st) {
    const unsigned grid = (unsigned)((P + kThreads - 1) / kThreads);
    if (grid_out) *grid_out = grid;
    if (eps_out != nullptr)                                  // CFNERF_F_EPS_GRAD: beside the launch below
        hipLaunchKernelGGL(flows_eps_kernel, dim3(grid), dim3(kThreads), 0, st, raw, theta, eps, eps_rows, flat, d_raw, d_ent, P, K, g_theta,
                           gms_partials, eps_out);
    hipLaunchKernelGGL(flows_bwd_kernel, dim3(grid), dim3(kThreads), 0, st, raw, theta, eps, eps_rows, flat, d_raw, d_ent, P, K, g_theta,
                       gms_partials);
    return hipGetLastError();
}

hipError_t launch_reduce_eps(const float* rows, int64_t n, int K, float* d_eps, hipStream_t st) {
    hipLaunchKernelGGL(reduce_eps_kernel, dim3((unsigned)K), dim3(256), 0, st, rows, n, K, d_eps);
    return hipGetLastError();
}

}  // namespace cfnerf
