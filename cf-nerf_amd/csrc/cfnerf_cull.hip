// cfnerf_cull.hip - rendering through an occupancy grid (CFNERF_F_CULL, evaluation only), a translation unit of its own:
//   cull_kernel<false>        count pass: the kept samples of every ray
//   cull_scan_kernel          exclusive scan of the N counts (ray_start [N+1], ray_start[N] = P')
//   cull_kernel<true>         emit pass: z_vals, slot, the compact point list pts_c and ray_of
//   composite_sparse_kernel   raw2outputs on raw rows that exist for the kept samples only
// What is shared with the other kernels comes from the inline device functions of cfnerf_device.h and, for the composite, cfnerf_composite.h and the text of cfnerf_comp_fwd_body.h.
//
// Compaction is deterministic - (ray, sample) order, no atomics: one wave per ray with lane = sample as in sample_points_kernel, a
// 64-sample chunk's keep mask is one ballot, a lane's rank the popcount of the mask bits below it.
#include "cfnerf_device.h"
#include "cfnerf_composite.h"
#include "cfnerf_kernels.h"

namespace cfnerf {

// The cell of a coordinate: floorf((p - lo) * scale), inside iff 0 <= t < res.  Exactly this fp32 arithmetic (the library is built with
// -ffp-contract=off: subtract, multiply, floor) - tests/test_hip_cull.py restates it in torch and asks for agreement on cell faces too.
// A NaN fails both comparisons: outside.
__device__ __forceinline__ bool cull_cell(float p, float lo, float scale, int res, int& cell) {
    const float t = floorf((p - lo) * scale);
    const bool in = t >= 0.f && t < (float)res;
    cell = in ? (int)t : 0;
    return in;
}

// EMIT = false: ray_start[n] = kept samples of ray n.  EMIT = true (after the scan): everything else.
template <bool EMIT>
__global__ __launch_bounds__(kThreads)
void cull_kernel(const CullArgs A) {
    __shared__ float ps_all[kWaves][192];
    const int lane = lane_id();
    const int wave = wave_id();
    float* ps = ps_all[wave];
    const int S = A.S;
    const int nch = (S + 63) / 64;
    const bool lind = A.lindisp != 0;
    const float* __restrict__ t_vals = A.t_vals;
    const float* __restrict__ t_rand = A.t_rand;
    auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
    for (int64_t n = (int64_t)blockIdx.x * kWaves + wave; n < A.N; n += (int64_t)gridDim.x * kWaves) {     // (no workgroup barrier below)
        const float* r = A.rays + n * 11;
        const float o0 = uni(r[0]), o1 = uni(r[1]), o2 = uni(r[2]), d0 = uni(r[3]), d1 = uni(r[4]), d2 = uni(r[5]);
        const float nearv = uni(r[6]), farv = uni(r[7]);
        int64_t row0 = 0;                                    // first compact row of this chunk
        if (EMIT) row0 = A.ray_start[n];
        int kept = 0;
        for (int ch = 0; ch < nch; ++ch) {
            const int s = ch * 64 + lane;
            const bool valid = s < S;
            const float zv = strat_depth(t_vals, t_rand, n, S, min(s, S - 1), nearv, farv, lind);      // the depth of sample_points_kernel: its function
            const float p0 = o0 + d0 * zv, p1 = o1 + d1 * zv, p2 = o2 + d2 * zv;                          // RUN:534: the bits of `pts`
            int ix, iy, iz;
            const bool in0 = cull_cell(p0, A.lo[0], A.scale[0], A.res[0], ix);
            const bool in1 = cull_cell(p1, A.lo[1], A.scale[1], A.res[1], iy);
            const bool in2 = cull_cell(p2, A.lo[2], A.scale[2], A.res[2], iz);
            bool keep = A.outside == 0;
            if (in0 && in1 && in2) {                         // (the cell index is inside the grid: the word exists)
                const uint64_t cell = ((uint64_t)ix * (uint64_t)A.res[1] + (uint64_t)iy) * (uint64_t)A.res[2] + (uint64_t)iz;
                keep = (A.occ_bits[cell >> 5] >> (cell & 31)) & 1u;
            }
            keep = keep && valid;
            const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
            const int cnt = __popcll(mask);
            if (EMIT) {
                const int rank = __popcll(mask & ((1ull << lane) - 1ull));
                if (valid) {
                    A.z_vals[n * S + s] = zv;
                    A.slot[n * S + s] = keep ? (int32_t)(row0 + rank) : -1;
                }
                // the chunk's kept points, packed in LDS, leave as coalesced rows
                wave_lds_turn();
                if (keep) { ps[rank * 3 + 0] = p0; ps[rank * 3 + 1] = p1; ps[rank * 3 + 2] = p2; }
                wave_lds_turn();
                float* prow = A.pts_c + row0 * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int f = c * 64 + lane;
                    if (f < cnt * 3) prow[f] = ps[f];
                }
                if (lane < cnt) A.ray_of[row0 + lane] = (int32_t)n;
                row0 += cnt;
            }
            kept += cnt;
        }
        if (!EMIT && lane == 0) A.ray_start[n] = kept;
    }
}

// ray_start[0..N) holds the counts: turned in place into their exclusive scan, ray_start[N] = the total.  One workgroup: thread t owns a
// contiguous run of rays, the kThreads run totals are scanned in LDS.  (N is the ray count of one evaluation chunk.)
__global__ __launch_bounds__(kThreads)
void cull_scan_kernel(int64_t* __restrict__ ray_start, int64_t N) {
    __shared__ int64_t part[kThreads];
    const int tid = threadIdx.x;
    const int64_t per = (N + kThreads - 1) / kThreads;
    const int64_t b = min((int64_t)tid * per, N), e = min(b + per, N);
    int64_t sum = 0;
    for (int64_t i = b; i < e; ++i) sum += ray_start[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int i = 0; i < kThreads; ++i) { const int64_t v = part[i]; part[i] = run; run += v; }
    }
    __syncthreads();
    int64_t run = part[tid];
    for (int64_t i = b; i < e; ++i) { const int64_t v = ray_start[i]; ray_start[i] = run; run += v; }
    if (tid == kThreads - 1) ray_start[N] = run;             // (the last thread's run ends at N: its `run` is the total)
}

// ---------------------------------------------------------------------------------------------
// composite_kernel (cfnerf_fwd.hip) on a COMPACT raw: the same text (cfnerf_comp_fwd_body.h, CFN_COMP_SPARSE 1); only the fetch differs.
// A ray's kept rows are contiguous in raw_c, [ray_start[ray], ray_start[ray + 1]); the buffer descriptor covers exactly that block, so
// whatever `slot` holds, a load returns this ray's rows or zeros - never another ray's memory, never an unmapped page.  A chunk's staged
// block starts at the chunk's first kept row; a kept lane reads row rank(sample) of it, a culled lane contributes alpha = 0: the
// transmittance factor (1 - 0) + 1e-10f == 1.0f and every sum gets + 0.0f, both exact, so the maps carry the bits of composite_kernel on
// the dense raw whose culled samples have the density latent -1e4 (softplus gives exactly 0 there in both transcendental modes).
template <int KG, bool FAST>
__global__ __launch_bounds__(kThreads, FAST ? 4 : 3)
void composite_sparse_kernel(const float* __restrict__ raw_c, const int32_t* __restrict__ slot, const int64_t* __restrict__ ray_start,
                             const float* __restrict__ z_vals, const float* __restrict__ rays_d, int64_t N, int S, int K, int white_bkgd,
                             float* rgb_map, float* disp_map, float* depth_map, float* weights) {
#define CFN_COMP_SPARSE 1
#include "cfnerf_comp_fwd_body.h"
#undef CFN_COMP_SPARSE
}

// ---- host launchers (cfnerf_kernels.h)
hipError_t launch_cull(const CullArgs& a, hipStream_t st) {
    if (a.N > 0) {
        const int64_t groups = (a.N + kWaves - 1) / kWaves;
        const unsigned grid = (unsigned)std::min<int64_t>(groups, 1 << 30);
        hipLaunchKernelGGL(cull_kernel<false>, dim3(grid), dim3(kThreads), 0, st, a);
        hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(kThreads), 0, st, a.ray_start, a.N);
        hipLaunchKernelGGL(cull_kernel<true>, dim3(grid), dim3(kThreads), 0, st, a);
    } else {
        hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(kThreads), 0, st, a.ray_start, (int64_t)0);      // ray_start[0] = 0
    }
    return hipGetLastError();
}

hipError_t launch_composite_sparse(const float* raw_c, const int32_t* slot, const int64_t* ray_start, const float* z, const float* d, int64_t N,
                                   int S, int K, int wb, float* rgb, float* disp, float* depth, float* weights, hipStream_t st) {
    const int grid = (int)((N + kWaves - 1) / kWaves);
#define CFN_COMPS(KG, FAST) hipLaunchKernelGGL((composite_sparse_kernel<KG, FAST>), dim3(grid), dim3(kThreads), 0, st, raw_c, slot, ray_start, z, d, N, S, K, wb, rgb, disp, depth, weights)
    if (K <= 4) CFN_COMPS(4, false);                // (the same split as launch_composite: the culled and the dense path share their arithmetic)
    else if (K < kFastFlowsK) CFN_COMPS(8, false);
    else CFN_COMPS(8, true);
#undef CFN_COMPS
    return hipGetLastError();
}

}  // namespace cfnerf
