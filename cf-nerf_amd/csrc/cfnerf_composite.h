// cfnerf_composite.h - what the four stand-alone composite kernels share outside their bodies: the pass constants and the staged LDS block.
//   composite_kernel         (cfnerf_fwd.hip)   dense forward            }  one body, cfnerf_comp_fwd_body.h (CFN_COMP_SPARSE 0 / 1)
//   composite_sparse_kernel  (cfnerf_cull.hip)  forward on a compact raw }
//   composite_bwd_kernel     (cfnerf_bwd.hip)   d_raw                    }  one body, cfnerf_comp_bwd_body.h (CFN_COMP_SEAM 0 / 1)
//   comp_seam_zgrad_kernel   (cfnerf_bwd.hip)   d_z_vals, d_rays_d       }
// raw2outputs (RUN:411-454) and its adjoint are written once each, as TEXT included per kernel (see the bodies for why not as functions).
// The cross-lane steps (comp_scan_mul, comp_sum, comp_last, comp_adjoint_D) stay in cfnerf_device.h with the fused kernels that share them.
#pragma once
#include "cfnerf_device.h"

namespace cfnerf {

constexpr int kCompKB = 64;                   // latents of one forward pass over a ray's chunks (their carries and sums wait in LDS, entry = lane)
constexpr int kCompMaxChunks = 64;            // adjoint: a latent's transmittance entering every chunk waits in LDS, S <= 4096

// The [64 samples][KG latents] block of quads (16 bytes = one (sample, latent) entry of raw [N,S,K,4]) of a 64-sample chunk, filled by
// KG LDS-DMA pieces: piece j, lane l lands at quad position p = 64 j + l.  Position p = sl * KG + c holds latent kk = c ^ swz(sl) of
// sample sl: the KG lanes of a sample still cover its one 16 KG-byte segment of global memory (every piece is 1 KB of full cache lines
// when K is a multiple of KG), and the transposed read - lane = sample, one latent - touches 16 different bank quads per 16 lanes.
template <int KG> struct CompStage {
    static_assert(KG == 4 || KG == 8, "a sample's segment is 64 or 128 bytes");
    static constexpr int kQuads = 64 * KG;
    static __device__ __forceinline__ int swz(int sl) { return (sl / (16 / KG)) & (KG - 1); }
    // this lane's byte offset (inside the chunk's rows of the ray, group 0) of the quad it moves in piece j
    static __device__ __forceinline__ unsigned piece_voff(int lane, int j, int K) {
        const int p = j * 64 + lane, sl = p / KG, kk = (p % KG) ^ swz(sl);
        return (unsigned)((sl * K + kk) * 16);
    }
    static __device__ __forceinline__ void fetch(i32x4 rsrc, unsigned lds0, const unsigned (&voff)[KG], int ch, int g0, int K) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the previous block's LDS reads have their data
        wave_lds_turn();
        const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane((ch * 64 * K + g0) * 16);
#pragma unroll
        for (int j = 0; j < KG; ++j) ds_dma16(rsrc, lds0 + j * 1024, voff[j], soff);
    }
    static __device__ __forceinline__ void landed() {            // (hipcc does not count asm memory operations: explicit wait)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wave_lds_turn();
    }
};

}  // namespace cfnerf
