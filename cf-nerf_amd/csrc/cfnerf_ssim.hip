// cfnerf_ssim.hip - ssim_kernel: the structural similarity of two image batches x, y [B,H,W,C] (channel-last fp32, as render_uncertainty
// returns them) under a separable odd window of `win` taps, as one stateless launch (CFNERF_MODE_SSIM in the white_bkgd argument of
// cfnerf_composite_fwd, include/cfnerf.h).  It writes the map on the valid interior [B,H-win+1,W-win+1,C] and - through per-tile partial
// sums and a second small launch - the mean of each image and channel.
//
// Tiling.  One workgroup per (channel, 32 x 32 output tile, image); the channel is the fastest block index, so the C workgroups that read
// the same cache lines are dispatched side by side.  The tile is staged with its halo (up to 46 x 46 pixels of x and of y) in LDS, the
// horizontal pass writes the five row sums (x, y, xx, yy, xy) of every staged row to LDS, the vertical pass reads them back.  Tiles at the
// right and bottom edges are ragged (th, tw < 32); an image smaller than a tile is one ragged tile.  Lanes walk the columns, so every LDS
// access of both passes has stride 1; in the vertical pass a thread owns 4 consecutive rows of its column and reads each row sum once.
//
// Cancellation.  The window variance E[x^2] - mu^2 of a bright, flat render (mu^2 ~ 0.94, variance ~ 4e-6, C2 = 9e-4) loses everything in
// fp32: the difference is off by ~6e-8 of mu^2, 1e-4 of C2 + variance.  Here the five moments are carried in fp64 from the first tap to
// the quotient: x * x of an fp32 x is exact in fp64, and the difference cancels against 2^-53, not 2^-24.  The taps are the host's fp32 taps
// divided by their sum in double (SsimArgs::taps), so that sum t_i t_j = 1 to 2^-53 as well - a defect d of that sum would come back as
// d mu^2 in the variance.  (Moments about a per-tile pivot, in fp32, remove the cancellation too, but they make every output of a tile a
// function of every pixel of it through the pivot: a NaN pixel, or a changed one, would then move bits outside its own window.)  Each
// output here is a function of the win x win pixels under its window and of nothing else.
//
// Exactness.  The xx, yy and xy sums are the same statements on the same taps, 2 mu_x mu_y is 2 * (mu_x * mu_y) and mu_x^2 + mu_y^2 the sum
// of the two rounded products: with y == x numerator and denominator are the same bits and the quotient is exactly 1.
//
// Mean.  Each workgroup adds the fp32 values it has written, in double and in a fixed order (per lane, xor tree across the wave, the four
// waves in order), and writes ONE double to its own slot of the caller's scratch; ssim_mean_kernel adds the slots of an image and channel
// in a fixed order.  No atomics, no ticket: two runs give the same bits, and nothing of one image depends on another.  A NaN under a
// window makes that output NaN, hence its tile's partial and that image-and-channel's mean, and nothing else.
#include <hip/hip_runtime.h>

#include "cfnerf_device.h"
#include "cfnerf_kernels.h"

namespace cfnerf {

constexpr int kSsimStage = kSsimTile + kSsimMaxWin - 1;      // 46: the staged rows / columns of a full tile under the widest window
constexpr int kSsimStrip = 4;                                // output rows of one thread in the vertical pass

__device__ __forceinline__ double ssim_wave_sum(double v) {
#pragma unroll
    for (int j = 1; j < 64; j <<= 1) v = v + __shfl_xor(v, j, 64);
    return v;
}

template <int WIN>
__global__ __launch_bounds__(kThreads)
void ssim_kernel(const SsimArgs a) {
    __shared__ float sx[kSsimStage][kSsimStage + 1], sy[kSsimStage][kSsimStage + 1];
    __shared__ double hq[5][kSsimStage][kSsimTile];         // row sums of x, y, xx, yy, xy
    __shared__ double red[kWaves];
    const int tid = threadIdx.x;
    const int C = a.C;
    int64_t blk = blockIdx.x;
    const int c = (int)(blk % C); blk /= C;
    const int tx = (int)(blk % a.tiles_x); blk /= a.tiles_x;
    const int ty = (int)(blk % a.tiles_y);
    const int64_t b = blk / a.tiles_y;
    const int Hi = a.H - WIN + 1, Wi = a.W - WIN + 1;      // the interior
    const int r0 = ty * kSsimTile, c0 = tx * kSsimTile;
    const int th = min(kSsimTile, Hi - r0), tw = min(kSsimTile, Wi - c0);
    const int sh = th + WIN - 1, sw = tw + WIN - 1;         // staged: rows r0 .. r0 + sh - 1 <= H - 1, columns c0 .. c0 + sw - 1 <= W - 1

    for (int i = tid; i < sh * sw; i += kThreads) {
        const int r = i / sw, q = i - r * sw;
        const int64_t g = ((b * a.H + (r0 + r)) * a.W + (c0 + q)) * C + c;
        sx[r][q] = a.x[g];
        sy[r][q] = a.y[g];
    }
    __syncthreads();

    for (int i = tid; i < sh * tw; i += kThreads) {
        const int r = i / tw, q = i - r * tw;
        double mx = 0., my = 0., xx = 0., yy = 0., xy = 0.;
#pragma unroll
        for (int j = 0; j < WIN; ++j) {
            const double t = a.taps[j], xv = (double)sx[r][q + j], yv = (double)sy[r][q + j];
            mx = fma(t, xv, mx);
            my = fma(t, yv, my);
            xx = fma(t, xv * xv, xx);
            yy = fma(t, yv * yv, yy);
            xy = fma(t, xv * yv, xy);
        }
        hq[0][r][q] = mx; hq[1][r][q] = my; hq[2][r][q] = xx; hq[3][r][q] = yy; hq[4][r][q] = xy;
    }
    __syncthreads();

    // vertical pass: a thread owns column q and kSsimStrip consecutive output rows, so a row sum read once feeds every output of the
    // strip that it lies under (kSsimStrip + WIN - 1 rows read instead of kSsimStrip * WIN); each output still adds its taps in the
    // order j = 0 .. WIN - 1.  A strip that hangs over a ragged tile's bottom edge stops at the last staged row.
    static_assert(kThreads * kSsimStrip == kSsimTile * kSsimTile, "one strip per thread");
    const int q = tid % kSsimTile, rs = tid / kSsimTile * kSsimStrip;
    double part = 0.;
    if (q < tw && rs < th) {
        double acc[kSsimStrip][5] = {};
#pragma unroll
        for (int k = 0; k < kSsimStrip + WIN - 1; ++k) {
            if (rs + k >= sh) break;                      // behind the staged rows: only outputs below the tile's edge would read them
            double h[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) h[m] = hq[m][rs + k][q];
#pragma unroll
            for (int i = 0; i < kSsimStrip; ++i) {
                if (k - i >= 0 && k - i < WIN) {          // (compile time)
                    const double t = a.taps[k - i];
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[i][m] = fma(t, h[m], acc[i][m]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kSsimStrip; ++i) {
            const int r = rs + i;
            if (r < th) {
                const double mx = acc[i][0], my = acc[i][1], xx = acc[i][2], yy = acc[i][3], xy = acc[i][4];
                const double pxx = mx * mx, pyy = my * my, pxy = mx * my;
                const double vx = a.cov_norm * (xx - pxx), vy = a.cov_norm * (yy - pyy), vxy = a.cov_norm * (xy - pxy);
                const double num = (2. * pxy + a.c1) * (2. * vxy + a.c2);
                const double den = ((pxx + pyy) + a.c1) * ((vx + vy) + a.c2);
                const float s = (float)(num / den);
                if (a.map != nullptr) a.map[((b * Hi + (r0 + r)) * Wi + (c0 + q)) * C + c] = s;
                part = part + (double)s;
            }
        }
    }
    if (a.partials != nullptr) {
        part = ssim_wave_sum(part);
        if (lane_id() == 0) red[tid >> 6] = part;
        __syncthreads();
        if (tid == 0) {
            double t = red[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t = t + red[w];
            a.partials[((b * C + c) * a.tiles_y + ty) * (int64_t)a.tiles_x + tx] = t;
        }
    }
}

// mean [B,C]: one wave per image and channel adds its tiles' partial sums in a fixed order
__global__ __launch_bounds__(64)
void ssim_mean_kernel(const double* partials, int n_tiles, double count, float* mean) {
    const double* p = partials + (int64_t)blockIdx.x * n_tiles;
    double t = 0.;
    for (int i = threadIdx.x; i < n_tiles; i += 64) t = t + p[i];
    t = ssim_wave_sum(t);
    if (threadIdx.x == 0) mean[blockIdx.x] = (float)(t / count);
}

hipError_t launch_ssim(const SsimArgs& a, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    const unsigned grid = (unsigned)(a.B * a.C * a.tiles_y * a.tiles_x);      // (the caller has checked that it fits)
    switch (a.win) {
#define CFN_SSIM(WIN) case WIN: hipLaunchKernelGGL(ssim_kernel<WIN>, dim3(grid), dim3(kThreads), 0, st, a); break;
        CFN_SSIM(3) CFN_SSIM(5) CFN_SSIM(7) CFN_SSIM(9) CFN_SSIM(11) CFN_SSIM(13) CFN_SSIM(15)
#undef CFN_SSIM
        default: return hipErrorInvalidValue;
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.mean != nullptr) {
        const double count = (double)(a.H - a.win + 1) * (double)(a.W - a.win + 1);
        hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)(a.B * a.C)), dim3(64), 0, st, a.partials, a.tiles_y * a.tiles_x, count, a.mean);
    }
    return hipGetLastError();
}

}  // namespace cfnerf
