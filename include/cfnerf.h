/*
 * cfnerf.h - C ABI of the MI355X-native CF-NeRF ray-batch hot path (libcfnerf_hip.so).
 *
 * The reference (poetrywanderer/CF-NeRF) is pure Python/PyTorch and has NO FFI layer: its seam is
 * the Python call chain  render() -> render_rays() -> network_query_fn() -> NeRF_Flows.forward()
 * -> raw2outputs()  (run_nerf_uncertainty_NF.py:103-170, 457-553, 67-85, 411-454;
 * model/models.py:188-291).  Each entry point below names the reference function it replaces.
 * The Python host mirror (cf-nerf_amd/) binds these symbols with ctypes and re-exposes the
 * reference's signatures; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - plain C, no torch types; every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every buffer: outputs, parameters, gradients, Adam moments and - through
 *     cfnerf_workspace_bytes / cfnerf_model_set_workspace - the train-step workspace (activation stash,
 *     pre-activation gradients, split-K partials).  A cfnerf_model itself owns only the packed weight copies and a
 *     few KB of scratch, allocated in cfnerf_model_create.  A caller that hands in NO workspace gets a model-owned
 *     one that grows on demand (the only allocation outside create; it synchronises the device when it grows);
 *   - every launch is asynchronous on the hipStream_t passed in (pass torch's current stream); on the steady
 *     path (same N, S, K and workspace as the previous step) no entry point allocates, frees or synchronises.
 *     NOT steady: a caller that alternates two shapes on one model - the coarse + fine sampling EXTENSION of the host
 *     mirror (train.Trainer.step_hierarchical: (N, 64, K) then (N, 192, K) every step) re-binds the one workspace twice
 *     per step, so both of its cfnerf_render_bwd calls take the plan-rebuild path (weight-gradient descriptors rebuilt
 *     and uploaded from double-buffered host copies, <= 300 MB of partials cleared: ~50 us each, asynchronous, but a host
 *     sync when the model-owned workspace has to grow).  One plan slot per model is the contract; a caller that needs two
 *     shapes at full speed uses two cfnerf_model handles, each re-packed from the one parameter buffer (cfnerf_model_set_params);
 *   - return value: 0 = OK, negative = cfnerf_status; cfnerf_last_error() gives a thread-local
 *     message.  No C++ exception crosses the ABI;
 *   - a handle lives on the device that was current at cfnerf_model_create (one handle per device, one
 *     process per GPU); calls made with another device current are rejected.  Calls that do not take a
 *     handle are stateless and re-entrant.  Calls on ONE handle share its workspaces (entropy partials,
 *     stash, split-K partials): issue them from one host thread at a time and on one stream at a time
 *     (or order the streams with events); different handles are independent;
 *   - all arithmetic is fp32 (exact-fp32 MFMA v_mfma_f32_32x32x2_f32 for the dense layers).
 */
#ifndef CFNERF_H
#define CFNERF_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: its dynamic symbol table holds the entry points declared in THIS header and
 * nothing else - no C++ symbol, no helper, no test hook (those live in a separate test library, tests/cfnerf_debug.h).
 * tests/test_abi_cpu.py compares `nm -D --defined-only` of the library with this header. */
#if defined(__GNUC__) || defined(__clang__)
#define CFNERF_API __attribute__((visibility("default")))
#else
#define CFNERF_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cfnerf_stream;            /* hipStream_t */

typedef enum cfnerf_status {
    CFNERF_OK = 0,
    CFNERF_E_INVALID = -1,              /* bad argument / shape */
    CFNERF_E_UNSUPPORTED = -2,          /* configuration the reference accepts silently but this path rejects */
    CFNERF_E_HIP = -3,                  /* HIP runtime error (message holds hipGetErrorString) */
    CFNERF_E_NOMEM = -4
} cfnerf_status;

/* The flags of config_parser() that reach the hot path (run_nerf_uncertainty_NF.py:556-719). */
typedef struct cfnerf_cfg {
    int32_t netdepth;                   /* --netdepth   (8)   skip connection after layer netdepth/2 (RUN:327) */
    int32_t netwidth;                   /* --netwidth   (256) a multiple of 64 in [64, 512] */
    int32_t multires;                   /* --multires   (10)  -> 63 input channels (run_nerf_helpers.py:54-69) */
    int32_t multires_views;             /* --multires_views (4) -> 27 channels */
    int32_t h_alpha_size;               /* --h_alpha_size (32) 32, 64, 96 or 128 */
    int32_t h_rgb_size;                 /* --h_rgb_size (64)  32, 64, 96 or 128, with netwidth / 2 + h_rgb_size <= max(netwidth, 128) */
    int32_t n_flows;                    /* --n_flows    (4)   1 .. 4 (fewer than 4 steps run as 4 with the missing steps' parameters zero: identity steps) */
} cfnerf_cfg;

typedef struct cfnerf_model cfnerf_model;   /* opaque: packed weights + workspaces for ONE device */

/* flags for the render / network entry points */
enum {
    CFNERF_F_TRAIN      = 1 << 0,       /* train branch of NeRF_Flows.forward (MOD:225-291): log-dets + entropy */
    CFNERF_F_LINDISP    = 1 << 1,       /* render_rays(lindisp=True)  RUN:513-514 */
    CFNERF_F_WHITE_BKGD = 1 << 2,       /* raw2outputs(white_bkgd=True) RUN:451-452 */
    CFNERF_F_STASH      = 1 << 3,       /* keep activations for cfnerf_render_bwd (implies TRAIN); ONE stash per model: a later
                                           STASH forward replaces it and bumps cfnerf_model_stash_generation */
    CFNERF_F_EPS_ROWS   = 1 << 4,       /* eps holds one [K,4] row per work item - per RAY in cfnerf_render_fwd ([N,K,4]), per POINT
                                           in cfnerf_network_fwd ([P,K,4]) - instead of one [K,4] for the launch: the reference draws
                                           fresh latents per netchunk (RUN:47-64,82; MOD:234,246), so a batch of several netchunks
                                           uses several latent sets.  Train branch only (cfnerf_render_eval refuses it).  With
                                           CFNERF_F_STASH the stash keeps the CALLER's eps pointer (no copy, no workspace growth):
                                           the rows buffer must stay alive and unchanged until the matching backward has been
                                           enqueued and has run, like a lent workspace */
    CFNERF_F_KSTATS_EXT = 1 << 5,       /* the metrics of the paper's tables from the same launch: kstats rows grow from 8 to 12 floats and
                                           sqerr rows from 3 to 6 (layouts at cfnerf_render_fwd / cfnerf_render_eval).  Accepted by
                                           cfnerf_render_eval and by cfnerf_render_fwd with kstats_opt (train or eval branch, without
                                           CFNERF_F_STASH and without CFNERF_F_EPS_ROWS); every other entry point that takes flags refuses
                                           it.  Without the flag every buffer shape and every output bit is what it was */
    CFNERF_F_GEOMETRY   = 1 << 6,       /* geometry only: the launch runs trunk -> h_alpha -> the density flow (and, for rays, the composite's
                                           depth / opacity sums) and skips the colour branch - feature head, views layer, h_rgb head, colour
                                           flows: 18.65 % of the dense work at W = 256 and three quarters of the flow phase.  Eval branch only:
                                           refused together with CFNERF_F_TRAIN, CFNERF_F_STASH, CFNERF_F_EPS_ROWS or CFNERF_F_KSTATS_EXT.
                                           Accepted by cfnerf_network_fwd (raw is [P,K], the density latent), cfnerf_render_fwd (rgb_map NULL,
                                           raw_opt [N,S,K], kstats_opt [N,6]) and cfnerf_render_eval (kstats [N,6], no gt / sqerr); layouts at
                                           those entry points.  What is written equals, bit for bit, the same quantity of the launch without
                                           the flag.  Every other entry point that takes flags refuses it.  Without the flag every buffer
                                           shape and every output bit is what it was */
    CFNERF_F_INPUT_GRAD = 0x80,         /* (= 1 << 7, bit 7) the matching cfnerf_network_bwd also writes d loss / d x, the gradient with respect to the
                                           pre-embedded inputs (the reference's NeRF_Flows.forward is an autograd graph in x too: a learnable
                                           front end - pose correction, deformation field, learned encoding - trains through it).  Accepted by
                                           cfnerf_network_fwd only, and only together with CFNERF_F_STASH (the stash remembers it); refused with
                                           CFNERF_F_GEOMETRY; combines freely with CFNERF_F_EPS_ROWS.  The backward of such a stash treats
                                           grad_flat as [x_off + P * (input_ch + input_ch_views)] floats with
                                               x_off = (cfnerf_param_count(cfg) + 63) / 64 * 64 :
                                           [0, param_count) the parameter gradient, bit for bit what it is without the flag; d_x
                                           [P, input_ch + input_ch_views] row-major from x_off; the floats in between are not written.
                                           Every other entry point that takes flags refuses it.  Without the flag there is no extra launch and
                                           every buffer shape and every output bit is what it was */
    CFNERF_F_RAY_GRAD   = 0x100,        /* (= 1 << 8, bit 8) the matching cfnerf_render_bwd / cfnerf_render_bwd_accumulate also writes d loss / d rays and d loss / d z_vals
                                           (the reference's render() is one autograd graph from c2w / rays_o / rays_d to the loss: pose
                                           refinement, registration of an image against a trained model, a learnable warp on the rays).
                                           Accepted by cfnerf_render_fwd only, and only together with CFNERF_F_STASH (the stash remembers it);
                                           combines with CFNERF_F_EPS_ROWS, CFNERF_F_LINDISP, CFNERF_F_WHITE_BKGD, z_vals_opt and both precision
                                           modes; refused with CFNERF_F_GEOMETRY / CFNERF_F_KSTATS_EXT.  The forward launch and every output bit
                                           are what they are without the flag.  The backward of such a stash treats grad_flat as
                                           [z_off + N * S] floats with
                                               r_off = (cfnerf_param_count(cfg) + 63) / 64 * 64,   z_off = r_off + (N * 11 + 63) / 64 * 64 :
                                           [0, param_count) the parameter gradient, bit for bit what it is without the flag (_accumulate
                                           still ADDS there); d_rays [N,11] row-major from r_off; d_z [N,S] from z_off; the pad floats
                                           between the blocks are not written.  Columns of d_rays: 0..2 d loss / d rays_o, 3..5 d loss /
                                           d rays_d (through the sample points AND through |rays_d| of the composite's distances, RUN:429),
                                           6, 7 written as 0 - the gradient for near / far is NOT computed: a caller who wants it chains
                                           d_z through the sampling lines (RUN:510-532) on the host - 8..10 d loss / d viewdirs.  d_z is the
                                           total gradient with respect to the sample depths (z_vals_opt if given, else the sampled z_vals):
                                           the composite's distances and depth_map, and the sample points.  The two ray blocks are per-launch
                                           quantities: ALWAYS overwritten, also by cfnerf_render_bwd_accumulate.  Cotangents of disp_map,
                                           weights and raw (CFNERF_F_COTANGENTS) reach d_rays and d_z as they reach the parameters.  Exact-fp32 MFMA
                                           in both precision modes, no atomics: bit-reproducible.  cfnerf_workspace_bytes does not change.  Every
                                           other entry point that takes flags refuses it.  Without the flag there is no extra launch and every
                                           buffer shape and every output bit is what it was */
    CFNERF_F_COTANGENTS = 0x200,        /* (= 1 << 9, bit 9) the matching cfnerf_render_bwd / cfnerf_render_bwd_accumulate takes cotangents for disp_map,
                                           weights and raw as well (in the reference every output of render() is on the autograd graph: a disparity
                                           loss, a density prior on raw[..., 3], a distortion or ray-entropy regulariser on the weights of
                                           raw2outputs, RUN:411-454).  There is no new entry point: with the flag in the stash, the `d_rgb_map` ARGUMENT
                                           of the backward is read as a pointer to a HOST struct cfnerf_cotangents (below) - the caller passes
                                           (const float*)&cot - whose member d_rgb_map is the cotangent proper.  The struct is read during the call
                                           and not kept; its members are DEVICE pointers that must stay alive until the backward has run.  d_depth_map
                                           and d_entropy stay arguments.  Accepted by cfnerf_render_fwd only, and only together with CFNERF_F_STASH
                                           (the forward launch never sees the bit: the stash remembers it); combines with CFNERF_F_RAY_GRAD (d_rays /
                                           d_z then hold the gradient of the same loss), CFNERF_F_EPS_ROWS, CFNERF_F_LINDISP, CFNERF_F_WHITE_BKGD,
                                           z_vals_opt and both precision modes; refused with CFNERF_F_GEOMETRY / CFNERF_F_KSTATS_EXT.  When the three
                                           optional members are NULL the backward launches exactly the kernels it launches without the flag: the
                                           parameter gradient, d_rays and d_z are the same bits.  cfnerf_workspace_bytes does not change.  Every other
                                           entry point that takes flags refuses it.  Without the flag every argument means what it meant */
    CFNERF_F_SEAM_GRAD  = 0x400,        /* (= 1 << 10, bit 10) cfnerf_composite_bwd also differentiates raw2outputs in z_vals and rays_d (RUN:424-429, 447:
                                           in the reference raw2outputs(raw, z_vals, rays_d) is a graph in all three arguments - the link a script that
                                           refines poses needs when it injects a network_query_fn of its own).  cfnerf_composite_bwd takes no flags:
                                           the bit is passed in its `white_bkgd` ARGUMENT, and the background is white iff (white_bkgd & ~0x400) != 0,
                                           so every value a caller passes today means what it meant.  There is no new entry point: with the bit, the
                                           `d_raw` ARGUMENT is read as a pointer to a HOST struct cfnerf_composite_grads (below) - the caller passes
                                           (float*)&grads - naming what to write: d_raw, d_z_vals, d_rays_d, each NULL when not wanted (all three NULL
                                           is refused).  The struct is read during the call and not kept.  d_raw is written by the launch of the plain
                                           call (the same bits); d_z_vals / d_rays_d by a second launch that reads raw once more, skipped when neither
                                           is wanted, as the first is when d_raw is not.  No atomics: bit-reproducible.  Every entry point that takes
                                           `flags` refuses the bit.  Without the bit the call is what it was */
    CFNERF_F_CULL       = 0x800,        /* (= 1 << 11, bit 11) render through an occupancy grid: samples in empty cells never reach the network.  An
                                           EVALUATION path (inference only, no backward) over the unfused seam, with no new entry point:
                                             cfnerf_sample_points with the flag reads its `pts` ARGUMENT as a pointer to a HOST struct cfnerf_cull (below) -
                                               the caller passes (float*)&cull - and writes z_vals as always plus the keep / skip decision of every sample
                                               and the compact list of the kept points, in (ray, sample) order;
                                             cfnerf_embed and cfnerf_network_fwd run on that list as on any P' points;
                                             cfnerf_composite_fwd takes the bit in its `white_bkgd` ARGUMENT - the background is white iff
                                               (white_bkgd & ~0x800) != 0, so every value a caller passes today means what it meant - and then reads raw as
                                               [P',K,4], rows for the kept samples only, and its `weights_opt` ARGUMENT as a pointer to a HOST struct
                                               cfnerf_sparse_raw (below), (float*)&sp.
                                           The caller learns P' by reading ray_start[N] back: ONE device-to-host copy per call, which SYNCHRONISES - the
                                           "nothing synchronises" contract of the train step does not cover this path and is not affected by it.  The
                                           compaction is deterministic (no atomics).  cfnerf_composite_bwd does not take the bit.  Every entry point that takes
                                           `flags` other than cfnerf_sample_points refuses it.  Without the bit every call is what it was */
    CFNERF_F_EPS_GRAD   = 0x1000,       /* (= 1 << 12, bit 12) the matching cfnerf_render_bwd / cfnerf_render_bwd_accumulate / cfnerf_network_bwd also writes
                                           d loss / d eps, the gradient with respect to the latents (in the reference eps.mul(std).add_(mean), MOD:239,251,
                                           is an ordinary autograd line: fitting a latent set to an observation, per-image or per-ray latents, a learned
                                           base distribution in front of the flows).  Accepted by cfnerf_render_fwd and cfnerf_network_fwd, and only
                                           together with CFNERF_F_STASH (the stash remembers it; the forward launch and every output bit are what they
                                           are without it); combines with CFNERF_F_EPS_ROWS, CFNERF_F_RAY_GRAD, CFNERF_F_COTANGENTS, CFNERF_F_INPUT_GRAD,
                                           CFNERF_F_LINDISP, CFNERF_F_WHITE_BKGD, z_vals_opt and both precision modes; refused with CFNERF_F_GEOMETRY,
                                           CFNERF_F_KSTATS_EXT and CFNERF_F_CULL.  The backward of such a stash treats grad_flat as [er_off + n * K * 4]
                                           floats, n = N rays (cfnerf_render_fwd) or P points (cfnerf_network_fwd).  With base_end the end of the blocks
                                           the stash already asks for - param_count, z_off + N * S with CFNERF_F_RAY_GRAD, x_off + P * (input_ch +
                                           input_ch_views) with CFNERF_F_INPUT_GRAD -
                                               e_off = (base_end + 63) / 64 * 64,   er_off = e_off + (4 * K + 63) / 64 * 64 :
                                           d_eps [K,4] from e_off and d_eps_rows [n,K,4] from er_off, columns rgb then alpha like eps; the pad floats are
                                           not written; everything before e_off is bit for bit what it is without the flag.  d_eps_rows[i] is
                                           d loss / d (row i of eps) had the launch been a CFNERF_F_EPS_ROWS launch - for a launch with one [K,4] set, the
                                           rows launch with n identical rows.  d_eps is the sum of the rows over i in a fixed order (double accumulators,
                                           rounded once): for a launch with one set, the gradient of that set.  Both hold the chain through
                                           z0 = eps * std + mean and the direct term of the base log-normal in the entropy (MOD:268,283,286; over the
                                           launch -d_entropy * eps[k,3] / K for the density latent and -d_entropy * eps[k,c] / (3 K) for a colour latent,
                                           each row 1 / n of it with its own eps).  Both are per-launch quantities: ALWAYS overwritten, also by
                                           cfnerf_render_bwd_accumulate.  No atomics: bit-reproducible.  cfnerf_workspace_bytes does not change - the
                                           caller's grad_flat is the only new memory.  Every other entry point that takes flags refuses it.  Without the
                                           flag there is no extra launch and every argument, buffer shape and output bit is what it was */
    CFNERF_F_RAY_REG    = 0x2000,       /* (= 1 << 13, bit 13) the two ray regularisers of few-view training as ONE stateless launch over the composite's
                                           weights [N,S,K] (what CFNERF_F_COTANGENTS made differentiable): the distortion loss of mip-NeRF 360 and the
                                           ray-entropy loss of InfoNeRF, with their gradient.  There is no new entry point: the bit is or-ed into the
                                           `white_bkgd` ARGUMENT of cfnerf_composite_fwd, which then composites nothing - z_vals [N,S] (non-decreasing
                                           per ray) is required, raw, rays_d, rgb_map, disp_map and depth_map must be NULL, and the `weights_opt` ARGUMENT
                                           is read as a pointer to a HOST struct cfnerf_ray_reg (below), (float*)&rr; the struct is read during the call
                                           and not kept.  For one (ray, latent), w_i = weights[n,i,k]:
                                             s_i = (z_i - near) / (far - near), near / far = columns 6 / 7 of rays [N,11]; rays NULL: s_i = z_i
                                             interval i < S-1 is [s_i, s_i+1]: m_i = (s_i + s_i+1) / 2, delta_i = s_i+1 - s_i; the last sample (the
                                               composite's 1e10 interval) is the point m_S-1 = s_S-1, delta_S-1 = 0
                                             D = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i
                                             A = sum_i w_i,  p_i = w_i / (A + 1e-10),  H = - sum_i p_i log(p_i + 1e-10),  mask = (A > acc_min), a constant
                                           and over the launch, with n = n_total (0: N):
                                             dist = sum_nk D / (n K),  ent = sum_nk mask H / (n K),  frac = sum_nk mask / (n K),
                                             reg = lambda_dist dist + lambda_ent ent
                                           scalars_out receives {reg, dist, ent, frac} (+ 4 floats of zeros), d_weights [N,S,K] = d reg / d weights -
                                           scaled, a cfnerf_cotangents.d_weights as it stands - and d_z_opt [N,S], when given, the DIRECT d reg / d z_vals
                                           through m and delta, summed over K, divided by (far - near); the path through the weights is the composite's
                                           backward's.  Launches that share n_total add up: their scalars and gradients are those of slices of one batch.
                                           O(S) per (ray, latent); any S in [1, 4096], K in [1, 128], N >= 0.  A lambda of 0 skips that term: the gradient
                                           then has the bits of the other term's alone.  The sums are integer accumulations: bit-reproducible.  Refused by
                                           name, before anything touches a device: a NULL struct, a NULL weights / d_weights / scalars_out / z_vals, a
                                           non-NULL raw / rays_d / rgb_map / disp_map / depth_map, the bit together with CFNERF_F_CULL, S < 1, K < 1, N < 0.
                                           cfnerf_composite_bwd does not take the bit; every entry point that takes `flags` refuses it.  NOTE: a white_bkgd
                                           value with bit 13 set used to mean "white" like any non-zero value; it now selects this mode (nothing in the
                                           project passes such a value).  Without the bit every call is what it was */
    CFNERF_F_KSCORES    = 0x4000        /* (= 1 << 14, bit 14) the K latent samples of a pixel scored as an ENSEMBLE, as ONE stateless launch over the
                                           rows of samples [M,K] (rgb_map [N,3,K] as M = 3N rows, depth_map / disp_map [N,K] as M = N rows): each row
                                           sorted ascending, its quantiles and - against a target y - the rank of y among the samples (the PIT) and the
                                           CRPS of the ensemble.  There is no new entry point: the bit is or-ed into the `white_bkgd` ARGUMENT of
                                           cfnerf_composite_fwd, which then composites nothing - N is the number of rows M, S must be 1, K in [1, 128],
                                           raw, z_vals, rays_d, rgb_map, disp_map and depth_map must be NULL, and the `weights_opt` ARGUMENT is read as a
                                           pointer to a HOST struct cfnerf_kscores (below), (float*)&ks; the struct is read during the call and not
                                           kept.  Every output is optional, at least one must be requested.  For one row x_0 .. x_K-1 with order
                                           statistics x_(0) <= .. <= x_(K-1) (NaN orders after +inf, as torch.sort does):
                                             sorted     the row ascending: a permutation of its 32-bit patterns (compare-and-select, no arithmetic on a
                                                        value: denormals, +-0, +-inf pass through untouched)
                                             quantiles  level t of n_levels <= 16 is (level_lo[t], level_frac[t]), made by the HOST from q in [0,1]:
                                                        lo = floor(q (K-1)) in double, frac = the fractional part rounded once to float; the value is
                                                        x_(lo) + frac (x_(hi) - x_(lo)), hi = min(lo + 1, K - 1) - numpy.quantile(method="linear"); with
                                                        frac == 0 it is x_(lo) bit for bit
                                             rank_code  (int32) 2 #{x_k < y} + #{x_k == y}, in [0, 2K];  pit = (float)rank_code / (float)(2K)
                                             crps       A - B,  A = (1/K) sum_k |x_k - y|,  B = (1/K^2) sum_{g<K-1} (g+1)(K-1-g) (x_(g+1) - x_(g)): B is the
                                                        ensemble's 1/(2K^2) sum_kl |x_k - x_l| over the sorted gaps, non-negative terms only
                                           rank_code, pit and crps need target [M].  A row that holds a NaN, or whose target is NaN, gets NaN quantiles /
                                           crps / pit and rank_code -1; the other rows are not affected.  No atomics and no reduction across rows: every
                                           output of a row depends on that row alone - bit-reproducible, whatever rows share a launch.  Refused by name,
                                           before anything touches a device: a NULL struct, a NULL samples, no output requested, crps / pit / rank_code
                                           without target, quantiles with n_levels outside [1,16], a level_lo outside [0, K-1] or a level_frac outside
                                           [0,1), a non-NULL raw / z_vals / rays_d / rgb_map / disp_map / depth_map, S != 1, K < 1, K > 128, N < 0, the
                                           bit together with CFNERF_F_CULL or CFNERF_F_RAY_REG.  cfnerf_composite_bwd does not take the bit; every entry
                                           point that takes `flags` refuses it.  NOTE: a white_bkgd value with bit 14 set used to mean "white" like any
                                           non-zero value; it now selects this mode (nothing in the project passes such a value).  Without the bit every
                                           call is what it was */
};

/* A mode bit that is not a flag of the network: like CFNERF_F_RAY_REG and CFNERF_F_KSCORES it travels in the `white_bkgd` ARGUMENT of
 * cfnerf_composite_fwd and selects a stateless launch of its own, but it has an enum of its own.
 *
 * CFNERF_MODE_SSIM (bit 15): the structural similarity (Wang et al. 2004; skimage.metrics.structural_similarity) of two image batches
 * x, y [B,H,W,C] - channel-last fp32, as the evaluation renders are - under a separable odd window of `win` taps, on the VALID interior:
 * with p = (win - 1) / 2 the map is [B,H-2p,W-2p,C] (there is no boundary mode), and `mean` [B,C] is its mean per image and channel.  With
 * the bit set nothing is composited: N is the number of images B, S must be 1, K is the channel count C in [1,4], raw, z_vals, rays_d,
 * rgb_map, disp_map and depth_map must be NULL, and the `weights_opt` ARGUMENT is read as a pointer to a HOST struct cfnerf_ssim (below),
 * (float*)&s; the struct is read during the call and not kept.  For every interior pixel and channel, with the taps t (used as t_i / sum t):
 *     mu_x, mu_y = sum_ij t_i t_j x, y          v_x, v_y, v_xy = cov_norm (sum_ij t_i t_j x^2, y^2, xy  -  mu_x^2, mu_y^2, mu_x mu_y)
 *     S = (2 mu_x mu_y + c1)(2 v_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(v_x + v_y + c2))
 * One kernel serves both conventions, because the HOST supplies taps and cov_norm: skimage's default is the uniform window, win = 7,
 * cov_norm = n / (n - 1) with n = win^2; gaussian_weights=True (Wang et al.) is sigma = 1.5, radius int(3.5 sigma + 0.5) = 5, win = 11,
 * cov_norm = 1, the taps normalised in double and rounded once to float.  c1 = (0.01 L)^2 and c2 = (0.03 L)^2 for a data range L.
 * Arithmetic: the five window moments are accumulated in fp64 from the fp32 pixels (x^2 is then exact), so v = E[x^2] - mu^2 does not
 * cancel against c2 on a bright, flat image as it does in fp32; the quotient is rounded once to fp32.  ssim(x, x) is exactly 1.0f at every
 * pixel and in the mean.  Every output pixel depends on the win x win pixels under its window alone: a NaN pixel makes NaN exactly the
 * outputs whose window covers it, plus mean[b,c] of its image and channel.  The mean is the sum of the fp32 map values, in fp64 and in a
 * fixed order (one partial sum per 32 x 32 tile in `scratch`, added by a second small launch): no atomics, bit-reproducible, and nothing
 * of an image depends on its batch-mates.  ssim_map and mean are each optional, at least one must be requested; mean needs scratch:
 * CFNERF_SSIM_SCRATCH_FLOATS(B, C, H, W, win) floats, 8-byte aligned (it holds doubles), owned by the caller, free once the stream has
 * passed the call.  Refused by name, before anything touches a device: a NULL struct, a NULL x or y, no output requested, mean without
 * scratch, a misaligned scratch, win even or outside [3,15], H or W below win, K outside [1,4], S != 1, N < 0 (N == 0 is accepted and
 * launches nothing), more than 2^31 - 1 tiles, a non-finite or non-positive c1, c2 or cov_norm, a non-finite tap or taps that do not
 * sum to a positive number, a non-NULL raw / z_vals / rays_d / rgb_map / disp_map / depth_map, the bit together with CFNERF_F_CULL,
 * CFNERF_F_RAY_REG or CFNERF_F_KSCORES.  Every entry point that takes `flags` refuses the bit.  cfnerf_composite_bwd does not take it:
 * there the background is white iff (white_bkgd & ~CFNERF_F_SEAM_GRAD) != 0, as it was, whatever other bits are set.  NOTE: in
 * cfnerf_composite_fwd a white_bkgd value with bit 15 set used to mean "white" like any non-zero value; it now selects this mode (nothing
 * in the project passes such a value).  Without the bit every call is what it was. */
enum cfnerf_mode { CFNERF_MODE_SSIM = 0x8000 };   /* bit 15 */

#define CFNERF_SSIM_TILE 32             /* the output tile of one workgroup: one partial sum per tile, image and channel */
/* floats of cfnerf_ssim.scratch for B images of H x W x C under a window of win taps (H, W >= win): two per partial sum */
#define CFNERF_SSIM_SCRATCH_FLOATS(B, C, H, W, win) \
    (2 * (int64_t)(B) * (int64_t)(C) * (((H) - (win)) / CFNERF_SSIM_TILE + 1) * (((W) - (win)) / CFNERF_SSIM_TILE + 1))

/* The cotangents of a CFNERF_F_COTANGENTS backward: a HOST struct of DEVICE pointers, passed in place of d_rgb_map. */
typedef struct cfnerf_cotangents {
    const float* d_rgb_map;             /* [N,3,K]   required */
    const float* d_disp_map;            /* [N,K]     NULL = zeros */
    const float* d_weights;             /* [N,S,K]   NULL = zeros; row-major, as weights_opt is written */
    const float* d_raw;                 /* [N,S,K,4] NULL = zeros; row-major, as raw_opt is written */
} cfnerf_cotangents;

/* What a CFNERF_F_SEAM_GRAD cfnerf_composite_bwd writes: a HOST struct of DEVICE pointers, passed in place of d_raw. */
typedef struct cfnerf_composite_grads {
    float* d_raw;                       /* [N,S,K,4] or NULL: not wanted */
    float* d_z_vals;                    /* [N,S]     or NULL */
    float* d_rays_d;                    /* [N,3]     or NULL */
} cfnerf_composite_grads;

/* The occupancy grid and the outputs of a CFNERF_F_CULL cfnerf_sample_points: a HOST struct of DEVICE pointers, passed in place of pts;
 * read during the call, not kept.  The grid is X*Y*Z cells on the box from `lo`; the cell of a point is, per axis,
 * floorf((p - lo) * scale) in fp32 (subtract, multiply, floor - nothing else), p with the bits the plain call writes to pts; the point is
 * inside iff 0 <= cell < res on all three axes.  A sample is KEPT iff its cell's bit is set; outside the box (or NaN) `outside` decides. */
typedef struct cfnerf_cull {
    const uint32_t* occ_bits;           /* X*Y*Z bits; cell (ix,iy,iz) is bit ((ix*Y+iy)*Z+iz) & 31 of word ((ix*Y+iy)*Z+iz) >> 5 */
    float   lo[3];                      /* corner of cell (0,0,0) */
    float   scale[3];                   /* res[d] / (hi[d] - lo[d]), computed by the HOST in fp32 */
    int32_t res[3];                     /* X, Y, Z cells (each >= 1) */
    int32_t outside;                    /* 0: a point outside the box (or NaN) is KEPT, 1: culled */
    int32_t* slot;                      /* [N,S] out: row of the sample in the compact list, -1 = culled */
    int64_t* ray_start;                 /* [N+1] out: exclusive scan of the per-ray kept counts; ray_start[N] = P' */
    float*   pts_c;                     /* [N*S,3] out: the first P' rows are written, in (ray, sample) order */
    int32_t* ray_of;                    /* [N*S] out: the ray of each compact row (the first P' entries are written) */
} cfnerf_cull;

/* Where the rows of a CFNERF_F_CULL cfnerf_composite_fwd's raw [P',K,4] belong: a HOST struct of DEVICE pointers, passed in place of
 * weights_opt; read during the call, not kept. */
typedef struct cfnerf_sparse_raw {
    const int32_t* slot;                /* [N,S] as written by cfnerf_sample_points */
    const int64_t* ray_start;           /* [N+1] */
    float* weights_opt;                 /* [N,S,K] or NULL; a culled sample's weights are written as 0 */
} cfnerf_sparse_raw;

/* The inputs and outputs of a CFNERF_F_RAY_REG cfnerf_composite_fwd: a HOST struct of DEVICE pointers, passed in place of weights_opt;
 * read during the call, not kept. */
typedef struct cfnerf_ray_reg {
    const float* weights;               /* [N,S,K] required: weights_opt of a forward */
    const float* rays;                  /* [N,11] or NULL: near / far in columns 6 / 7; NULL: s = z */
    float   lambda_dist;                /* weight of the distortion term; 0 skips it */
    float   lambda_ent;                 /* weight of the ray-entropy term; 0 skips it */
    float   acc_min;                    /* a (ray, latent) enters the entropy iff its sum of weights is above this */
    int64_t n_total;                    /* rays the means are taken over; 0 means N */
    float*  d_weights;                  /* [N,S,K] out, required: d reg / d weights, scaled */
    float*  d_z_opt;                    /* [N,S] out or NULL: the direct d reg / d z_vals */
    float*  scalars_out;                /* 8 floats out, 8-byte aligned, required: {reg, dist, ent, frac, 0, 0, 0, 0}; the 32 bytes serve as the
                                           launch's accumulators until it ends */
} cfnerf_ray_reg;

/* The inputs and outputs of a CFNERF_F_KSCORES cfnerf_composite_fwd: a HOST struct of DEVICE pointers and host quantile levels, passed in
 * place of weights_opt; read during the call, not kept. */
typedef struct cfnerf_kscores {
    const float* samples;               /* [M,K] required, row-major */
    const float* target;                /* [M] or NULL; required by rank_code, pit and crps */
    float*   sorted;                    /* [M,K] out or NULL */
    float*   quantiles;                 /* [M,n_levels] out or NULL */
    int32_t* rank_code;                 /* [M] out or NULL: 2 #below + #equal; -1 for a row with a NaN */
    float*   pit;                       /* [M] out or NULL: rank_code / (2K) */
    float*   crps;                      /* [M] out or NULL */
    int32_t  n_levels;                  /* quantile levels, 1..16 (read with quantiles only) */
    int32_t  level_lo[16];              /* floor(q (K-1)), in [0, K-1] */
    float    level_frac[16];            /* q (K-1) - level_lo, in [0, 1) */
} cfnerf_kscores;

/* The inputs and outputs of a CFNERF_MODE_SSIM cfnerf_composite_fwd: a HOST struct of DEVICE pointers and host window parameters, passed
 * in place of weights_opt; read during the call, not kept. */
typedef struct cfnerf_ssim {
    const float* x;                     /* [B,H,W,C] required, channel-last */
    const float* y;                     /* [B,H,W,C] required */
    float*   ssim_map;                  /* [B,H-win+1,W-win+1,C] out or NULL */
    float*   mean;                      /* [B,C] out or NULL; needs scratch */
    float*   scratch;                   /* CFNERF_SSIM_SCRATCH_FLOATS(B,C,H,W,win) floats, 8-byte aligned, or NULL without mean */
    int32_t  H;
    int32_t  W;
    int32_t  win;                       /* taps of the separable window: odd, 3..15 */
    double   cov_norm;                  /* n / (n - 1), n = win^2 (sample covariance, skimage's default) or 1 */
    double   c1;                        /* (0.01 L)^2 */
    double   c2;                        /* (0.03 L)^2 */
    float    taps[15];                  /* the first win are read; used as taps[i] / (their sum) */
} cfnerf_ssim;

CFNERF_API int         cfnerf_version(void);
CFNERF_API const char* cfnerf_last_error(void);

/* ---- parameters ------------------------------------------------------------------------------
 * Parameters live in ONE flat fp32 device buffer owned by the caller, laid out in the order of
 * NeRF_Flows.state_dict() (model/models.py:38-67, 339-350), each tensor
 * row-major as nn.Linear stores it ([out, in]).  cfnerf_param_count / cfnerf_param_offset describe
 * that layout so the host side can map state_dict keys to slices of the buffer.  The same layout
 * is used for gradients and Adam moments, so the multi-GPU exchange is a single all-reduce.      */
CFNERF_API int64_t cfnerf_param_count(const cfnerf_cfg* cfg);
/* offset (in floats) and element count of a state_dict key such as "pts_linears.5.weight"; -1 if unknown */
CFNERF_API int64_t cfnerf_param_offset(const cfnerf_cfg* cfg, const char* key, int64_t* numel);
/* i-th key of the layout (0 <= i < number of tensors), NULL past the end */
CFNERF_API const char* cfnerf_param_key(const cfnerf_cfg* cfg, int index);

/* replaces: create_nerf()'s NeRF_Flows(args) construction, RUN:317-331 (device side only) */
CFNERF_API int cfnerf_model_create(const cfnerf_cfg* cfg, cfnerf_model** out);
CFNERF_API int cfnerf_model_destroy(cfnerf_model* m);
/* (Re)pack the flat parameter buffer into the MFMA-fragment-ordered copies the kernels stream.
 * Call after loading a checkpoint and after every optimiser step.  replaces: the implicit
 * parameter broadcast of nn.DataParallel, RUN:330 */
CFNERF_API int cfnerf_model_set_params(cfnerf_model* m, const float* flat_params, cfnerf_stream s);

/* ---- ray set-up ------------------------------------------------------------------------------
 * replaces: the ray preparation inside render(), RUN:129-158, with get_rays (HLP:288-297) and
 * ndc_rays (HLP:360-377).  Either `rays_o`/`rays_d` ([N,3] each) are given, or (c2w_host != NULL)
 * rays are generated for the N pixels pixel0 .. pixel0+N-1 (row-major) of the H x W image, so ranks can
 * tile an image by rows.  Output `rays` is the [N,11] pack o3,d3,near,far,viewdir3 of RUN:152-158. */
CFNERF_API int cfnerf_rays_setup(int H, int W, float focal, const float* c2w_host /*[3,4] row-major or NULL*/,
                      const float* rays_o, const float* rays_d, int64_t N, int64_t pixel0,
                      int ndc, float near_, float far_, float* rays /*[N,11]*/, cfnerf_stream s);

/* replaces: ndc_rays(H, W, focal, near, rays_o, rays_d) as a standalone call, HLP:360-377 (render() itself goes through
 * cfnerf_rays_setup, which applies it with near = 1 like RUN:149): rays_o, rays_d [N,3] -> out_o, out_d [N,3] in NDC.
 * (get_rays, HLP:288-297, as a standalone call is cfnerf_rays_setup with c2w_host and ndc = 0: columns 0..5 of its output.)   */
CFNERF_API int cfnerf_ndc_rays(int H, int W, float focal, float near_, const float* rays_o, const float* rays_d, int64_t N,
                    float* out_o, float* out_d, cfnerf_stream s);

/* replaces: Embedder.embed / get_embedder(multires) as a standalone call, HLP:21-69:
 * x [P,3] -> out [P, 3 + 6*multires] = [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(L-1) x), cos(2^(L-1) x)]        */
CFNERF_API int cfnerf_embed(const float* x, int64_t P, int multires, float* out, cfnerf_stream s);

/* replaces: the sampling lines of render_rays as a standalone call, RUN:510-534 (used by the unfused query path):
 * rays [N,11], t_vals [S], t_rand [N,S] or NULL, LINDISP flag -> z_vals [N,S], pts [N,S,3]
 * With CFNERF_F_CULL (evaluation only) pts is (float*)&cull of a host struct cfnerf_cull: z_vals [N,S] is written with the bits of the call
 * without the flag (t_rand and CFNERF_F_LINDISP are honoured), and through the struct slot [N,S], ray_start [N+1], the kept points
 * pts_c [P',3] (the bits of the plain call's pts, in (ray, sample) order) and ray_of [P'].  The capacity N * S (< 2^31) always fits: the call
 * cannot overflow.  P' = ray_start[N] is on the device: reading it is one synchronising device-to-host copy per call.  Three launches (count,
 * a scan over the N rays, emit), no atomics.  A NULL struct, a NULL occ_bits, slot, ray_start, pts_c or ray_of, or a res below 1 is refused
 * before anything touches a device.                                                                                                        */
CFNERF_API int cfnerf_sample_points(const float* rays, const float* t_vals, const float* t_rand, int flags, int64_t N, int S,
                         float* z_vals, float* pts, cfnerf_stream s);

/* ---- fused forward ---------------------------------------------------------------------------
 * replaces: render_rays() RUN:457-553 = sampling RUN:510-534, run_network RUN:67-85 with the
 * positional encoding HLP:21-69, NeRF_Flows.forward MOD:188-291 (TriangularSylvesterNeRF
 * MOD:358-416, FLW:189-268) and raw2outputs RUN:411-454, in one launch.
 *   rays    [N,11]          t_vals [S]            t_rand [N,S] or NULL (perturb == 0)
 *   z_vals_opt [N,S] or NULL: explicit sample depths per ray (then t_vals / t_rand are not read: t_vals may be NULL or shorter than S) - used by the
 *                     hierarchical-sampling EXTENSION below, which the reference does not have
 *   eps     [K,4] = (eps_rgb0, eps_rgb1, eps_rgb2, eps_alpha) per latent sample (MOD:234,246 / 198,204);
 *           with CFNERF_F_EPS_ROWS [N,K,4]: row i holds the latents of ray i
 *   rgb_map [N,3,K]  disp_map [N,K]  depth_map [N,K]           (written unless all three are NULL and kstats is given)
 *   raw_opt [N,S,K,4], weights_opt [N,S,K], pts_opt [N,S,3]    (NULL = not wanted)
 *   kstats_opt [N,8]  fused reductions over the K latent samples, what the evaluation loop derives from the
 *                     per-K maps at RUN:1122-1131: mean_K rgb (3) | np.std_K(rgb) * n/(n-1) (3) | mean_K disp | mean_K depth
 *                     with CFNERF_F_KSTATS_EXT [N,12]: columns 0..7 as above, bit for bit, then
 *                       8  uncertainty of disp      9  uncertainty of depth      (the depth-uncertainty maps of the paper's AUSE tables)
 *                       10 mean_K of the accumulated opacity acc_map (RUN:449)    11 its uncertainty
 *                     "uncertainty" is the estimator of columns 3..5: np.std over K (biased) * n/(n-1), RUN:1130
 *   entropy_out [1]   loss_entropy of MOD:286 (TRAIN only, may be NULL otherwise); with CFNERF_F_EPS_ROWS the point-weighted
 *                     mean over the launch (= the mean of the reference's per-netchunk values weighted by their points)
 * With CFNERF_F_GEOMETRY (eval branch): rgb_map must be NULL; disp_map and depth_map [N,K] go together or are both NULL; raw_opt is
 * [N,S,K], the density latent raw[..., 3] alone; weights_opt [N,S,K] and pts_opt as above; kstats_opt is [N,6] =
 *     mean_K disp | mean_K depth | uncertainty of disp | uncertainty of depth | mean_K acc_map | its uncertainty
 * - columns 6..11 of a CFNERF_F_KSTATS_EXT row, bit for bit (K >= 2).  z_vals_opt, CFNERF_F_LINDISP and t_rand behave as above;
 * CFNERF_F_WHITE_BKGD is accepted and has no effect (it only touches colour).  Either the per-K maps or kstats_opt must be requested. */
CFNERF_API int cfnerf_render_fwd(cfnerf_model* m, const float* rays, const float* t_vals, const float* t_rand,
                      const float* z_vals_opt, const float* eps, int64_t N, int S, int K, int flags,
                      float* rgb_map, float* disp_map, float* depth_map,
                      float* raw_opt, float* weights_opt, float* pts_opt, float* kstats_opt, float* entropy_out,
                      cfnerf_stream s);

/* replaces: what the training loop's evaluation block derives from a full-image render (render_path_train RUN:247-314 with
 * RUN:1117-1131: K-mean prediction, np.std * n/(n-1) uncertainty, mean disparity / depth) and the per-pixel integrand of
 * img2mse(rgb_mean, target) (RUN:1028, HLP:15), all reduced INSIDE the fused forward: only 32 (+12) bytes per pixel leave
 * the chip instead of 20*K.  Eval branch (fixed eps, no jitter).  kstats [N,8] as in cfnerf_render_fwd; gt_opt [N,3] and
 * sqerr_opt [N,3] = (K-mean rgb - gt)^2 go together or are both NULL.  eps is always [K,4]: CFNERF_F_EPS_ROWS is refused.
 * With CFNERF_F_KSTATS_EXT kstats is [N,12] (columns as in cfnerf_render_fwd) and sqerr_opt is [N,6]: columns 0..2 the squared error,
 * bit for bit, columns 3..5 the per-channel integrand of the loss's negative log-likelihood (RUN:1034-1042) at that pixel,
 *     h     = torch.std_K(rgb) * n/(n-1) * (0.8/n)^(-1/7) + 1e-5                       (torch.std: UNBIASED, then n/(n-1) on top)
 *     nll_c = -log( mean_K[ exp(-(rgb_k - gt)^2 / (2 h^2)) ] * (2 pi)^(-1.5) / h + 1e-5 )
 * whose mean over pixels and channels is loss_nll of cfnerf_loss_fwd_bwd.  This is the TRAIN loop's estimator with its quirk (the
 * n/(n-1) factor applied to an already unbiased std); it is NOT the estimator of kstats columns 3..5 (np.std, biased, * n/(n-1)).
 * 48 + 24 = 72 (+12 for gt) bytes per pixel instead of 20*K; evaluated with libm expf / logf in every flow-math mode.
 * With CFNERF_F_GEOMETRY kstats is [N,6] (columns as in cfnerf_render_fwd: depth and disparity maps with their uncertainty, 24 bytes per
 * pixel) and gt_opt / sqerr_opt must be NULL. */
CFNERF_API int cfnerf_render_eval(cfnerf_model* m, const float* rays, const float* t_vals, const float* eps, int64_t N, int S, int K,
                       int flags, const float* gt_opt, float* kstats, float* sqerr_opt, cfnerf_stream s);

/* EXTENSION (not in the reference, whose N_importance / network_fine are dead parameters, RUN:467-468; the
 * semantics restated are those of the reference's upstream, yenchenlin/nerf-pytorch sample_pdf): inverse-CDF
 * resampling of N_importance depths per ray from the K-mean of the coarse weights, merged and sorted with the
 * coarse depths.  The coarse depths are recomputed from (rays, t_vals, t_rand, LINDISP flag) exactly as
 * cfnerf_render_fwd samples them.  weights [N,S,K], u [N,N_importance] in [0,1] -> z_out [N,S+N_importance].    */
CFNERF_API int cfnerf_sample_pdf(const float* rays, const float* t_vals, const float* t_rand, int flags, const float* weights,
                      const float* u, int64_t N, int S, int K, int N_importance, float* z_out, cfnerf_stream s);

/* replaces: NeRF_Flows.forward(x, is_val, is_test) MOD:188-291 on pre-embedded inputs x [P,90]
 * (what batchify()/run_network hand to the model, RUN:47-64,82).  raw [P,K,4].  With CFNERF_F_STASH (implies TRAIN) the
 * activations are kept for cfnerf_network_bwd (the model's ONE stash, bound as one "ray" of P samples: size the workspace
 * with cfnerf_workspace_bytes(cfg, 1, P, K)).  eps [K,4]; with CFNERF_F_EPS_ROWS [P,K,4], one row per point (the
 * reference's netchunk boundaries are point boundaries).
 * With CFNERF_F_GEOMETRY (eval branch; what NeRF_Flows.sample MOD:69-96 computes): x keeps its [P,90] stride and its view columns are not
 * read; raw is [P,K], the pre-softplus density latent of every (point, latent) = raw[p,k,3] of the launch without the flag, bit for bit;
 * entropy_out is ignored.                                                                          */
CFNERF_API int cfnerf_network_fwd(cfnerf_model* m, const float* x, const float* eps, int64_t P, int K, int flags,
                       float* raw, float* entropy_out, cfnerf_stream s);

/* replaces: raw2outputs() RUN:411-454 as a standalone call.  raw [N,S,K,4] (16-byte aligned, S * K * 16 bytes per ray < 2 GiB: it is
 * fetched through one buffer descriptor per ray), z_vals [N,S], rays_d [N,3]; any K >= 1, any S >= 1
 * With CFNERF_F_CULL or-ed into white_bkgd (evaluation only; the background is white iff (white_bkgd & ~0x800) != 0) raw is [P',K,4], the rows
 * of the kept samples alone in (ray, sample) order, and weights_opt is (float*)&sp of a host struct cfnerf_sparse_raw naming slot, ray_start
 * and the weights proper.  The maps and weights are, bit for bit, those of the plain call on the dense raw [N,S,K,4] in which every culled
 * sample has the density latent -1e4 (softplus gives exactly 0 there): a culled sample contributes alpha = 0.  Only the sign of slot is
 * read; a ray's rows are fetched through a descriptor of exactly its block [ray_start[ray], ray_start[ray + 1]), so inconsistent indices
 * read zeros, never another ray's rows.  A NULL struct, slot or ray_start is refused.  No backward: cfnerf_composite_bwd does not take the bit.
 * With CFNERF_F_RAY_REG or-ed into white_bkgd nothing is composited: the call evaluates the distortion and ray-entropy regularisers of
 * weights [N,S,K] and their gradient, from (float*)&rr of a host struct cfnerf_ray_reg in weights_opt (contract at the flag).
 * With CFNERF_F_KSCORES or-ed into white_bkgd nothing is composited either: the call sorts and scores the N rows of samples [N,K] as
 * ensembles (quantiles, PIT rank, CRPS), from (float*)&ks of a host struct cfnerf_kscores in weights_opt (contract at the flag).
 * With CFNERF_MODE_SSIM or-ed into white_bkgd nothing is composited either: the call writes the SSIM map and the per-image means of the N
 * image pairs of (float*)&s, a host struct cfnerf_ssim in weights_opt (contract at enum cfnerf_mode). */
CFNERF_API int cfnerf_composite_fwd(const float* raw, const float* z_vals, const float* rays_d,
                         int64_t N, int S, int K, int white_bkgd,
                         float* rgb_map, float* disp_map, float* depth_map, float* weights_opt,
                         cfnerf_stream s);

/* ---- train step ------------------------------------------------------------------------------
 * replaces: the loss lines RUN:1026-1050 (K-mean MSE/PSNR, KDE negative log-likelihood with the
 * detached n/(n-1)-scaled bandwidth, + beta1 * entropy).  Writes d(loss)/d(rgb_map) [N,3,K] and
 * scalars_out[4] = {loss, loss_nll, mse, psnr}.  `n_total` is the GLOBAL ray count the means are
 * taken over (N for one GPU, N * world_size when rays are sharded).  scalars_out must be 8-byte aligned (its
 * 16 bytes double as the two 64-bit fixed-point accumulators of the multi-workgroup reduction).     */
CFNERF_API int cfnerf_loss_fwd_bwd(const float* rgb_map, const float* target, const float* entropy, int64_t N, int K,
                        float beta1, int64_t n_total, float* d_rgb_map, float* scalars_out, cfnerf_stream s);

/* ---- train-step workspace (ownership contract of SURVEY 8b) -------------------------------------
 * Bytes of device memory a CFNERF_F_STASH forward + cfnerf_render_bwd of an (N rays, S samples, K latents) batch
 * need: the activations autograd would have kept for loss.backward() (RUN:1066), the pre-activation gradients
 * and the split-K weight-gradient partials.  -1 on a bad argument.                                               */
CFNERF_API int64_t cfnerf_workspace_bytes(const cfnerf_cfg* cfg, int64_t N, int S, int K);
/* Hand the model a caller-owned block (256-byte aligned, e.g. a torch uint8 tensor) to use as that workspace.  The
 * library then never allocates on the train path: a batch that does not fit is refused with CFNERF_E_NOMEM.  The
 * block must stay alive until the next cfnerf_model_set_workspace / cfnerf_model_destroy.  (NULL, 0) returns to
 * the default, a model-owned block grown on demand.  Any stashed forward is dropped.                            */
CFNERF_API int cfnerf_model_set_workspace(cfnerf_model* m, void* workspace, size_t bytes);
/* Identity of the forward the model's ONE stash currently holds: every CFNERF_F_STASH forward increments it.
 * 0 = no stashed forward.  Read it right after the forward and pass it to cfnerf_render_bwd.                    */
CFNERF_API uint64_t cfnerf_model_stash_generation(const cfnerf_model* m);

/* replaces: loss.backward() (RUN:1066) through raw2outputs, the flows and the MLP for the batch
 * of the cfnerf_render_fwd(... CFNERF_F_STASH ...) whose generation is `stash_generation`; if a later STASH forward
 * has replaced that stash the call fails (CFNERF_E_INVALID) instead of differentiating the wrong batch.
 * d_depth_map may be NULL.  d_entropy points to ONE device float, d(loss)/d(loss_entropy) (e.g. beta1); NULL
 * means 0.  grad_flat [param_count] is OVERWRITTEN with the gradient in the flat parameter layout.  A CFNERF_F_EPS_ROWS
 * forward is differentiated with its per-ray rows, read from the caller's eps buffer (see CFNERF_F_EPS_ROWS).  If the forward carried
 * CFNERF_F_COTANGENTS, d_rgb_map is NOT a device array: it is (const float*)&cot of a host struct cfnerf_cotangents, which adds the cotangents of
 * disp_map, weights and raw (each may be NULL; see the flag).  If the forward carried CFNERF_F_RAY_GRAD, grad_flat is [z_off + N * S] floats and the call also
 * writes d_rays [N,11] from r_off and d_z [N,S] from z_off (layout and columns at CFNERF_F_RAY_GRAD); without it only [0, param_count) is touched.
 * If the forward carried CFNERF_F_EPS_GRAD, grad_flat is [er_off + N * K * 4] floats and the call also writes d_eps [K,4] from e_off and
 * d_eps_rows [N,K,4] from er_off, behind those blocks (layout at CFNERF_F_EPS_GRAD); _accumulate overwrites these two as well. */
CFNERF_API int cfnerf_render_bwd(cfnerf_model* m, uint64_t stash_generation, const float* d_rgb_map, const float* d_depth_map,
                      const float* d_entropy, float* grad_flat, cfnerf_stream s);
/* replaces: the same loss.backward() when ONE optimiser step's batch is walked in slices (the reference renders any N_rand and any
 * `chunk`, RUN:88-100,602: its autograd graph grows with the batch; here the train-step workspace does - 3 MiB per ray at W = 256 -
 * so a batch larger than the workspace the caller wants to lend is cut into equal slices, each rendered with CFNERF_F_STASH and
 * differentiated before the next one replaces the stash).  Exactly cfnerf_render_bwd, except that the slice's gradient is ADDED to
 * grad_flat: call cfnerf_render_bwd for the first slice (it overwrites) and this for the others, with the loss of every slice taken
 * with n_total = the FULL batch (cfnerf_loss_fwd_bwd) and d_entropy = beta1 / n_slices.  The sum over slices is the full batch's
 * gradient up to the summation order (tests/test_hip_train.py: 8 x 1024 rays against one 8192-ray launch).  The early ranges
 * (cfnerf_grad_early_ranges) are final only after the LAST slice's call.  As in cfnerf_render_bwd, the d_rgb_map argument of a
 * CFNERF_F_COTANGENTS stash is (const float*)&cot of a host struct cfnerf_cotangents holding that slice's cotangents.                 */
CFNERF_API int cfnerf_render_bwd_accumulate(cfnerf_model* m, uint64_t stash_generation, const float* d_rgb_map, const float* d_depth_map,
                                 const float* d_entropy, float* grad_flat, cfnerf_stream s);

/* ---- the UNFUSED seam, differentiable like the reference's ---------------------------------------------------------
 * In the reference NeRF_Flows.forward (MOD:188-291) and raw2outputs (RUN:411-454) are ordinary autograd graphs, so a caller
 * that injects its own network_query_fn (RUN:382-394, called at RUN:538) still trains.  These two entry points are the
 * tail of cfnerf_render_bwd split at `raw`, with the same arithmetic.
 *
 * replaces: loss.backward() through NeRF_Flows.forward for the cfnerf_network_fwd(... CFNERF_F_STASH ...) whose generation
 * is `stash_generation`.  d_raw [P,K,4] = d loss / d raw (NULL = zeros), d_entropy = ONE device float, d loss /
 * d loss_entropy (NULL = 0).  grad_flat [param_count] is OVERWRITTEN.  If the forward carried CFNERF_F_INPUT_GRAD, grad_flat is
 * [x_off + P * (input_ch + input_ch_views)] floats, x_off = (cfnerf_param_count(cfg) + 63) / 64 * 64: the parameter gradient in
 * [0, param_count) as before, and d_x [P, input_ch + input_ch_views] = d loss / d x row-major from x_off (exact-fp32 MFMA in both
 * precision modes, no atomics: bit-reproducible); the floats between param_count and x_off are not written.  Without that flag
 * only [0, param_count) is touched.  If the forward carried CFNERF_F_EPS_GRAD, grad_flat is [er_off + P * K * 4] floats and the call also
 * writes d_eps [K,4] from e_off and d_eps_rows [P,K,4] from er_off, behind the blocks above (layout at CFNERF_F_EPS_GRAD).    */
CFNERF_API int cfnerf_network_bwd(cfnerf_model* m, uint64_t stash_generation, const float* d_raw, const float* d_entropy,
                       float* grad_flat, cfnerf_stream s);
/* replaces: loss.backward() through raw2outputs(raw, z_vals, rays_d) RUN:411-454, stateless: the forward is recomputed from
 * raw [N,S,K,4], z_vals [N,S], rays_d [N,3].  d_rgb_map [N,3,K]; d_disp_map [N,K], d_depth_map [N,K], d_weights [N,S,K] may
 * be NULL (= zeros).  Writes d_raw [N,S,K,4] = d loss / d raw.  S <= 4096.
 * With CFNERF_F_SEAM_GRAD or-ed into white_bkgd, d_raw is (float*)&grads of a host struct cfnerf_composite_grads and the call writes
 * whichever of d_raw [N,S,K,4], d_z_vals [N,S] = d loss / d z_vals and d_rays_d [N,3] = d loss / d rays_d it names (see the flag):
 * the distances z_{s+1} - z_s and |rays_d| of RUN:426-429 and depth_map's explicit z (RUN:447); the last interval 1e1 is a constant. */
CFNERF_API int cfnerf_composite_bwd(const float* raw, const float* z_vals, const float* rays_d, int64_t N, int S, int K, int white_bkgd,
                         const float* d_rgb_map, const float* d_disp_map, const float* d_depth_map, const float* d_weights,
                         float* d_raw, cfnerf_stream s);

/* ---- overlap of the multi-GPU gradient exchange with the end of the backward --------------------------------
 * replaces: nothing in the reference (its nn.DataParallel, RUN:330, gathers gradients inside autograd).  Most of
 * grad_flat - every bias, the base Gaussians, and each weight whose gradient comes from the big weight-gradient
 * launches alone - is final BEFORE the small-job launch that ends cfnerf_render_bwd.  cfnerf_grad_early_ranges
 * reports those flat ranges (they depend on the configuration only; available after the first cfnerf_render_bwd);
 * cfnerf_stream_wait_grad_early makes `waiter` (e.g. the communication stream) wait for the event recorded at
 * that point of the LAST cfnerf_render_bwd, so the all-reduce of those ranges runs while the rest still computes.
 * The early point exists from the first cfnerf_render_bwd AFTER a call of cfnerf_grad_early_ranges on (a caller that never asks
 * gets one reduction launch at the end instead of two); before that the event fires when the whole gradient is final - a
 * waiter is always correct, only not early.                                                                                 */
CFNERF_API int cfnerf_grad_early_ranges(cfnerf_model* m, int64_t* offsets, int64_t* counts, int max_ranges);
CFNERF_API int cfnerf_stream_wait_grad_early(cfnerf_model* m, cfnerf_stream waiter);

/* replaces: torch.optim.Adam.step() RUN:339,1067 on the flat buffers (betas .9/.999, eps 1e-8),
 * followed by the re-pack of cfnerf_model_set_params.  step is 1-based.  grad_scale multiplies
 * the gradient first (1/world_size after a sum all-reduce).                                      */
CFNERF_API int cfnerf_adam_step(cfnerf_model* m, float* flat_params, const float* grad_flat, float* exp_avg,
                     float* exp_avg_sq, int64_t step, float lr, float grad_scale, cfnerf_stream s);

/* OPT-IN arithmetic mode of the fused forward's dense layers.  0 (default): exact-fp32 MFMA
 * (v_mfma_f32_32x32x2_f32).  1: "bf16x3" - every fp32 operand is carried as hi + lo bf16 and a product is evaluated
 * as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (the dropped lo*lo term is ~2^-18
 * relative); it is held to the SAME parity tolerances by tests/test_hip_bf16x3.py.  Applies to the fused forward,
 * the backward-data kernel and the large weight-gradient GEMMs (the narrow ones stay exact fp32).  A stashed forward belongs to
 * the mode it ran in: CHANGING the mode drops it (its generation id is retired, like after cfnerf_model_set_workspace).     */
CFNERF_API int cfnerf_model_set_precision(cfnerf_model* m, int mode);

/* Arithmetic of the flow phase of the fused kernels (the K conditional Sylvester flows, MOD:401-413 / FLW:225-268, the activations
 * and the composite, RUN:424-449, of every (point, latent sample)).  1: libm throughout (correctly rounded tanhf / logf / expf /
 * log1pf, IEEE division) - ~1300 vector instructions per (point, latent).  2: the same functions on the hardware transcendentals
 * (v_exp_f32 / v_log_f32 / v_rcp_f32, ~1 ulp each; tanh = 1 - 2 / (1 + e^2x)) - ~250 instructions; held to the same parity bounds
 * by the tests.  0 (default): 1 below 16 latent samples (the reference's plumbing and headline configurations stay on libm bit
 * for bit), 2 from 16 on, where the flow phase grows from 5 % (K = 16) to 20 % (K = 64, the reference's default) of the launch.   */
CFNERF_API int cfnerf_model_set_flow_math(cfnerf_model* m, int mode);

/* bytes currently held by the model: packed weights + the bound workspace, whoever owns it (diagnostics) */
CFNERF_API int64_t cfnerf_model_workspace_bytes(const cfnerf_model* m);

/* Measurement helpers for bench.py: kernel durations from HIP events recorded on the launch stream.
 *   mode 0: off (default).  mode 1: every stage of a step (ten events per train step: costs ~1 % of it).
 *   mode 2: the fused forward launch only (two events per step) - what the timed region of bench.py runs with.
 * cfnerf_timing_fwd_mean_ms: mean duration (ms) of the last min(n, 64) timed fused-forward launches since the mode was set.
 * cfnerf_timing_last_ms: last launch of a stage (stages 1..4 need mode 1).  Both return < 0 when nothing was timed.        */
CFNERF_API int   cfnerf_timing_enable(cfnerf_model* m, int mode);
CFNERF_API float cfnerf_timing_fwd_mean_ms(cfnerf_model* m, int n);
CFNERF_API float cfnerf_timing_last_ms(cfnerf_model* m, int which /*0=fwd 1=bwd_tail 2=bwd_data 3=bwd_dw 4=adam*/);

#ifdef __cplusplus
}
#endif
#endif /* CFNERF_H */
