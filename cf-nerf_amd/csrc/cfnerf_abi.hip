// cfnerf_abi.hip - the extern "C" boundary of libcfnerf_hip.so (see include/cfnerf.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "cfnerf_kernels.h"
#include "cfnerf_model.h"

using namespace cfnerf;

static thread_local char g_err[512] = "";

int cfnerf::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// device-side part of cfnerf_model_create; on failure the caller destroys the partially built handle
static int model_init_device(cfnerf_model* m) {
    const cfnerf_cfg* cfg = &m->cfg;
    HIPCHK(hipGetDevice(&m->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, m->device));
    m->n_cu = prop.multiProcessorCount;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CFNERF_E_UNSUPPORTED, "device is %s; this library is built for gfx950 (MI355X) only", prop.gcnArchName);
    const size_t pbytes = (size_t)m->plan.tab.packed_floats * sizeof(float);
    HIPCHK(hipMalloc(&m->d_packed, pbytes));
    HIPCHK(hipMemset(m->d_packed, 0, pbytes));
    HIPCHK(hipMalloc(&m->d_packed16, (size_t)m->plan.tab.packed16_elems * 2));
    HIPCHK(hipMemset(m->d_packed16, 0, (size_t)m->plan.tab.packed16_elems * 2));
    HIPCHK(hipMalloc(&m->d_descs, m->plan.descs.size() * sizeof(PackDesc)));
    HIPCHK(hipMemcpy(m->d_descs, m->plan.descs.data(), m->plan.descs.size() * sizeof(PackDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&m->d_pack_table, (size_t)m->plan.total_elems * 3 * sizeof(uint32_t)));
    HIPCHK(launch_pack_index(m->d_descs, (int)m->plan.descs.size(), m->plan.total_elems, m->d_pack_table, nullptr));
    HIPCHK(hipDeviceSynchronize());
    m->ent_cap = fused_fwd_max_grid(cfg->netwidth, cfg->h_alpha_size, m->n_cu);
    HIPCHK(hipMalloc(&m->d_ent_partials, (size_t)m->ent_cap * 2 * sizeof(float)));
    HIPCHK(hipMalloc(&m->d_enc_scratch, (size_t)m->ent_cap * kTileM * 64 * sizeof(float)));
    HIPCHK(hipMalloc(&m->d_eps, kMaxK * 4 * sizeof(float)));
    for (int i = 0; i < kFwdRing; ++i) {
        HIPCHK(hipEventCreate(&m->fr0[i]));
        HIPCHK(hipEventCreate(&m->fr1[i]));
    }
    for (int i = 0; i < kNumTimers; ++i) {
        HIPCHK(hipEventCreate(&m->ev0[i]));
        HIPCHK(hipEventCreate(&m->ev1[i]));
    }
    m->ws_bytes = pbytes + sizeof(NetTab);
    // launch attributes and occupancy belong to (kernel, device): set here, with the model's device current
    HIPCHK(fused_fwd_set_attributes(cfg->netwidth, cfg->h_alpha_size, &m->fwd_blocks_per_cu));
    HIPCHK(bwd_set_attributes(cfg->netwidth, cfg->h_alpha_size));
    return CFNERF_OK;
}

size_t cfnerf::workspace_bytes_for(const cfnerf_cfg& c, int64_t n, int s, int k) {
    return Stash::carve(nullptr, nullptr, c, n, s, k, build_layout(c).total);
}

static int flow_math_bits(const cfnerf_model* m) {
    return m->flow_math == 0 ? 0 : (CFNERF_F_FLOW_MATH_SET | (m->flow_math == 2 ? CFNERF_F_FLOW_MATH_FAST : 0));
}

// Point the stash at its block for an (N,S,K) batch.  A caller-provided block (cfnerf_model_set_workspace) is never
// grown: too small is an error.  A model-owned block is (re)allocated here - the only place the train path allocates.
static int stash_bind(cfnerf_model* m, int64_t n, int s, int k) {
    Stash& q = m->stash;
    if (q.base && q.bound_N == n && q.bound_S == s && q.bound_K == k) return CFNERF_OK;
    const size_t need = Stash::carve(nullptr, nullptr, m->cfg, n, s, k, m->layout.total);
    if (need > q.cap) {
        if (q.base && !q.owned)
            return fail(CFNERF_E_NOMEM, "the workspace handed to cfnerf_model_set_workspace holds %zu bytes but N=%lld S=%d K=%d needs %zu "
                        "(size it with cfnerf_workspace_bytes)", q.cap, (long long)n, s, k, need);
        if (hipDeviceSynchronize() != hipSuccess) return fail(CFNERF_E_HIP, "hipDeviceSynchronize failed");
        q.release();
        void* p = nullptr;
        if (hipMalloc(&p, need) != hipSuccess)
            return fail(CFNERF_E_NOMEM, "workspace allocation of %zu bytes failed (N=%lld S=%d K=%d)", need, (long long)n, s, k);
        q.base = static_cast<char*>(p); q.cap = need; q.owned = true;
    }
    q.used = Stash::carve(&q, q.base, m->cfg, n, s, k, m->layout.total);
    q.bound_N = n; q.bound_S = s; q.bound_K = k;
    q.valid = false;
    ++q.bind_serial;
    return CFNERF_OK;
}

// The arguments every fused forward launch shares: the weights, the flag word and - for a STASH launch - the model's one stash,
// bound for (n, s) (a cfnerf_network_fwd launch binds it as ONE "ray" of P samples, `points`) and handed to this forward: its
// streams, the Q4 layout decision and a new generation (older backward passes are refused).
static int forward_args(cfnerf_model* m, FwdArgs& a, int flags, int64_t n, int s, int K, bool points) {
    a.wp = m->d_packed; a.wp16 = m->d_packed16; a.flat = m->flat;
    a.K = K; a.flags = (flags & 0xffff & ~(CFNERF_F_INPUT_GRAD | CFNERF_F_RAY_GRAD | CFNERF_F_COTANGENTS | CFNERF_F_EPS_GRAD)) | flow_math_bits(m);      // (INPUT_GRAD / RAY_GRAD / COTANGENTS / EPS_GRAD are the backward's business: Stash::flags)
    if (!(flags & CFNERF_F_STASH)) return CFNERF_OK;
    if (int rc = stash_bind(m, n, s, K)) return rc;
    Stash& q = m->stash;
    a.st_enc = q.enc; a.st_gd = q.gd; a.st_h = q.h; a.st_feat = q.feat; a.st_v = q.v; a.st_ha = q.ha; a.st_hr = q.hr;
    a.st_theta = q.theta;
    a.st_mbits = reinterpret_cast<uint32_t*>(q.mbits);
    q.n_tiles = n * (int64_t)((s + kTileM - 1) / kTileM);
    a.n_tiles = q.n_tiles;
    a.st_raw = q.raw;                    // the backward reads the model's OWN (tile-transposed) copy: the caller may drop its tensor,
                                         // and a caller's raw is written by the same launch (rounds 1-4: a device-to-device copy after it)
    q.N = n; q.S = s; q.K = K; q.flags = flags; q.valid = true; q.points = points;
    q.eps_rows = (flags & CFNERF_F_EPS_ROWS) ? a.eps : nullptr;
    q.q4 = (s % kTileM == 0) && m->precision == 0;      // whole tiles, fp32 mode: the wide streams take the Q4 layout (cfnerf_device.h)
    a.q4 = q.q4;
    ++q.generation;
    return CFNERF_OK;
}

// the train branch of cfnerf_render_fwd / cfnerf_network_fwd: STASH implies TRAIN (written to `flags`), TRAIN needs entropy_out, rows are train-only
static int train_flags(int& flags, const float* entropy_out) {
    if (flags & CFNERF_F_STASH) flags |= CFNERF_F_TRAIN;
    if ((flags & CFNERF_F_TRAIN) && !entropy_out) return fail(CFNERF_E_INVALID, "TRAIN needs entropy_out");
    if ((flags & CFNERF_F_EPS_ROWS) && !(flags & CFNERF_F_TRAIN))
        return fail(CFNERF_E_INVALID, "CFNERF_F_EPS_ROWS is a train-branch mode (the eval branch uses the fixed [K,4] latents)");
    return CFNERF_OK;
}

// ... and the launch that ends it: the entropy over n * s points; with STASH also the backward's copies of a ray launch's `rays` and of a [K,4] set
static int finish_train_fwd(cfnerf_model* m, int grid, const float* eps, int64_t n, int s, int K, int flags, const float* rays, float* entropy_out, hipStream_t st) {
    const bool keep = flags & CFNERF_F_STASH, rows = flags & CFNERF_F_EPS_ROWS;
    HIPCHK(launch_entropy_finalize(m->d_ent_partials, grid, m->flat, eps, K, (double)n * s * K, entropy_out, (keep && !rows) ? m->d_eps : nullptr,
                                   rays, (keep && rays) ? m->stash.rays : nullptr, rays ? n * 11 : 0, rows ? n : 0, s, st));
    return CFNERF_OK;
}

// the fused forward of a ray launch, between the timing events of cfnerf_timing_enable
static int timed_fused_fwd(cfnerf_model* m, const FwdArgs& a, bool train, hipStream_t st, int* grid, int mode = 0) {
    if (m->timing) HIPCHK(hipEventRecord(m->fr0[m->fwd_launches % kFwdRing], st));
    HIPCHK(launch_fused_fwd(a, m->plan.tab, mode, train, m->precision, m->n_cu, m->fwd_blocks_per_cu, st, grid));
    if (m->timing) { HIPCHK(hipEventRecord(m->fr1[m->fwd_launches % kFwdRing], st)); ++m->fwd_launches; }
    return CFNERF_OK;
}

// a handle lives on the device that was current when it was created (one handle per device, one process per GPU)
static int check_device(const cfnerf_model* m) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != m->device)
        return fail(CFNERF_E_INVALID, "model lives on device %d but the current device is %d (hipSetDevice / torch.cuda.set_device first)",
                    m->device, dev);
    return CFNERF_OK;
}

// Flags that only some entry points implement: CFNERF_F_KSTATS_EXT widens the kstats / sqerr rows of the two render entry points,
// CFNERF_F_GEOMETRY selects the geometry-only launch of the three fused-forward entry points, CFNERF_F_INPUT_GRAD asks the backward of
// a cfnerf_network_fwd stash for d loss / d x, CFNERF_F_RAY_GRAD the backward of a cfnerf_render_fwd stash for d loss / d rays and d loss / d z_vals,
// CFNERF_F_COTANGENTS makes the backward of a cfnerf_render_fwd stash read its d_rgb_map argument as a host cfnerf_cotangents,
// CFNERF_F_SEAM_GRAD belongs to the white_bkgd argument of cfnerf_composite_bwd alone, CFNERF_F_CULL turns the pts argument of
// cfnerf_sample_points into a host cfnerf_cull (and travels in the white_bkgd argument of cfnerf_composite_fwd), CFNERF_F_EPS_GRAD asks the
// backward of a cfnerf_render_fwd / cfnerf_network_fwd stash for d loss / d eps, CFNERF_F_RAY_REG belongs to the white_bkgd argument of
// cfnerf_composite_fwd alone (the ray regularisers of a cfnerf_ray_reg), and so do CFNERF_F_KSCORES (the ensemble scores of a cfnerf_kscores)
// and CFNERF_MODE_SSIM (the image similarity of a cfnerf_ssim; an enum of its own, the same argument).
// Anywhere else they would be silently ignored: `allowed` holds those of them that `who` takes.
static int refuse_mode_flags(int flags, int allowed, const char* who) {
    if (flags & CFNERF_F_KSTATS_EXT & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_KSTATS_EXT (it widens kstats / sqerr of cfnerf_render_eval and cfnerf_render_fwd)", who);
    if (flags & CFNERF_F_GEOMETRY & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_GEOMETRY (the geometry-only launch of cfnerf_network_fwd, cfnerf_render_fwd and cfnerf_render_eval)", who);
    if (flags & CFNERF_F_INPUT_GRAD & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_INPUT_GRAD (the input gradient of cfnerf_network_fwd with CFNERF_F_STASH, written by cfnerf_network_bwd)", who);
    if (flags & CFNERF_F_RAY_GRAD & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_RAY_GRAD (the ray gradient of cfnerf_render_fwd with CFNERF_F_STASH, written by cfnerf_render_bwd)", who);
    if (flags & CFNERF_F_COTANGENTS & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_COTANGENTS (the cotangent descriptor of cfnerf_render_fwd with CFNERF_F_STASH, read by cfnerf_render_bwd)", who);
    if (flags & CFNERF_F_SEAM_GRAD)                     // (no entry point with a `flags` argument takes it)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_SEAM_GRAD (d_z_vals / d_rays_d of cfnerf_composite_bwd, passed in its white_bkgd argument)", who);
    if (flags & CFNERF_F_CULL & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_CULL (the occupancy-grid descriptor of cfnerf_sample_points; cfnerf_composite_fwd takes the bit in its white_bkgd argument)", who);
    if (flags & CFNERF_F_EPS_GRAD & ~allowed)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_EPS_GRAD (the latent gradient of cfnerf_render_fwd / cfnerf_network_fwd with CFNERF_F_STASH, written by their backward)", who);
    if (flags & CFNERF_F_RAY_REG)                       // (no entry point with a `flags` argument takes it)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_RAY_REG (the ray regularisers of cfnerf_composite_fwd, passed in its white_bkgd argument)", who);
    if (flags & CFNERF_F_KSCORES)                       // (no entry point with a `flags` argument takes it)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_F_KSCORES (the ensemble scores of cfnerf_composite_fwd, passed in its white_bkgd argument)", who);
    if (flags & CFNERF_MODE_SSIM)                       // (no entry point with a `flags` argument takes it)
        return fail(CFNERF_E_INVALID, "%s does not take CFNERF_MODE_SSIM (the image similarity of cfnerf_composite_fwd, passed in its white_bkgd argument)", who);
    return CFNERF_OK;
}

// the host descriptor of a CFNERF_F_CULL cfnerf_sample_points, checked before anything touches a device
static int check_cull(const cfnerf_cull* c) {
    if (!c) return fail(CFNERF_E_INVALID, "CFNERF_F_CULL: the pts argument must be (float*)&cull of a host struct cfnerf_cull, got NULL");
    static const char* const names[] = {"occ_bits", "slot", "ray_start", "pts_c", "ray_of"};
    const void* const ptrs[] = {c->occ_bits, c->slot, c->ray_start, c->pts_c, c->ray_of};
    for (int i = 0; i < 5; ++i)
        if (!ptrs[i]) return fail(CFNERF_E_INVALID, "CFNERF_F_CULL: member %s of cfnerf_cull is NULL", names[i]);
    for (int d = 0; d < 3; ++d)
        if (c->res[d] < 1) return fail(CFNERF_E_INVALID, "CFNERF_F_CULL: member res[%d] of cfnerf_cull is %d (every axis needs at least 1 cell)", d, c->res[d]);
    return CFNERF_OK;
}

// CFNERF_F_GEOMETRY is an eval-branch launch of its own kernel: no train branch, no stash, one latent set, its own [N,6] statistics
static int check_geometry_flags(int flags) {
    static const struct { int bit; const char* name; } bad[] = {{CFNERF_F_TRAIN, "CFNERF_F_TRAIN"}, {CFNERF_F_STASH, "CFNERF_F_STASH"},
                                                                {CFNERF_F_EPS_ROWS, "CFNERF_F_EPS_ROWS"}, {CFNERF_F_KSTATS_EXT, "CFNERF_F_KSTATS_EXT"},
                                                                {CFNERF_F_INPUT_GRAD, "CFNERF_F_INPUT_GRAD"}, {CFNERF_F_RAY_GRAD, "CFNERF_F_RAY_GRAD"},
                                                                {CFNERF_F_COTANGENTS, "CFNERF_F_COTANGENTS"}, {CFNERF_F_EPS_GRAD, "CFNERF_F_EPS_GRAD"}};
    for (const auto& b : bad)
        if (flags & b.bit)
            return fail(CFNERF_E_INVALID, "CFNERF_F_GEOMETRY is an eval-branch launch without the colour branch: it cannot be combined with %s", b.name);
    return CFNERF_OK;
}

// CFNERF_F_RAY_REG in the white_bkgd argument of cfnerf_composite_fwd: everything is checked by name before anything touches a device
static int composite_ray_reg(const float* raw, const float* z_vals, const float* rays_d, int64_t N, int S, int K, int white_bkgd, const float* rgb_map,
                             const float* disp_map, const float* depth_map, const cfnerf_ray_reg* rr, hipStream_t st) {
    if (white_bkgd & CFNERF_F_CULL)
        return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG cannot be combined with CFNERF_F_CULL (the regularisers read a dense weights [N,S,K])");
    if (!rr) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: the weights_opt argument must be (float*)&rr of a host struct cfnerf_ray_reg, got NULL");
    const struct { const void* p; const char* name; } banned[] = {{raw, "raw"}, {rays_d, "rays_d"}, {rgb_map, "rgb_map"}, {disp_map, "disp_map"},
                                                                  {depth_map, "depth_map"}};
    for (const auto& b : banned)
        if (b.p) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: the %s argument must be NULL (nothing is composited)", b.name);
    if (!z_vals) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: the z_vals argument is NULL");
    if (!rr->weights) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: member weights of cfnerf_ray_reg is NULL");
    if (!rr->d_weights) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: member d_weights of cfnerf_ray_reg is NULL");
    if (!rr->scalars_out) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: member scalars_out of cfnerf_ray_reg is NULL");
    if (reinterpret_cast<uintptr_t>(rr->scalars_out) % 8)
        return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: member scalars_out of cfnerf_ray_reg must be 8-byte aligned");
    if (S < 1) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: S must be at least 1, got %d", S);
    if (K < 1) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: K must be at least 1, got %d", K);
    if (N < 0) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: N must not be negative, got %lld", (long long)N);
    if (S > 4096 || K > kMaxK) return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_RAY_REG: S must be in [1,4096] and K in [1,%d], got S=%d K=%d", kMaxK, S, K);
    if (rr->n_total < 0) return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_REG: member n_total of cfnerf_ray_reg is negative");
    const int64_t n_total = rr->n_total ? rr->n_total : N;
    RayRegArgs a{};
    a.w = rr->weights; a.z = z_vals; a.rays = rr->rays; a.dw = rr->d_weights; a.dz = rr->d_z_opt; a.scalars = rr->scalars_out;
    a.acc = reinterpret_cast<unsigned long long*>(rr->scalars_out + 2);
    a.N = N; a.S = S; a.K = K;
    a.inv = n_total > 0 ? 1.0 / ((double)n_total * K) : 0.0;
    a.cd = (float)((double)rr->lambda_dist * a.inv); a.ce = (float)((double)rr->lambda_ent * a.inv);
    a.lambda_dist = rr->lambda_dist; a.lambda_ent = rr->lambda_ent; a.acc_min = rr->acc_min;
    HIPCHK(launch_ray_reg(a, st));
    return CFNERF_OK;
}

// CFNERF_F_KSCORES in the white_bkgd argument of cfnerf_composite_fwd: everything is checked by name before anything touches a device
static int composite_kscores(const float* raw, const float* z_vals, const float* rays_d, int64_t N, int S, int K, int white_bkgd, const float* rgb_map,
                             const float* disp_map, const float* depth_map, const cfnerf_kscores* ks, hipStream_t st) {
    if (white_bkgd & CFNERF_F_CULL)
        return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES cannot be combined with CFNERF_F_CULL (nothing is composited: the rows of samples [N,K] are scored)");
    if (white_bkgd & CFNERF_F_RAY_REG)
        return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES cannot be combined with CFNERF_F_RAY_REG (each selects a mode of its own, with its own struct in weights_opt)");
    if (!ks) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: the weights_opt argument must be (float*)&ks of a host struct cfnerf_kscores, got NULL");
    const struct { const void* p; const char* name; } banned[] = {{raw, "raw"}, {z_vals, "z_vals"}, {rays_d, "rays_d"}, {rgb_map, "rgb_map"},
                                                                  {disp_map, "disp_map"}, {depth_map, "depth_map"}};
    for (const auto& b : banned)
        if (b.p) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: the %s argument must be NULL (nothing is composited)", b.name);
    if (!ks->samples) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: member samples of cfnerf_kscores is NULL");
    if (!ks->sorted && !ks->quantiles && !ks->rank_code && !ks->pit && !ks->crps)
        return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: no output requested (sorted, quantiles, rank_code, pit and crps of cfnerf_kscores are all NULL)");
    const struct { const void* p; const char* name; } scored[] = {{ks->crps, "crps"}, {ks->pit, "pit"}, {ks->rank_code, "rank_code"}};
    for (const auto& o : scored)
        if (o.p && !ks->target) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: member %s of cfnerf_kscores needs member target, which is NULL", o.name);
    if (S != 1) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: S must be 1 (the rows are samples [N,K]), got %d", S);
    if (K < 1) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: K must be at least 1, got %d", K);
    if (K > kMaxK) return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_KSCORES: K must be at most %d, got %d", kMaxK, K);
    if (N < 0) return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: N must not be negative, got %lld", (long long)N);
    KScoresArgs a{};
    if (ks->quantiles) {
        if (ks->n_levels < 1 || ks->n_levels > 16)
            return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: member n_levels of cfnerf_kscores must be in [1,16] with quantiles, got %d", ks->n_levels);
        for (int t = 0; t < ks->n_levels; ++t) {
            if (ks->level_lo[t] < 0 || ks->level_lo[t] > K - 1)
                return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: member level_lo[%d] of cfnerf_kscores is %d, outside [0, K-1] = [0, %d]", t, ks->level_lo[t], K - 1);
            if (!(ks->level_frac[t] >= 0.f && ks->level_frac[t] < 1.f))
                return fail(CFNERF_E_INVALID, "CFNERF_F_KSCORES: member level_frac[%d] of cfnerf_kscores is %g, outside [0, 1)", t, (double)ks->level_frac[t]);
            a.level_lo[t] = ks->level_lo[t];
            a.level_frac[t] = ks->level_frac[t];
        }
        a.Q = ks->n_levels;
    }
    a.samples = ks->samples; a.target = ks->target; a.sorted = ks->sorted; a.quantiles = ks->quantiles;
    a.rank_code = ks->rank_code; a.pit = ks->pit; a.crps = ks->crps;
    a.M = N; a.K = K;
    HIPCHK(launch_k_scores(a, st));
    return CFNERF_OK;
}

// CFNERF_MODE_SSIM in the white_bkgd argument of cfnerf_composite_fwd: everything is checked by name before anything touches a device
static int composite_ssim(const float* raw, const float* z_vals, const float* rays_d, int64_t N, int S, int K, int white_bkgd, const float* rgb_map,
                          const float* disp_map, const float* depth_map, const cfnerf_ssim* ss, hipStream_t st) {
    const struct { int bit; const char* name; } modes[] = {{CFNERF_F_CULL, "CFNERF_F_CULL"}, {CFNERF_F_RAY_REG, "CFNERF_F_RAY_REG"},
                                                           {CFNERF_F_KSCORES, "CFNERF_F_KSCORES"}};
    for (const auto& o : modes)
        if (white_bkgd & o.bit)
            return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM cannot be combined with %s (each selects a mode of its own, with its own struct in weights_opt)", o.name);
    if (!ss) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: the weights_opt argument must be (float*)&s of a host struct cfnerf_ssim, got NULL");
    const struct { const void* p; const char* name; } banned[] = {{raw, "raw"}, {z_vals, "z_vals"}, {rays_d, "rays_d"}, {rgb_map, "rgb_map"},
                                                                  {disp_map, "disp_map"}, {depth_map, "depth_map"}};
    for (const auto& b : banned)
        if (b.p) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: the %s argument must be NULL (nothing is composited)", b.name);
    if (!ss->x) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member x of cfnerf_ssim is NULL");
    if (!ss->y) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member y of cfnerf_ssim is NULL");
    if (!ss->ssim_map && !ss->mean) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: no output requested (ssim_map and mean of cfnerf_ssim are both NULL)");
    if (ss->mean && !ss->scratch) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member mean of cfnerf_ssim needs member scratch, which is NULL");
    if (ss->mean && reinterpret_cast<uintptr_t>(ss->scratch) % 8)
        return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member scratch of cfnerf_ssim must be 8-byte aligned (it holds doubles)");
    if (S != 1) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: S must be 1 (N images of K channels), got %d", S);
    if (K < 1 || K > 4) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: K (the channel count) must be in [1,4], got %d", K);
    if (N < 0) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: N must not be negative, got %lld", (long long)N);
    const int win = ss->win;
    if (win < 3 || win > kSsimMaxWin || win % 2 == 0)
        return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member win of cfnerf_ssim must be odd and in [3,%d], got %d", kSsimMaxWin, win);
    if (ss->H < win) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member H of cfnerf_ssim is %d, below win = %d (the valid interior is empty)", ss->H, win);
    if (ss->W < win) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member W of cfnerf_ssim is %d, below win = %d (the valid interior is empty)", ss->W, win);
    const struct { double v; const char* name; } positive[] = {{ss->cov_norm, "cov_norm"}, {ss->c1, "c1"}, {ss->c2, "c2"}};
    for (const auto& q : positive)
        if (!(q.v > 0.) || !std::isfinite(q.v))
            return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member %s of cfnerf_ssim must be finite and positive, got %g", q.name, q.v);
    SsimArgs a{};
    double tsum = 0.;
    for (int i = 0; i < win; ++i) {
        if (!std::isfinite(ss->taps[i])) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member taps[%d] of cfnerf_ssim is not finite", i);
        tsum += (double)ss->taps[i];
    }
    if (!(tsum > 0.)) return fail(CFNERF_E_INVALID, "CFNERF_MODE_SSIM: member taps of cfnerf_ssim must sum to a positive number, got %g", tsum);
    for (int i = 0; i < win; ++i) a.taps[i] = (double)ss->taps[i] / tsum;
    a.tiles_y = (ss->H - win) / kSsimTile + 1; a.tiles_x = (ss->W - win) / kSsimTile + 1;
    if ((double)N * K * a.tiles_y * a.tiles_x > 2147483647.)
        return fail(CFNERF_E_UNSUPPORTED, "CFNERF_MODE_SSIM: N * K * tiles = %lld * %d * %d * %d workgroups, above 2^31 - 1: split the batch", (long long)N, K, a.tiles_y, a.tiles_x);
    a.x = ss->x; a.y = ss->y; a.map = ss->ssim_map; a.mean = ss->mean;
    a.partials = ss->mean ? reinterpret_cast<double*>(ss->scratch) : nullptr;
    a.B = N; a.C = K; a.H = ss->H; a.W = ss->W; a.win = win;
    a.cov_norm = ss->cov_norm; a.c1 = ss->c1; a.c2 = ss->c2;
    HIPCHK(launch_ssim(a, st));
    return CFNERF_OK;
}

extern "C" int cfnerf_model_destroy(cfnerf_model* m);

extern "C" {

int cfnerf_version(void) { return 100; }
const char* cfnerf_last_error(void) { return g_err; }

int64_t cfnerf_param_count(const cfnerf_cfg* cfg) {
    if (!cfg) { fail(CFNERF_E_INVALID, "cfg is NULL"); return -1; }
    if (const char* why = validate_cfg(*cfg)) { fail(CFNERF_E_UNSUPPORTED, "%s", why); return -1; }
    return build_layout(*cfg).total;
}

int64_t cfnerf_param_offset(const cfnerf_cfg* cfg, const char* key, int64_t* numel) {
    if (!cfg || !key) { fail(CFNERF_E_INVALID, "NULL argument"); return -1; }
    if (const char* why = validate_cfg(*cfg)) { fail(CFNERF_E_UNSUPPORTED, "%s", why); return -1; }
    ParamLayout L = build_layout(*cfg);
    const ParamEntry* e = L.find(key);
    if (!e) { fail(CFNERF_E_INVALID, "unknown parameter key '%s'", key); return -1; }
    if (numel) *numel = e->numel();
    return e->off;
}

const char* cfnerf_param_key(const cfnerf_cfg* cfg, int index) {
    static thread_local std::string key;
    if (!cfg || validate_cfg(*cfg)) return nullptr;
    ParamLayout L = build_layout(*cfg);
    if (index < 0 || index >= (int)L.e.size()) return nullptr;
    key = L.e[index].key;
    return key.c_str();
}

int cfnerf_model_create(const cfnerf_cfg* cfg, cfnerf_model** out) {
    if (!cfg || !out) return fail(CFNERF_E_INVALID, "NULL argument");
    if (const char* why = validate_cfg(*cfg)) return fail(CFNERF_E_UNSUPPORTED, "%s", why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CFNERF_E_HIP, "no HIP device visible: the CF-NeRF hot path has no CPU fallback");
    cfnerf_model* m = new (std::nothrow) cfnerf_model();
    if (!m) return fail(CFNERF_E_NOMEM, "host allocation failed");
    m->cfg = *cfg;
    m->layout = build_layout(*cfg);
    m->plan = build_pack_plan(*cfg, m->layout);
    const int rc = model_init_device(m);
    if (rc != CFNERF_OK) {                 // g_err already says why; release whatever was allocated
        cfnerf_model_destroy(m);
        return rc;
    }
    *out = m;
    return CFNERF_OK;
}

int cfnerf_model_destroy(cfnerf_model* m) {
    if (!m) return CFNERF_OK;
    hipDeviceSynchronize();
    hipFree(m->d_packed); hipFree(m->d_packed16); hipFree(m->d_descs); hipFree(m->d_pack_table); hipFree(m->d_ent_partials);
    hipFree(m->d_enc_scratch);
    hipFree(m->d_eps);
    m->stash.release();
    m->bwd.release();
    for (int i = 0; i < kNumTimers; ++i) { if (m->ev0[i]) hipEventDestroy(m->ev0[i]); if (m->ev1[i]) hipEventDestroy(m->ev1[i]); }
    for (int i = 0; i < kFwdRing; ++i) { if (m->fr0[i]) hipEventDestroy(m->fr0[i]); if (m->fr1[i]) hipEventDestroy(m->fr1[i]); }
    delete m;
    return CFNERF_OK;
}

int cfnerf_model_set_params(cfnerf_model* m, const float* flat_params, cfnerf_stream s) {
    if (!m || !flat_params) return fail(CFNERF_E_INVALID, "NULL argument");
    if (int rc = check_device(m)) return rc;
    m->flat = flat_params;
    // the split-bf16 copy is only refreshed while the opt-in mode is selected
    HIPCHK(launch_pack(flat_params, m->d_packed, m->precision ? m->d_packed16 : nullptr, m->d_pack_table, m->plan.total_elems, (hipStream_t)s));
    return CFNERF_OK;
}

int cfnerf_rays_setup(int H, int W, float focal, const float* c2w_host, const float* rays_o, const float* rays_d,
                      int64_t N, int64_t pixel0, int ndc, float near_, float far_, float* rays, cfnerf_stream s) {
    if (!rays || N < 0) return fail(CFNERF_E_INVALID, "bad rays/N");
    if (N == 0) return CFNERF_OK;
    RaysC2W c{};
    if (c2w_host) {
        if (pixel0 < 0 || pixel0 + N > (int64_t)H * W)
            return fail(CFNERF_E_INVALID, "c2w given: pixels [%lld, %lld) exceed H*W = %lld", (long long)pixel0, (long long)(pixel0 + N), (long long)H * W);
        std::memcpy(c.m, c2w_host, sizeof c.m);
    } else if (!rays_o || !rays_d) {
        return fail(CFNERF_E_INVALID, "either c2w_host or rays_o/rays_d must be given");
    }
    HIPCHK(launch_rays_setup(H, W, focal, c, c2w_host ? 1 : 0, rays_o, rays_d, N, pixel0, ndc, near_, far_, rays, (hipStream_t)s));
    return CFNERF_OK;
}

int cfnerf_ndc_rays(int H, int W, float focal, float near_, const float* rays_o, const float* rays_d, int64_t N, float* out_o, float* out_d,
                    cfnerf_stream s) {
    if (N < 0 || H < 1 || W < 1) return fail(CFNERF_E_INVALID, "bad N/H/W");
    if (N == 0) return CFNERF_OK;
    if (!rays_o || !rays_d || !out_o || !out_d) return fail(CFNERF_E_INVALID, "NULL argument");
    HIPCHK(launch_ndc_rays(H, W, focal, near_, rays_o, rays_d, N, out_o, out_d, (hipStream_t)s));
    return CFNERF_OK;
}

int cfnerf_embed(const float* x, int64_t P, int multires, float* out, cfnerf_stream s) {
    if (P < 0 || multires < 1 || multires > 16) return fail(CFNERF_E_INVALID, "bad P / multires (1..16)");
    if (P == 0) return CFNERF_OK;
    if (!x || !out) return fail(CFNERF_E_INVALID, "NULL argument");
    HIPCHK(launch_embed(x, P, multires, out, (hipStream_t)s));
    return CFNERF_OK;
}

int cfnerf_sample_points(const float* rays, const float* t_vals, const float* t_rand, int flags, int64_t N, int S, float* z_vals,
                         float* pts, cfnerf_stream s) {
    if (int rc = refuse_mode_flags(flags, CFNERF_F_CULL, "cfnerf_sample_points")) return rc;
    if (flags & CFNERF_F_CULL) {                 // pts is a host cfnerf_cull: z_vals + the keep / skip decisions + the compact point list
        const cfnerf_cull* c = reinterpret_cast<const cfnerf_cull*>(pts);
        if (int rc = check_cull(c)) return rc;
        if (N < 0 || S < 1) return fail(CFNERF_E_INVALID, "bad N/S");
        if (N * (int64_t)S > 0x7fffffff) return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_CULL: N * S must stay below 2^31 (slot holds 32-bit rows)");
        if (N > 0 && (!rays || !t_vals || !z_vals)) return fail(CFNERF_E_INVALID, "NULL argument");
        CullArgs a{};
        a.rays = rays; a.t_vals = t_vals; a.t_rand = t_rand; a.occ_bits = c->occ_bits;
        for (int d = 0; d < 3; ++d) { a.lo[d] = c->lo[d]; a.scale[d] = c->scale[d]; a.res[d] = c->res[d]; }
        a.outside = c->outside != 0; a.lindisp = (flags & CFNERF_F_LINDISP) != 0; a.S = S; a.N = N;
        a.z_vals = z_vals; a.slot = c->slot; a.ray_start = c->ray_start; a.pts_c = c->pts_c; a.ray_of = c->ray_of;
        HIPCHK(launch_cull(a, (hipStream_t)s));  // (N == 0: ray_start[0] = 0)
        return CFNERF_OK;
    }
    if (N < 0 || S < 1) return fail(CFNERF_E_INVALID, "bad N/S");
    if (N == 0) return CFNERF_OK;
    if (!rays || !t_vals || !z_vals) return fail(CFNERF_E_INVALID, "NULL argument");
    HIPCHK(launch_sample_points(rays, t_vals, t_rand, flags, N, S, z_vals, pts, (hipStream_t)s));
    return CFNERF_OK;
}

static int check_common(cfnerf_model* m, int K) {
    if (!m) return fail(CFNERF_E_INVALID, "model is NULL");
    if (!m->flat) return fail(CFNERF_E_INVALID, "cfnerf_model_set_params has not been called");
    if (int rc = check_device(m)) return rc;
    if (K < 1 || K > kMaxK) return fail(CFNERF_E_UNSUPPORTED, "K_samples must be in [1,%d], got %d", kMaxK, K);
    return CFNERF_OK;
}

int cfnerf_render_fwd(cfnerf_model* m, const float* rays, const float* t_vals, const float* t_rand, const float* z_vals_opt,
                      const float* eps, int64_t N, int S, int K, int flags, float* rgb_map, float* disp_map, float* depth_map,
                      float* raw_opt, float* weights_opt, float* pts_opt, float* kstats_opt, float* entropy_out, cfnerf_stream s) {
    if (int rc = check_common(m, K)) return rc;
    if (N < 0 || S < 1) return fail(CFNERF_E_INVALID, "bad N/S");
    if (int rc = refuse_mode_flags(flags, CFNERF_F_KSTATS_EXT | CFNERF_F_GEOMETRY | CFNERF_F_RAY_GRAD | CFNERF_F_COTANGENTS | CFNERF_F_EPS_GRAD, "cfnerf_render_fwd")) return rc;
    if (flags & CFNERF_F_EPS_GRAD) {
        if (flags & CFNERF_F_GEOMETRY)
            return fail(CFNERF_E_INVALID, "CFNERF_F_EPS_GRAD cannot be combined with CFNERF_F_GEOMETRY (a geometry-only launch keeps no stash to differentiate)");
        if (!(flags & CFNERF_F_STASH))
            return fail(CFNERF_E_INVALID, "CFNERF_F_EPS_GRAD needs CFNERF_F_STASH (d loss / d eps is written by cfnerf_render_bwd from the stashed forward)");
        if (flags & CFNERF_F_KSTATS_EXT)
            return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_EPS_GRAD cannot be combined with CFNERF_F_KSTATS_EXT (evaluation metrics: render without a stash)");
    }
    if (flags & CFNERF_F_COTANGENTS) {
        if (flags & CFNERF_F_GEOMETRY)
            return fail(CFNERF_E_INVALID, "CFNERF_F_COTANGENTS cannot be combined with CFNERF_F_GEOMETRY (a geometry-only launch keeps no stash to differentiate)");
        if (!(flags & CFNERF_F_STASH))
            return fail(CFNERF_E_INVALID, "CFNERF_F_COTANGENTS needs CFNERF_F_STASH (the cotangent descriptor is read by cfnerf_render_bwd of the stashed forward)");
        if (flags & CFNERF_F_KSTATS_EXT)
            return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_COTANGENTS cannot be combined with CFNERF_F_KSTATS_EXT (evaluation metrics: render without a stash)");
    }
    if (flags & CFNERF_F_RAY_GRAD) {
        if (flags & CFNERF_F_GEOMETRY)
            return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_GRAD cannot be combined with CFNERF_F_GEOMETRY (a geometry-only launch keeps no stash to differentiate)");
        if (!(flags & CFNERF_F_STASH))
            return fail(CFNERF_E_INVALID, "CFNERF_F_RAY_GRAD needs CFNERF_F_STASH (d loss / d rays and d loss / d z_vals are written by cfnerf_render_bwd from the stashed forward)");
        if (flags & CFNERF_F_KSTATS_EXT)
            return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_RAY_GRAD cannot be combined with CFNERF_F_KSTATS_EXT (evaluation metrics: render without a stash)");
    }
    if (N == 0) return CFNERF_OK;            // empty batch: nothing to do (buffers may be NULL)
    if (!rays || !eps || (!t_vals && !z_vals_opt)) return fail(CFNERF_E_INVALID, "NULL argument");
    const bool geom = flags & CFNERF_F_GEOMETRY;
    if (geom) {
        if (int rc = check_geometry_flags(flags)) return rc;
        if (rgb_map) return fail(CFNERF_E_INVALID, "CFNERF_F_GEOMETRY computes no colour: rgb_map must be NULL");
        if ((disp_map == nullptr) != (depth_map == nullptr)) return fail(CFNERF_E_INVALID, "CFNERF_F_GEOMETRY: disp_map and depth_map must be given together");
    }
    const bool maps = geom ? (disp_map && depth_map) : (rgb_map && disp_map && depth_map);
    if (!geom && !maps && (rgb_map || disp_map || depth_map)) return fail(CFNERF_E_INVALID, "rgb_map/disp_map/depth_map must be given together");
    if (!maps && !kstats_opt) return fail(CFNERF_E_INVALID, "either the per-K maps or kstats_opt must be requested");
    if (kstats_opt && K < 2) return fail(CFNERF_E_INVALID, "kstats needs K >= 2 (std * n/(n-1))%s", geom ? " - also the [N,6] rows of CFNERF_F_GEOMETRY" : "");
    hipStream_t st = (hipStream_t)s;
    if (int rc = train_flags(flags, entropy_out)) return rc;
    if (flags & CFNERF_F_KSTATS_EXT) {
        if (!kstats_opt) return fail(CFNERF_E_INVALID, "CFNERF_F_KSTATS_EXT needs kstats_opt (it widens its rows to 12 floats)");
        if (flags & (CFNERF_F_STASH | CFNERF_F_EPS_ROWS))
            return fail(CFNERF_E_UNSUPPORTED, "CFNERF_F_KSTATS_EXT is not built for CFNERF_F_STASH / CFNERF_F_EPS_ROWS launches (evaluation metrics: render without a stash, one latent set)");
    }
    const bool train = flags & CFNERF_F_TRAIN;
    FwdArgs a{};
    // Explicit depths: the caller's sample table is not read (cfnerf.h: it may be NULL, or - the hierarchical extension's coarse table under a fine
    // pass - shorter than S).  fused_fwd_kernel still issues its three table loads at index s < S before it discards them, which read past a
    // shorter table (a memory-access fault whenever that table ends its allocation's last mapped page): it is handed the first row of z_vals_opt
    // instead, S readable floats whose values go unused.  The geometry kernel does not load at all.
    a.rays = rays; a.t_vals = z_vals_opt ? z_vals_opt : t_vals; a.t_rand = z_vals_opt ? nullptr : t_rand; a.z_in = z_vals_opt; a.eps = eps;
    a.N = N; a.S = S; a.P = N * (int64_t)S;
    a.rgb_map = rgb_map; a.disp = disp_map; a.depth = depth_map;
    a.raw = raw_opt; a.weights = weights_opt; a.pts = pts_opt; a.kstats = kstats_opt;
    a.ent_partials = train ? m->d_ent_partials : nullptr;
    a.enc_scratch = m->d_enc_scratch;
    const bool keep = flags & CFNERF_F_STASH;
    if (keep && !maps) return fail(CFNERF_E_INVALID, "STASH needs the per-K maps");
    if (int rc = forward_args(m, a, flags, N, S, K, false)) return rc;
    if (keep) { a.st_z = m->stash.z; a.st_at = m->stash.at; }
    // (with STASH the backward's own copies of the step's rays and latents are written by finish_train_fwd - the forward reads the caller's)
    int grid = 0;
    if (int rc = timed_fused_fwd(m, a, train, st, &grid)) return rc;
    return train ? finish_train_fwd(m, grid, eps, N, S, K, flags, rays, entropy_out, st) : CFNERF_OK;
}

int cfnerf_render_eval(cfnerf_model* m, const float* rays, const float* t_vals, const float* eps, int64_t N, int S, int K, int flags,
                       const float* gt_opt, float* kstats, float* sqerr_opt, cfnerf_stream s) {
    if (int rc = check_common(m, K)) return rc;
    if (N < 0 || S < 1) return fail(CFNERF_E_INVALID, "bad N/S");
    if (int rc = refuse_mode_flags(flags, CFNERF_F_KSTATS_EXT | CFNERF_F_GEOMETRY, "cfnerf_render_eval")) return rc;
    if (N == 0) return CFNERF_OK;
    if (!rays || !eps || !t_vals || !kstats) return fail(CFNERF_E_INVALID, "NULL argument");
    const bool geom = flags & CFNERF_F_GEOMETRY;
    if (geom) {
        if (int rc = check_geometry_flags(flags)) return rc;
        if (gt_opt || sqerr_opt) return fail(CFNERF_E_INVALID, "CFNERF_F_GEOMETRY computes no colour: gt_opt and sqerr_opt must be NULL");
    }
    if (K < 2) return fail(CFNERF_E_INVALID, "kstats needs K >= 2 (std * n/(n-1))%s", geom ? " - also the [N,6] rows of CFNERF_F_GEOMETRY" : "");
    if ((gt_opt == nullptr) != (sqerr_opt == nullptr)) return fail(CFNERF_E_INVALID, "gt_opt and sqerr_opt must be given together");
    if (flags & (CFNERF_F_TRAIN | CFNERF_F_STASH)) return fail(CFNERF_E_INVALID, "cfnerf_render_eval is the eval branch only");
    if (flags & CFNERF_F_EPS_ROWS)
        return fail(CFNERF_E_INVALID, "cfnerf_render_eval uses the fixed [K,4] eval latents: CFNERF_F_EPS_ROWS (per-ray latent rows) is a train-branch mode");
    FwdArgs a{};
    a.rays = rays; a.t_vals = t_vals; a.eps = eps;
    a.N = N; a.S = S; a.P = N * (int64_t)S;
    a.kstats = kstats; a.gt = gt_opt; a.sqerr = sqerr_opt; a.enc_scratch = m->d_enc_scratch;
    if (int rc = forward_args(m, a, flags, N, S, K, false)) return rc;
    int grid = 0;
    return timed_fused_fwd(m, a, false, (hipStream_t)s, &grid);
}

int cfnerf_sample_pdf(const float* rays, const float* t_vals, const float* t_rand, int flags, const float* weights, const float* u,
                      int64_t N, int S, int K, int N_importance, float* z_out, cfnerf_stream s) {
    if (int rc = refuse_mode_flags(flags, 0, "cfnerf_sample_pdf")) return rc;
    if (N < 0 || S < 3 || K < 1 || N_importance < 1) return fail(CFNERF_E_INVALID, "bad N/S/K/N_importance (S >= 3)");
    if (S + N_importance > 1024) return fail(CFNERF_E_UNSUPPORTED, "S + N_importance must be <= 1024");
    if (N == 0) return CFNERF_OK;
    if (!rays || !t_vals || !weights || !u || !z_out) return fail(CFNERF_E_INVALID, "NULL argument");
    HIPCHK(launch_sample_pdf(rays, t_vals, t_rand, flags, weights, u, N, S, K, N_importance, z_out, (hipStream_t)s));
    return CFNERF_OK;
}

int cfnerf_network_fwd(cfnerf_model* m, const float* x, const float* eps, int64_t P, int K, int flags, float* raw,
                       float* entropy_out, cfnerf_stream s) {
    if (int rc = check_common(m, K)) return rc;
    const bool geom = flags & CFNERF_F_GEOMETRY;
    if (geom) if (int rc = check_geometry_flags(flags)) return rc;
    if (int rc = refuse_mode_flags(flags, CFNERF_F_GEOMETRY | CFNERF_F_INPUT_GRAD | CFNERF_F_EPS_GRAD, "cfnerf_network_fwd")) return rc;
    if ((flags & CFNERF_F_EPS_GRAD) && !(flags & CFNERF_F_STASH))
        return fail(CFNERF_E_INVALID, "CFNERF_F_EPS_GRAD needs CFNERF_F_STASH (d loss / d eps is written by cfnerf_network_bwd from the stashed forward)");
    if ((flags & CFNERF_F_INPUT_GRAD) && !(flags & CFNERF_F_STASH))
        return fail(CFNERF_E_INVALID, "CFNERF_F_INPUT_GRAD needs CFNERF_F_STASH (d loss / d x is written by cfnerf_network_bwd from the stashed forward)");
    if (P < 0 || P > 0x7fffffff) return fail(CFNERF_E_INVALID, "bad P");
    if (P == 0) return CFNERF_OK;
    if (!x || !eps || !raw) return fail(CFNERF_E_INVALID, "NULL argument");
    if (int rc = train_flags(flags, entropy_out)) return rc;
    const bool train = flags & CFNERF_F_TRAIN;
    hipStream_t st = (hipStream_t)s;
    FwdArgs a{};
    a.eps = eps; a.x = x; a.P = P; a.N = 0; a.S = 1; a.raw = raw;
    a.ent_partials = train ? m->d_ent_partials : nullptr;
    if (int rc = forward_args(m, a, flags, 1, (int)P, K, true)) return rc;      // points-mode stash: ONE "ray" of P samples
    int grid = 0;
    if (geom) return timed_fused_fwd(m, a, false, st, &grid, 1);      // (timed like a ray launch: tools/ab_geometry.py)
    HIPCHK(launch_fused_fwd(a, m->plan.tab, 1, train, m->precision, m->n_cu, m->fwd_blocks_per_cu, st, &grid));
    return train ? finish_train_fwd(m, grid, eps, P, 1, K, flags, nullptr, entropy_out, st) : CFNERF_OK;
}

int cfnerf_composite_fwd(const float* raw, const float* z_vals, const float* rays_d, int64_t N, int S, int K,
                         int white_bkgd, float* rgb_map, float* disp_map, float* depth_map, float* weights_opt,
                         cfnerf_stream s) {
    if (white_bkgd & CFNERF_MODE_SSIM)           // nothing is composited: weights_opt is a host cfnerf_ssim, N image pairs of K channels
        return composite_ssim(raw, z_vals, rays_d, N, S, K, white_bkgd, rgb_map, disp_map, depth_map,
                              reinterpret_cast<const cfnerf_ssim*>(weights_opt), (hipStream_t)s);
    if (white_bkgd & CFNERF_F_KSCORES)           // nothing is composited: weights_opt is a host cfnerf_kscores, N rows of K samples
        return composite_kscores(raw, z_vals, rays_d, N, S, K, white_bkgd, rgb_map, disp_map, depth_map,
                                 reinterpret_cast<const cfnerf_kscores*>(weights_opt), (hipStream_t)s);
    if (white_bkgd & CFNERF_F_RAY_REG)           // nothing is composited: weights_opt is a host cfnerf_ray_reg
        return composite_ray_reg(raw, z_vals, rays_d, N, S, K, white_bkgd, rgb_map, disp_map, depth_map,
                                 reinterpret_cast<const cfnerf_ray_reg*>(weights_opt), (hipStream_t)s);
    if (white_bkgd & CFNERF_F_CULL) {            // raw is [P',K,4], weights_opt a host cfnerf_sparse_raw; white iff (white_bkgd & ~0x800) != 0
        const cfnerf_sparse_raw* sp = reinterpret_cast<const cfnerf_sparse_raw*>(weights_opt);
        if (!sp) return fail(CFNERF_E_INVALID, "CFNERF_F_CULL: the weights_opt argument must be (float*)&sp of a host struct cfnerf_sparse_raw, got NULL");
        if (!sp->slot) return fail(CFNERF_E_INVALID, "CFNERF_F_CULL: member slot of cfnerf_sparse_raw is NULL");
        if (!sp->ray_start) return fail(CFNERF_E_INVALID, "CFNERF_F_CULL: member ray_start of cfnerf_sparse_raw is NULL");
        if (N < 0 || S < 1 || K < 1) return fail(CFNERF_E_INVALID, "bad N/S/K");
        if (N == 0) return CFNERF_OK;
        // (raw may be NULL: P' = 0 leaves nothing to read - every descriptor is then empty)
        if (!z_vals || !rays_d || !rgb_map || !disp_map || !depth_map) return fail(CFNERF_E_INVALID, "NULL argument");
        if ((int64_t)S * K * 16 >= (1ll << 31)) return fail(CFNERF_E_UNSUPPORTED, "cfnerf_composite_fwd: S * K * 16 bytes per ray must stay below 2 GiB");
        HIPCHK(launch_composite_sparse(raw, sp->slot, sp->ray_start, z_vals, rays_d, N, S, K, (white_bkgd & ~CFNERF_F_CULL) != 0, rgb_map, disp_map,
                                       depth_map, sp->weights_opt, (hipStream_t)s));
        return CFNERF_OK;
    }
    if (N < 0 || S < 1 || K < 1) return fail(CFNERF_E_INVALID, "bad N/S/K");
    if (N == 0) return CFNERF_OK;
    if (!raw || !z_vals || !rays_d || !rgb_map || !disp_map || !depth_map) return fail(CFNERF_E_INVALID, "NULL argument");
    if ((int64_t)S * K * 16 >= (1ll << 31)) return fail(CFNERF_E_UNSUPPORTED, "cfnerf_composite_fwd: S * K * 16 bytes per ray must stay below 2 GiB");
    HIPCHK(launch_composite(raw, z_vals, rays_d, N, S, K, white_bkgd, rgb_map, disp_map, depth_map, weights_opt, (hipStream_t)s));
    return CFNERF_OK;
}

int cfnerf_model_set_precision(cfnerf_model* m, int mode) {
    if (!m) return fail(CFNERF_E_INVALID, "model is NULL");
    if (mode != 0 && mode != 1) return fail(CFNERF_E_INVALID, "precision mode must be 0 (fp32 MFMA) or 1 (bf16x3 split MFMA)");
    const bool need_pack16 = mode != 0 && m->precision == 0 && m->flat != nullptr;
    if (mode != m->precision && m->stash.valid) {      // a stashed forward belongs to the mode it ran in (operand copies, the layout of its wide streams): its
        m->stash.valid = false;                         // backward in the other mode would read it wrongly - dropped like a re-bound workspace
        ++m->stash.generation;
    }
    m->precision = mode;
    if (need_pack16) {      // bring the bf16 copy up to date with the current parameters (rare call: fully synchronous)
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(launch_pack(m->flat, m->d_packed, m->d_packed16, m->d_pack_table, m->plan.total_elems, nullptr));
        HIPCHK(hipDeviceSynchronize());
    }
    return CFNERF_OK;
}

int cfnerf_model_set_flow_math(cfnerf_model* m, int mode) {
    if (!m) return fail(CFNERF_E_INVALID, "model is NULL");
    if (mode < 0 || mode > 2) return fail(CFNERF_E_INVALID, "flow math mode must be 0 (auto), 1 (libm) or 2 (hardware transcendentals)");
    m->flow_math = mode;
    return CFNERF_OK;
}

int64_t cfnerf_model_workspace_bytes(const cfnerf_model* m) { return m ? (int64_t)(m->ws_bytes + m->stash.cap) : 0; }

int64_t cfnerf_workspace_bytes(const cfnerf_cfg* cfg, int64_t N, int S, int K) {
    if (!cfg) { fail(CFNERF_E_INVALID, "cfg is NULL"); return -1; }
    if (const char* why = validate_cfg(*cfg)) { fail(CFNERF_E_UNSUPPORTED, "%s", why); return -1; }
    if (K < 1 || K > kMaxK) { fail(CFNERF_E_UNSUPPORTED, "K_samples must be in [1,%d], got %d", kMaxK, K); return -1; }
    if (N < 0 || S < 1) { fail(CFNERF_E_INVALID, "bad N/S"); return -1; }
    return (int64_t)workspace_bytes_for(*cfg, N, S, K);
}

int cfnerf_model_set_workspace(cfnerf_model* m, void* workspace, size_t bytes) {
    if (!m) return fail(CFNERF_E_INVALID, "model is NULL");
    if ((workspace == nullptr) != (bytes == 0)) return fail(CFNERF_E_INVALID, "workspace and bytes must both be given or both be 0");
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(CFNERF_E_INVALID, "workspace must be 256-byte aligned");
    if (int rc = check_device(m)) return rc;
    Stash& q = m->stash;
    if (q.owned && q.base) HIPCHK(hipDeviceSynchronize());      // kernels may still use the block about to be freed
    q.release();                                                // frees a model-owned block; forgets a caller-owned one
    if (workspace) { q.base = static_cast<char*>(workspace); q.cap = bytes; q.owned = false; }
    return CFNERF_OK;
}

uint64_t cfnerf_model_stash_generation(const cfnerf_model* m) { return (m && m->stash.valid) ? m->stash.generation : 0; }

int cfnerf_timing_enable(cfnerf_model* m, int mode) {
    if (!m) return fail(CFNERF_E_INVALID, "model is NULL");
    if (mode < 0 || mode > 2) return fail(CFNERF_E_INVALID, "timing mode must be 0 (off), 1 (every stage) or 2 (fused forward only)");
    m->timing = mode;
    m->fwd_launches = 0;
    return CFNERF_OK;
}

float cfnerf_timing_fwd_mean_ms(cfnerf_model* m, int n) {
    if (!m || !m->timing || n < 1 || m->fwd_launches == 0) return -1.f;
    const uint64_t have = m->fwd_launches < (uint64_t)kFwdRing ? m->fwd_launches : (uint64_t)kFwdRing;
    const uint64_t take = (uint64_t)n < have ? (uint64_t)n : have;
    double sum = 0;
    for (uint64_t i = 0; i < take; ++i) {
        const int slot = (int)((m->fwd_launches - 1 - i) % kFwdRing);
        float ms = 0.f;
        if (hipEventSynchronize(m->fr1[slot]) != hipSuccess) return -1.f;
        if (hipEventElapsedTime(&ms, m->fr0[slot], m->fr1[slot]) != hipSuccess) return -1.f;
        sum += ms;
    }
    return (float)(sum / (double)take);
}

float cfnerf_timing_last_ms(cfnerf_model* m, int which) {
    if (!m || which < 0 || which >= kNumTimers || !m->timing) return -1.f;
    if (which == 0) return cfnerf_timing_fwd_mean_ms(m, 1);
    if (m->timing != 1) return -1.f;
    float ms = -1.f;
    if (hipEventSynchronize(m->ev1[which]) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, m->ev0[which], m->ev1[which]) != hipSuccess) return -1.f;
    return ms;
}

}  // extern "C"

// ---- train-step entry points: implemented in cfnerf_bwd.hip -------------------------------------
