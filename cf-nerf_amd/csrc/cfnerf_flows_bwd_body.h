// cfnerf_flows_bwd_body.h - the body of flows_bwd_kernel and flows_eps_kernel (cfnerf_tail.hip), included ONCE PER KERNEL between the braces
// of the kernel with CFN_FLOWS_EPS 0 / 1, shared as TEXT like cfnerf_tail_body.h: with CFN_FLOWS_EPS 0 the preprocessor leaves exactly the
// kernel of before, and the compiler emits exactly its code.
// CFN_FLOWS_EPS 1 (CFNERF_F_EPS_GRAD of a points stash; the kernel runs BESIDE flows_bwd_kernel and writes nothing that one writes - see
// cfnerf_tail_body.h for why): lane = point, so the lane holds d loss / d z0 of every latent of its point by itself and writes the point's
// [K,4] row of d_eps_rows (`eps_out` [P,K,4]): the chain through z0 = eps std + mean plus the point's share of the
// base log-normal's direct term (MOD:268,283,286: -d_entropy eps / (K P) = cE eps, a colour latent a third of it).
#pragma clang fp contract(fast)
    const int lane = lane_id_opaque(), wave = wave_id();
    const int64_t pi = (int64_t)blockIdx.x * kThreads + wave * 64 + lane;
    const bool valid = pi < P;
    const int64_t p = valid ? pi : 0;
    const float cE = -((d_ent != nullptr) ? d_ent[0] : 0.f) / (float)((double)P * (double)K);
    const float a_mean = flat[0], a_std = flat[1];
    const float r_mean[3] = {flat[2], flat[3], flat[4]};
    const float r_std[3] = {flat[5], flat[6], flat[7]};
    float th[84], gms[8];
    GReg gth;
    const float* const e_pt = eps_rows ? eps + p * K * 4 : eps;            // CFNERF_F_EPS_ROWS: this point's [K,4] row
    {
        const f32x4* tp = reinterpret_cast<const f32x4*>(theta + p * kThetaAll);
#pragma unroll
        for (int q = 0; q < 18; ++q) { const f32x4 v = tp[q]; th[q * 4] = v[0]; th[q * 4 + 1] = v[1]; th[q * 4 + 2] = v[2]; th[q * 4 + 3] = v[3]; }
#pragma unroll
        for (int q = 0; q < 3; ++q) { const f32x4 v = tp[kThetaRgb / 4 + q]; th[72 + q * 4] = v[0]; th[73 + q * 4] = v[1]; th[74 + q * 4] = v[2]; th[75 + q * 4] = v[3]; }
    }
    gth.clear();
#pragma unroll
    for (int i = 0; i < 8; ++i) gms[i] = 0.f;
    for (int k = 0; k < K; ++k) {
        const f32x4 rv = *reinterpret_cast<const f32x4*>(raw + (((p >> 6) * K + k) * 64 + (p & 63)) * 4);    // tile-transposed stash: [tile p / 64][k][row p % 64][4]
        f32x4 g; g[0] = g[1] = g[2] = g[3] = 0.f;
        if (d_raw != nullptr) g = *reinterpret_cast<const f32x4*>(d_raw + (p * K + k) * 4);
        const f32x4 e = *reinterpret_cast<const f32x4*>(e_pt + k * 4);
        const float c0 = t_sigmoid(rv[0]), c1 = t_sigmoid(rv[1]), c2 = t_sigmoid(rv[2]), sg = t_sigmoid(rv[3]);
        float ga = g[3] + cE * (1.f - sg);                                     // + d(-mean(a - softplus a))  MOD:263
        float gz[3] = {g[0] + cE * (1.f - 2.f * c0), g[1] + cE * (1.f - 2.f * c1), g[2] + cE * (1.f - 2.f * c2)};   // MOD:278
        if (!valid) { ga = 0.f; gz[0] = gz[1] = gz[2] = 0.f; }
#if CFN_FLOWS_EPS
        float gl[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) gl[i] = 0.f;
        flows_adjoint(th, gth, gl, e, a_mean, a_std, r_mean, r_std, ga, gz, cE, valid);
        // (gl[0] = d z0 of the density latent, gl[2..4] of the colour latents)
        if (valid) {
            f32x4 o;
            o[0] = gl[2] * r_std[0] + cE * (1.f / 3.f) * e[0];
            o[1] = gl[3] * r_std[1] + cE * (1.f / 3.f) * e[1];
            o[2] = gl[4] * r_std[2] + cE * (1.f / 3.f) * e[2];
            o[3] = gl[0] * a_std + cE * e[3];
            *reinterpret_cast<f32x4*>(eps_out + (p * K + k) * 4) = o;
        }
#else
        flows_adjoint(th, gth, gms, e, a_mean, a_std, r_mean, r_std, ga, gz, cE, valid);
#endif
    }
#if !CFN_FLOWS_EPS
    if (valid) store_gtheta_row(g_theta + p * kThetaAll, th, gth);
#pragma unroll
    for (int i = 0; i < 8; ++i) gms[i] = wave_sum(gms[i]);
    if (lane == 0) {
        const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
#pragma unroll
        for (int i = 0; i < 8; ++i) gms_partials[row * 8 + i] = gms[i];
    }
#endif
