// Host side of the C ABI: the charge-aware seq2seq Aether (s2s_charges.h) -- plan, fused step (also as the decoder on given
// logits), device rollout, the encoder's per-time-step features and the staged field query.  Included by aether_hip.hip inside its extern "C" block; not a stand-alone source file.

namespace {

// The plan: the plain model's (S2SPlanLayout, its filter image EA + 4 features wide) and behind it the chargeless slices of
// the widened layers, the folded filter bank (the image's source) with its bias, and the bias tables.
struct S2SChargePlan {
    S2SPlanLayout P;
    size_t w0s, res1s, p1s[4], in_s[3], w2f, b2f, t_f0, t_res1, t_g[3], t_p1[4], total;
    S2SChargePlan(int D, int he, int hd, int K, int R, int prior_layers, int ph)
        : P(D, he, hd, K, R, prior_layers, ph, -1, 0, S2SDims(D).EA + 4) {
        const S2SDims d(D);
        size_t off = P.total;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        w0s = take((size_t)he * he);
        res1s = take((size_t)he * d.RF);
        for (int k = 0; k < 4; ++k) p1s[k] = take(k < K ? (size_t)hd * d.EA : 0);
        for (int g = 0; g < 3; ++g) in_s[g] = take((size_t)hd * d.RF);
        w2f = take((size_t)(d.EA + 4) * he * he);
        b2f = take((size_t)(d.EA + 4) * he);
        t_f0 = take((size_t)3 * he);
        t_res1 = take((size_t)3 * he);
        for (int g = 0; g < 3; ++g) t_g[g] = take((size_t)3 * hd);
        for (int k = 0; k < 4; ++k) t_p1[k] = take(k < K ? (size_t)4 * hd : 0);
        total = off;
    }
};

// The step's workspace: the plain step's and behind it the index arrays and the edge features with the indicator columns.
struct S2SChargeWs {
    size_t nidx, nscale, eidx, ea, total;
    S2SChargeWs(int D, size_t base_total, int64_t Nn, int64_t E) {
        size_t off = align_up(base_total, 256);
        auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
        nidx = take((size_t)Nn * 4);
        nscale = take((size_t)Nn * 4);
        eidx = take((size_t)E * 4);
        ea = take((size_t)E * (S2SDims(D).EA + 4) * 4);
        total = off;
    }
};

size_t s2s_charges_plan_size(int D, int he, int hd, int R, int prior_layers, int ph, int K) {
    if (s2s_plan_size(D, he, hd, R, prior_layers, ph, K, -1) == 0) return 0;
    return S2SChargePlan(D, he, hd, K, R, prior_layers, ph).total;
}

// The parameter structs the step works on: the caller's, with the widened layers replaced by their chargeless slices in the
// plan (the step reads the other tensors where the caller has them).
struct S2SChargeView {
    AetherS2SFieldParams fp;
    AetherS2SPriorParams pp;
    AetherS2SDecoderParams dp;
    S2SChargeArgs chg;
    S2SChargeView(const AetherS2SFieldParams* f, const AetherS2SPriorParams* p, const AetherS2SDecoderParams* q, const char* plan,
                  const S2SChargePlan& C, int K) : fp(*f), pp(*p), dp(*q), chg{} {
        auto pl = [&](size_t off) { return reinterpret_cast<const float*>(plan + off); };
        fp.w0 = pl(C.w0s);
        pp.res1_w = pl(C.res1s); pp.filt_w2 = pl(C.w2f); pp.filt_b2 = pl(C.b2f);
        for (int k = 0; k < K; ++k) dp.pmsg_fc1_w[k] = pl(C.p1s[k]);
        dp.input_r_w = pl(C.in_s[0]); dp.input_i_w = pl(C.in_s[1]); dp.input_n_w = pl(C.in_s[2]);
        chg.t_f0 = pl(C.t_f0); chg.t_res1 = pl(C.t_res1);
        chg.t_gr = pl(C.t_g[0]); chg.t_gi = pl(C.t_g[1]); chg.t_gn = pl(C.t_g[2]);
        for (int k = 0; k < K; ++k) chg.t_p1[k] = pl(C.t_p1[k]);
        chg.b2 = pl(C.b2f);
    }
};

int s2s_charges_check(const char* what, const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp,
                      const AetherS2SDecoderParams* dp, const void* plan, const S2SSizes& z, bool pointers, int burn_in_steps,
                      int steps) {
    if (!fp) return s2s_fail(AETHER_EINVAL, what, "null pointer");           // (the charge-aware field query is built in)
    return s2s_entry_check(what, false, fp, pp, dp, nullptr, plan, z, true, pointers, burn_in_steps, steps);
}

// What an entry call works on: the view of the caller's structs, the step's arguments on it (built once, from the charge plan's
// layout) and, after prepare(), the index arrays in the workspace (one launch per entry call).
struct S2SChargeCall {
    S2SChargePlan C;
    S2SChargeView view;
    S2SStepArgs a;
    S2SChargeCall(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp, const void* plan,
                  const S2SSizes& z, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr)
        : C(z.D, z.he, z.hd, z.K, z.R, z.prior_layers, z.ph), view(fp, pp, dp, (const char*)plan, C, z.K),
          a{z, &view.fp, &view.pp, &view.dp, nullptr, (const char*)plan, send, recv, order, rowptr, true, C.P,
            S2SStepLayout(z.D, z.he, z.hd, z.R, z.ph, z.K, z.Nn, z.E)} {}
    S2SChargeCall(const S2SChargeCall&) = delete;              // (a points into view)
    int prepare(const char* what, const int32_t* charge_index, void* workspace, size_t workspace_bytes, hipStream_t st) {
        const S2SChargeWs W(a.D, a.L.total, a.Nn, a.E);
        if (workspace_bytes < W.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
        char* ws = (char*)workspace;
        int32_t* nidx = reinterpret_cast<int32_t*>(ws + W.nidx);
        int32_t* eidx = reinterpret_cast<int32_t*>(ws + W.eidx);
        float* nscale = reinterpret_cast<float*>(ws + W.nscale);
        const int64_t items = a.Nn > a.E ? a.Nn : a.E;
        k_s2s_charge_index<<<dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st>>>(charge_index, a.Nn, a.send, a.recv, a.E, nidx,
                                                                                     nscale, eidx, async_error_word());
        view.chg.nidx = nidx; view.chg.nscale = nscale; view.chg.eidx = eidx; view.chg.ea = reinterpret_cast<float*>(ws + W.ea);
        a.chg = &view.chg;
        return AETHER_OK;
    }
};

}  // namespace

size_t aether_s2s_charges_plan_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                     int prior_hidden, int num_edge_types) {
    return s2s_charges_plan_size(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types);
}

int aether_s2s_charges_plan_build(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                                  const float* charge_embedding, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden,
                                  int prior_layers, int prior_hidden, int num_edge_types, void* plan, size_t plan_bytes,
                                  void* stream) {
    if (!fp || !pp || !dp || !charge_embedding || !plan) return fail(AETHER_EINVAL, "s2s_charges_plan_build: null pointer");
    const int D = num_dims, he = encoder_hidden, hd = decoder_hidden, K = num_edge_types;
    if (int rc = s2s_plan_buffer_check("s2s_charges_plan_build",
                                       s2s_charges_plan_size(D, he, hd, rnn_hidden, prior_layers, prior_hidden, K), plan, plan_bytes))
        return rc;
    const S2SChargePlan C(D, he, hd, K, rnn_hidden, prior_layers, prior_hidden);
    const S2SDims d(D);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)plan;
    auto fl = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    const float* emb = charge_embedding;
    // chargeless slices of the widened layers (row strides: + 16 / + 32 embedding columns)
    auto slice = [&](const float* W, int cols, int ld, size_t off, int rows) {
        k_s2s_pad_rows<<<blocks((int64_t)rows * cols), dim3(256), 0, st>>>(W, cols, ld, fl(off), cols, rows);
    };
    slice(fp->w0, he, he + S2S_CE, C.w0s, he);
    slice(pp->res1_w, d.RF, d.RF + S2S_CE, C.res1s, he);
    for (int k = 0; k < K; ++k) slice(dp->pmsg_fc1_w[k], d.EA, d.EA + 2 * S2S_CE, C.p1s[k], hd);
    const float* in_w[3] = {dp->input_r_w, dp->input_i_w, dp->input_n_w};
    const float* in_b[3] = {dp->input_r_b, dp->input_i_b, dp->input_n_b};
    const float* pr_b[3] = {dp->present_r_b, dp->present_i_b, dp->present_n_b};
    for (int g = 0; g < 3; ++g) slice(in_w[g], d.RF, d.RF + S2S_CE, C.in_s[g], hd);
    // the fold: four one-hot blocks of the filter bank, bias tables
    k_s2s_charge_filter_fold<<<blocks((int64_t)(d.EA + 4) * he * (he / 4 + 1)), dim3(256), 0, st>>>(pp->filt_w2, pp->filt_b2, emb,
                                                                                                  d.EA, he, fl(C.w2f), fl(C.b2f));
    auto table = [&](const float* W, int ldw, int col0, const float* b1, const float* b2, int pair, int M, size_t off) {
        k_s2s_charge_table<<<blocks((pair ? 4 : 3) * M), dim3(256), 0, st>>>(W, ldw, col0, b1, b2, emb, pair, M, fl(off));
    };
    table(fp->w0, he + S2S_CE, he, fp->b0, nullptr, 0, he, C.t_f0);
    table(pp->res1_w, d.RF + S2S_CE, d.RF, pp->res1_b, nullptr, 0, he, C.t_res1);
    for (int g = 0; g < 3; ++g) table(in_w[g], d.RF + S2S_CE, d.RF, in_b[g], pr_b[g], 0, hd, C.t_g[g]);
    for (int k = 0; k < K; ++k) table(dp->pmsg_fc1_w[k], d.EA + 2 * S2S_CE, d.EA, dp->pmsg_fc1_b[k], nullptr, 1, hd, C.t_p1[k]);
    // the plain plan on the slices; its filter image from the folded bank (EA + 4 features)
    S2SChargeView view(fp, pp, dp, base, C, K);
    s2s_plan_build_front(&view.fp, &view.pp, D, he, rnn_hidden, prior_layers, prior_hidden, C.P, base, st, d.EA + 4);
    s2s_plan_build_recurrent(&view.dp, D, hd, K, C.P, base, st);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_charges_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                          int num_edge_types, int64_t n_nodes, int64_t n_edges) {
    const size_t base = aether_s2s_step_workspace_bytes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden,
                                                        num_edge_types, n_nodes, n_edges);
    if (base == 0) return 0;
    return S2SChargeWs(num_dims, base, n_nodes, n_edges).total;
}

int aether_s2s_charges_step(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                            const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                            int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                            int64_t n_nodes, int64_t n_edges, const int32_t* charge_index, const int64_t* send, const int64_t* recv,
                            const int64_t* order, const int64_t* rowptr, const float* inputs, const float* ext_field,
                            const float* ext_logits, const float* decoder_hidden_in, const float* h0, const float* c0,
                            const float* uniform, void* workspace,
                            size_t workspace_bytes, float* outputs, float* decoder_hidden_out, float* h1, float* c1,
                            float* edges_out, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    if (int rc = s2s_charges_check("s2s_charges_step", fp, pp, dp, plan, z,
                                   charge_index && send && recv && order && rowptr && inputs && decoder_hidden_in && uniform &&
                                       workspace && outputs && decoder_hidden_out && (ext_logits || (h0 && c0 && h1 && c1)) &&
                                       (!ext_logits || ext_field),
                                   0, 1)) return rc;
    S2SChargeCall call(fp, pp, dp, plan, z, send, recv, order, rowptr);
    if (int rc = call.prepare("s2s_charges_step", charge_index, workspace, workspace_bytes, (hipStream_t)stream)) return rc;
    call.a.ext_logits = ext_logits;
    return s2s_run_step("s2s_charges_step", call.a, workspace, workspace_bytes, {inputs, decoder_hidden_in, h0, c0}, ext_field, uniform,
                        {outputs, decoder_hidden_out, h1, c1}, edges_out, stream);
}

int aether_s2s_charges_rollout(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                               const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden,
                               int prior_layers, int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars,
                               float tau, int64_t n_nodes, int64_t n_edges, const int32_t* charge_index, const int64_t* send,
                               const int64_t* recv, const int64_t* order, const int64_t* rowptr, int burn_in_steps,
                               const float* burn_in, int steps, const float* inputs, float* decoder_state, float* h, float* c,
                               const float* uniform, void* workspace, size_t workspace_bytes, float* predictions,
                               float* edges_out, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    if (int rc = s2s_charges_check("s2s_charges_rollout", fp, pp, dp, plan, z,
                                   charge_index && send && recv && order && rowptr && inputs && decoder_state && h && c && uniform &&
                                       workspace && (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                   burn_in_steps, steps)) return rc;
    S2SChargeCall call(fp, pp, dp, plan, z, send, recv, order, rowptr);
    if (int rc = call.prepare("s2s_charges_rollout", charge_index, workspace, workspace_bytes, (hipStream_t)stream)) return rc;
    return s2s_run_rollout("s2s_charges_rollout", call.a, workspace, workspace_bytes, burn_in_steps, burn_in, steps, inputs,
                           decoder_state, h, c, uniform, predictions, edges_out, stream);
}

int aether_s2s_charges_encoder_features(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp,
                                        const AetherS2SDecoderParams* dp, const void* plan, int num_dims, int encoder_hidden,
                                        int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                                        int polar, int num_vars, int64_t n_nodes, int64_t n_edges, const int32_t* charge_index,
                                        const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                                        const float* inputs, const float* field, void* workspace, size_t workspace_bytes,
                                        float* features, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, 0,
                     polar, num_vars, 1.0f, n_nodes, n_edges};
    if (int rc = s2s_charges_check("s2s_charges_encoder_features", fp, pp, dp, plan, z,
                                   charge_index && send && recv && order && rowptr && inputs && field && workspace && features, 0, 1))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    S2SChargeCall call(fp, pp, dp, plan, z, send, recv, order, rowptr);
    if (int rc = call.prepare("s2s_charges_encoder_features", charge_index, workspace, workspace_bytes, st)) return rc;
    call.a.features_out = features;
    auto no_jobs = [](S2SJobs&) { return (int)AETHER_OK; };
    if (int rc = s2s_front_impl(call.a, call.a.L, call.a.P, (char*)workspace, inputs, field, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, no_jobs, no_jobs, st)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_charges_field_workspace_bytes(int64_t n_points, int hidden) {
    if (n_points <= 0 || hidden <= 0) return 0;
    return 3 * align_up((size_t)n_points * (size_t)hidden * sizeof(float), 256) + align_up((size_t)n_points * 4, 256);
}

int aether_s2s_charges_field(const AetherS2SFieldParams* fp, const void* plan, int num_dims, int encoder_hidden, int decoder_hidden,
                             int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int64_t n_points,
                             const float* x, int x_stride, const int32_t* charge_index, void* workspace, size_t workspace_bytes,
                             float* field, void* stream) {
    if (!fp || !plan || !x || !charge_index || !workspace || !field || !fp->B || !fp->w2 || !fp->b2 || !fp->w4 || !fp->b4)
        return fail(AETHER_EINVAL, "s2s_charges_field: null pointer");
    const int D = num_dims, he = encoder_hidden;
    if (s2s_charges_plan_size(D, he, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types) == 0)
        return fail(AETHER_EINVAL, "s2s_charges_field: bad sizes");
    if (n_points <= 0 || x_stride < D) return fail(AETHER_EINVAL, "s2s_charges_field: bad sizes");
    if (workspace_bytes < aether_s2s_charges_field_workspace_bytes(n_points, he))
        return fail(AETHER_ESPACE, "s2s_charges_field: workspace too small");
    const S2SChargePlan C(D, he, decoder_hidden, num_edge_types, rnn_hidden, prior_layers, prior_hidden);
    hipStream_t st = (hipStream_t)stream;
    const char* base = (const char*)plan;
    auto pl = [&](size_t off) { return reinterpret_cast<const float*>(base + off); };
    auto im = [&](size_t off) { return off ? reinterpret_cast<const void*>(base + off) : nullptr; };
    const size_t plane = align_up((size_t)n_points * he * sizeof(float), 256);
    float* gamma = reinterpret_cast<float*>(workspace);
    float* h1 = reinterpret_cast<float*>((char*)workspace + plane);
    float* h2 = reinterpret_cast<float*>((char*)workspace + 2 * plane);
    int32_t* nidx = reinterpret_cast<int32_t*>((char*)workspace + 3 * plane);
    k_s2s_charge_index<<<dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, st>>>(charge_index, n_points, nullptr, nullptr, 0,
                                                                                     nidx, nullptr, nullptr, async_error_word());
    const int half = he / 2;
    const unsigned rb = (unsigned)((n_points * half + 255) / 256);
    dispatch_dim(D, [&](auto DD) {
        k_s2s_rff<decltype(DD)::value><<<dim3(rb), dim3(256), 0, st>>>(x, x_stride, fp->B, half, gamma, n_points);
    });
    S2SJobs T;
    T.n = 1; T.j[0] = s2s_job(1, pl(C.w0s), he, nullptr, gamma, he, h1, he, he, he, n_points);
    T.j[0].Wimg = im(C.P.i_f0); T.j[0].btab = pl(C.t_f0); T.j[0].bidx = nidx; T.j[0].bstride = he;
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    T.n = 1; T.j[0] = s2s_job(1, fp->w2, he, fp->b2, h1, he, h2, he, he, he, n_points);
    T.j[0].Wimg = im(C.P.i_f2);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    if (s2s_linear(0, fp->w4, he, fp->b4, h2, field, D, he, n_points, D, nullptr, 0, 0, st)) return AETHER_EINVAL;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
