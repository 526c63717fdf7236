// Host side of the C ABI: the variable-N dNRI baseline (nn/dynamicvars/dnri_dynamicvars.py) on the scene engine of
// host_dyn_step.inc -- the staged prior and decoder steps, one prediction step and the whole prediction loop as ONE call for
// 1 .. 256 scenes (dyn_dnri.h has the kernels).  The model has no field and no frames: no field, localizer, edge-attribute or
// filter launch is made and no buffer is sized for one.  Included by aether_hip.hip inside its extern "C" block, after
// host_dyn_step.inc (whose scene checks and step / rollout drivers it shares); not a stand-alone source file.

namespace {
// Workspace of the prior step: node rows, edge rows, the BatchNorm affines and the summed LSTM biases.
struct DynDnriPriorLayout {
    size_t X1a, X1, Ps, Pr, T2, X2, X2n, X3a, X3, T4, X4, G, Y1, Y2, bn, lb, total;
    DynDnriPriorLayout(int h, int R, int ph, int64_t Nn, int64_t E) {
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, hh = (size_t)h;
        X1a = take(nn * hh); X1 = take(nn * hh); Ps = take(nn * hh); Pr = take(nn * hh); T2 = take(ee * hh); X2 = take(ee * hh);
        X2n = take(nn * hh); X3a = take(nn * hh); X3 = take(nn * hh); T4 = take(ee * hh); X4 = take(ee * hh);
        G = take(ee * 4 * (size_t)R);
        Y1 = take(ee * (size_t)(ph > 0 ? ph : 1)); Y2 = take(ee * (size_t)(ph > 0 ? ph : 1));
        bn = take(8 * hh); lb = take(4 * (size_t)R);
        total = off;
    }
};
// Workspace of the decoder step: the node products of the first message layer, the messages, the gate's rows, the lists.
struct DynDnriDecLayout {
    size_t A, S, Tm, M, agg, hr, hi, hh, o1, o2, ewn, lists, counts, total;
    DynDnriDecLayout(int h, int K, int64_t Nn, int64_t E) {
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, hh_ = (size_t)h, kk = (size_t)K;
        A = take(kk * nn * hh_); S = take(kk * nn * hh_); Tm = take(kk * ee * hh_); M = take(ee * hh_);
        agg = take(nn * hh_); hr = take(nn * hh_); hi = take(nn * hh_); hh = take(nn * hh_); o1 = take(nn * hh_); o2 = take(nn * hh_);
        ewn = take(ee * kk); lists = take(ee * kk * 2); counts = take(64);
        total = off;
    }
};

int dyn_dnri_prior_impl(const AetherDynDnriPriorParams* p, int h, int R, int prior_layers, int ph, int K, int64_t Nn, int64_t E,
                        const float* inputs, const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                        const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes, float* logits,
                        float* h1, float* c1, hipStream_t st) {
    if (!p || !inputs || !h0 || !c0 || !send || !recv || !order || !rowptr || !workspace || !logits || !h1 || !c1)
        return fail(AETHER_EINVAL, "dyn_dnri_prior: null pointer");
    if (h < 128 || h % 128 != 0) return fail(AETHER_EINVAL, "dyn_dnri_prior: hidden must be a multiple of 128");
    if (R < 16 || R % 16 != 0) return fail(AETHER_EINVAL, "dyn_dnri_prior: rnn_hidden must be a multiple of 16");
    if (prior_layers < 1 || prior_layers > 4) return fail(AETHER_EINVAL, "dyn_dnri_prior: 1..4 prior layers");
    if (prior_layers > 1 && (ph < 16 || ph % 16 != 0))
        return fail(AETHER_EINVAL, "dyn_dnri_prior: prior_hidden must be a multiple of 16");
    if (K < 1 || K > 4 || Nn <= 0 || E <= 0 || E > INT32_MAX / 64) return fail(AETHER_EINVAL, "dyn_dnri_prior: bad sizes");
    const float* bns[4] = {nullptr, nullptr, nullptr, nullptr};
    const DynDnriPriorLayout L(h, R, ph, Nn, E);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "dyn_dnri_prior: workspace too small");
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    for (int l = 0; l < 4; ++l) {
        if (!p->mlp_w0[l] || !p->mlp_b0[l] || !p->mlp_w3[l] || !p->mlp_b3[l]) return fail(AETHER_EINVAL, "dyn_dnri_prior: null weight");
        if (!p->mlp_bn_w[l]) continue;                         // no_encoder_bn
        if (!p->mlp_bn_b[l] || !p->mlp_bn_mean[l] || !p->mlp_bn_var[l])
            return fail(AETHER_EINVAL, "dyn_dnri_prior: incomplete BatchNorm pointers");
        bns[l] = wp(L.bn) + (size_t)2 * l * h;
    }
    if (!p->lstm_w_ih || !p->lstm_w_hh || !p->lstm_b_ih || !p->lstm_b_hh) return fail(AETHER_EINVAL, "dyn_dnri_prior: null LSTM weight");
    for (int l = 0; l < prior_layers; ++l)
        if (!p->prior_w[l] || !p->prior_b[l]) return fail(AETHER_EINVAL, "dyn_dnri_prior: null prior_fc_out weight");
    S2SJobs T;
    auto one = [&](S2SJob J) { T.n = 0; T.j[T.n++] = J; return s2s_launch_jobs(T, st); };
    auto bn_job = [&](S2SJob J, int l) { if (bns[l]) { J.post_scale = bns[l]; J.post_shift = bns[l] + h; } return J; };
    // ---- mlp1 on the raw 4 columns (:412): the first Linear in the node kernel (with the BatchNorm affines and the LSTM bias)
    {
        const int64_t work = std::max<int64_t>(std::max<int64_t>(Nn * (h / 4), (int64_t)4 * h), (int64_t)4 * R);
        k_dyn_dnri_node_in<<<blocks(work), dim3(256), 0, st>>>(
            inputs, p->mlp_w0[0], p->mlp_b0[0], wp(L.X1a), h, Nn, p->mlp_bn_w[0], p->mlp_bn_w[1], p->mlp_bn_w[2], p->mlp_bn_w[3],
            p->mlp_bn_b[0], p->mlp_bn_b[1], p->mlp_bn_b[2], p->mlp_bn_b[3], p->mlp_bn_mean[0], p->mlp_bn_mean[1], p->mlp_bn_mean[2],
            p->mlp_bn_mean[3], p->mlp_bn_var[0], p->mlp_bn_var[1], p->mlp_bn_var[2], p->mlp_bn_var[3], wp(L.bn), p->lstm_b_ih,
            p->lstm_b_hh, wp(L.lb), R);
    }
    if (int rc = one(bn_job(s2s_job(4, p->mlp_w3[0], h, p->mlp_b3[0], wp(L.X1a), h, wp(L.X1), h, h, h, Nn), 0))) return rc;
    // ---- [x_send | x_recv] -> mlp2 (:413-415): the first Linear as the node products of its two halves, no [E, 2h] rows
    T.n = 0;
    T.j[T.n++] = s2s_job(0, p->mlp_w0[1], 2 * h, p->mlp_b0[1], wp(L.X1), h, wp(L.Ps), h, h, h, Nn);
    T.j[T.n++] = s2s_job(0, p->mlp_w0[1] + h, 2 * h, nullptr, wp(L.X1), h, wp(L.Pr), h, h, h, Nn);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    k_s2s_dnri_pair_elu<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(wp(L.Ps), wp(L.Pr), send, recv, wp(L.T2), h, E);
    if (int rc = one(bn_job(s2s_job(4, p->mlp_w3[1], h, p->mlp_b3[1], wp(L.T2), h, wp(L.X2), h, h, h, E), 1))) return rc;
    // ---- index_add_ over the receiver (:416-417): a sum; mlp3 (:418)
    k_dyn_dnri_recv_sum<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.X2), order, rowptr, wp(L.X2n), h);
    if (int rc = one(s2s_job(4, p->mlp_w0[2], h, p->mlp_b0[2], wp(L.X2n), h, wp(L.X3a), h, h, h, Nn))) return rc;
    if (int rc = one(bn_job(s2s_job(4, p->mlp_w3[2], h, p->mlp_b3[2], wp(L.X3a), h, wp(L.X3), h, h, h, Nn), 2))) return rc;
    // ---- [x_send | x_recv | skip] -> mlp4 (:419-421): node halves in one launch, the skip third through the GEMM with the
    // gathers in its epilogue -- no [E, 3h] rows
    T.n = 0;
    T.j[T.n++] = s2s_job(0, p->mlp_w0[3], 3 * h, p->mlp_b0[3], wp(L.X3), h, wp(L.Ps), h, h, h, Nn);
    T.j[T.n++] = s2s_job(0, p->mlp_w0[3] + h, 3 * h, nullptr, wp(L.X3), h, wp(L.Pr), h, h, h, Nn);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    { S2SJob J = s2s_job(4, p->mlp_w0[3] + 2 * h, 3 * h, nullptr, wp(L.X2), h, wp(L.T4), h, h, h, E);
      J.g1 = wp(L.Ps); J.i1 = send; J.g2 = wp(L.Pr); J.i2 = recv;
      if (int rc = one(J)) return rc; }
    if (int rc = one(bn_job(s2s_job(4, p->mlp_w3[3], h, p->mlp_b3[3], wp(L.T4), h, wp(L.X4), h, h, h, E), 3))) return rc;
    // ---- one LSTM step per edge (:558-560): [W_ih | W_hh] . [x | h0] in one launch, then the cell; prior_fc_out (:566)
    { S2SJob J = s2s_job(0, p->lstm_w_ih, h, wp(L.lb), wp(L.X4), h, wp(L.G), 4 * R, 4 * R, h, E);
      J.W2 = p->lstm_w_hh; J.X2 = h0; J.K2 = R; J.ldw2 = R; J.ldx2 = R;
      if (int rc = one(J)) return rc; }
    k_s2s_lstm_cell<<<blocks(E * R), dim3(256), 0, st>>>(wp(L.G), c0, h1, c1, R, E);
    const float* cur = h1;
    int cur_k = R;
    for (int l = 0; l < prior_layers; ++l) {
        const bool last = l + 1 == prior_layers;
        float* dst = last ? logits : wp(l % 2 == 0 ? L.Y1 : L.Y2);
        const int M = last ? K : ph;
        if (int rc = one(s2s_job(last ? 0 : 4, p->prior_w[l], cur_k, p->prior_b[l], cur, cur_k, dst, M, M, cur_k, E))) return rc;
        cur = dst;
        cur_k = M;
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// The scatter of the one-call step: the last layer writes the un-compacted rows itself (k_dyn_dnri_out)
struct DynDnriScatter { const int* cidx; const int* status; int64_t n_rows; float* hidden; bool counts_zeroed; };

int dyn_dnri_decoder_impl(const AetherDynDnriDecoderParams* p, int h, int K, int skip_first, int64_t Nn, int64_t E,
                          const float* inputs, const float* hidden_in, const float* edge_w, const int64_t* send,
                          const int64_t* recv, const int64_t* agg_order, const int64_t* agg_rowptr, float agg_div,
                          const float* agg_div_node, void* workspace, size_t workspace_bytes, float* outputs, float* hidden_out,
                          hipStream_t st, const DynDnriScatter* sc) {
    if (!p || !inputs || !hidden_in || !edge_w || !send || !recv || !agg_order || !agg_rowptr || !workspace || !outputs || !hidden_out)
        return fail(AETHER_EINVAL, "dyn_dnri_decoder: null pointer");
    if (h < 128 || h % 128 != 0) return fail(AETHER_EINVAL, "dyn_dnri_decoder: hidden must be a multiple of 128");
    if (K < 1 || K > 4) return fail(AETHER_EINVAL, "dyn_dnri_decoder: 1..4 edge types");
    if (skip_first && K < 2) return fail(AETHER_EINVAL, "dyn_dnri_decoder: skip_first needs two edge types");
    if (Nn < 2 || E <= 0 || E > INT32_MAX / 64)
        return fail(AETHER_EINVAL, "dyn_dnri_decoder: bad sizes (a scene with one present object has no edges and is not taken)");
    if (!agg_div_node && !(agg_div > 0.0f)) return fail(AETHER_EINVAL, "dyn_dnri_decoder: agg_div must be positive");
    const int k0 = skip_first ? 1 : 0;
    for (int k = k0; k < K; ++k)
        if (!p->msg_fc1_w[k] || !p->msg_fc1_b[k] || !p->msg_fc2_w[k] || !p->msg_fc2_b[k])
            return fail(AETHER_EINVAL, "dyn_dnri_decoder: null message weight");
    if (!p->hidden_r_w || !p->hidden_i_w || !p->hidden_h_w || !p->input_r_w || !p->input_r_b || !p->input_i_w || !p->input_i_b ||
        !p->input_n_w || !p->input_n_b || !p->out1_w || !p->out1_b || !p->out2_w || !p->out2_b || !p->out3_w || !p->out3_b)
        return fail(AETHER_EINVAL, "dyn_dnri_decoder: null weight");
    const DynDnriDecLayout L(h, K, Nn, E);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "dyn_dnri_decoder: workspace too small");
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int64_t* lists = reinterpret_cast<int64_t*>(ws + L.lists);
    float* A = wp(L.A);
    float* S = wp(L.S);
    S2SJobs T;
    if (!(sc && sc->counts_zeroed)) HIP_OK(hipMemsetAsync(counts, 0, 64 * sizeof(int), st));
    // ---- per-type edge lists of the (one-hot) sample; the receiver | sender halves of msg_fc1 on the hidden state (:635-638, :652)
    k_s2s_select_all<<<blocks(E), dim3(256), 0, st>>>(edge_w, K, k0, 1.0f, wp(L.ewn), lists, (size_t)E, counts, E);
    T.n = 0;
    for (int k = k0; k < K; ++k) {
        T.j[T.n++] = s2s_job(0, p->msg_fc1_w[k], 2 * h, p->msg_fc1_b[k], hidden_in, h, A + (size_t)k * Nn * h, h, h, h, Nn);
        T.j[T.n++] = s2s_job(0, p->msg_fc1_w[k] + h, 2 * h, nullptr, hidden_in, h, S + (size_t)k * Nn * h, h, h, h, Nn);
    }
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    k_s2s_dnri_pair<false><<<blocks(E * (h / 4)), dim3(256), 0, st>>>(A, S, Nn, send, recv, edge_w, K, k0, wp(L.Tm), wp(L.M), h, E);
    // ---- second layer of every used type in one launch: rows through the type's list, times the sample's weight (:654-655)
    T.n = 0;
    for (int k = k0; k < K; ++k) {
        S2SJob J = s2s_job(3, p->msg_fc2_w[k], h, p->msg_fc2_b[k], wp(L.Tm) + (size_t)k * E * h, h, wp(L.M), h, h, h, E);
        J.xidx = lists + (size_t)k * E; J.yidx = lists + (size_t)k * E; J.n_dev = counts + k;
        J.scale = wp(L.ewn) + k; J.sstride = K;
        T.j[T.n++] = J;
    }
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    // ---- / norm, sum over the edge2node rows / (num_vars - 1) of the object's scene (:656-661)
    k_dyn_dnri_aggregate<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.M), agg_order, agg_rowptr, wp(L.agg), h, (float)(K - k0), agg_div,
                                                                  agg_div_node);
    // ---- GRU-style gate on the raw inputs (:669-675)
    T.n = 0;
    T.j[T.n++] = s2s_job(0, p->hidden_r_w, h, nullptr, wp(L.agg), h, wp(L.hr), h, h, h, Nn);
    T.j[T.n++] = s2s_job(0, p->hidden_i_w, h, nullptr, wp(L.agg), h, wp(L.hi), h, h, h, Nn);
    T.j[T.n++] = s2s_job(0, p->hidden_h_w, h, nullptr, wp(L.agg), h, wp(L.hh), h, h, h, Nn);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    k_s2s_dnri_gate<<<blocks(Nn * (h / 4)), dim3(256), 0, st>>>(inputs, 4, p->input_r_w, p->input_r_b, p->input_i_w, p->input_i_b,
                                                               p->input_n_w, p->input_n_b, wp(L.hr), wp(L.hi), wp(L.hh), hidden_in,
                                                               hidden_out, h, Nn);
    // ---- output MLP, residual and (the step) the rows back to their objects (:678-686)
    auto one = [&](S2SJob J) { T.n = 0; T.j[T.n++] = J; return s2s_launch_jobs(T, st); };
    if (int rc = one(s2s_job(2, p->out1_w, h, p->out1_b, hidden_out, h, wp(L.o1), h, h, h, Nn))) return rc;
    if (int rc = one(s2s_job(2, p->out2_w, h, p->out2_b, wp(L.o1), h, wp(L.o2), h, h, h, Nn))) return rc;
    const int64_t rows = sc ? sc->n_rows : Nn;
    k_dyn_dnri_out<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st>>>(wp(L.o2), p->out3_w, p->out3_b, h, inputs, outputs, rows,
                                                                          sc ? sc->cidx : nullptr, sc ? sc->status : nullptr,
                                                                          hidden_out, sc ? sc->hidden : nullptr);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

struct DynDnriBatchLayout : DynSceneLayout {
    size_t ws_prior, ws_dec;
    size_t b_prior, b_dec;
    DynDnriBatchLayout(const AetherDynStepConfig& c, int B, int n_max, const DynBatchSizes& Z) : DynSceneLayout(c, B, n_max, Z) {
        b_prior = DynDnriPriorLayout(c.encoder_hidden, c.rnn_hidden, c.prior_hidden, Z.n_total, Z.e_total).total;
        b_dec = DynDnriDecLayout(c.decoder_hidden, c.num_edge_types, Z.n_total, Z.e_total).total;
        ws_prior = take(b_prior); ws_dec = take(b_dec);
    }
};

// DNRIDynamicVars on the driver of host_dyn_step.inc: present, kNN, csr, index, prior, sample, decoder (whose last kernel
// writes the rows back to their objects: no finish launch).
struct DynDnriModel {
    using Layout = DynDnriBatchLayout;
    using Ctx = DynStepCtx<Layout>;
    static constexpr const char* step_name = "dyn_dnri_step_batched";
    static constexpr const char* rollout_name = "dyn_dnri_rollout_batched";
    const AetherDynDnriPriorParams* prior_params;
    const AetherDynDnriDecoderParams* decoder_params;
    bool params_ok() const { return prior_params && decoder_params; }
    int config_check(const char* entry, const AetherDynStepConfig& c) const {
        if (c.skip_first && c.num_edge_types < 2) return dyn_fail(AETHER_EINVAL, entry, "skip_first needs two edge types");
        if (c.prior_layers < 1 || c.prior_layers > 4 || (c.prior_layers > 1 && (c.prior_hidden < 16 || c.prior_hidden % 16 != 0)))
            return dyn_fail(AETHER_EINVAL, entry, "1..4 prior layers, prior_hidden a multiple of 16");
        return AETHER_OK;
    }
    size_t counts_offset(const Ctx& X) const {
        return X.L.ws_dec + DynDnriDecLayout(X.c.decoder_hidden, X.c.num_edge_types, X.n, X.E).counts;
    }
    int field(const Ctx&) const { return AETHER_OK; }                  // (no field)
    // the callers' graphs in the numbering of the batch, LSTM state rows of their edges (:554-559)
    void index(const Ctx& X) const {
        const Layout& L = X.L;
        const int R = X.c.rnn_hidden;
        const int64_t work = std::max<int64_t>(X.E * (R / 4), X.Z.o_total);
        k_dynb_dnri_index<<<dyn_blocks(work), dim3(256), 0, X.st()>>>(X.S, X.graph_send, X.graph_recv, X.node_inds, X.ip(L.idx),
                                                                     X.edge2node, R, X.prior_h, X.prior_c, X.ip(L.send),
                                                                     X.ip(L.recv), X.ip(L.slot), X.fp(L.h0), X.fp(L.c0),
                                                                     X.ip(L.order));
    }
    int prior(const Ctx& X) const {
        const Layout& L = X.L;
        const AetherDynStepConfig& c = X.c;
        return dyn_dnri_prior_impl(prior_params, c.encoder_hidden, c.rnn_hidden, c.prior_layers, c.prior_hidden, c.num_edge_types,
                                   X.n, X.E, X.fp(L.cur_in), X.fp(L.h0), X.fp(L.c0), X.ip(L.ksend), X.ip(L.krecv), X.ip(L.korder),
                                   X.ip(L.krowptr), X.ws + L.ws_prior, L.b_prior, X.fp(L.logits), X.fp(L.h1), X.fp(L.c1), X.st());
    }
    // decoder step on the callers' graphs (:618-688); its last kernel writes the rows back to their objects
    int decode(const Ctx& X, const float* ew) const {
        const Layout& L = X.L;
        const AetherDynStepConfig& c = X.c;
        const DynDnriScatter sc{X.cidx(), X.status(), X.rows, X.decoder_hidden, true};
        return dyn_dnri_decoder_impl(decoder_params, c.decoder_hidden, c.num_edge_types, c.skip_first, X.n, X.E, X.fp(L.cur_in),
                                     X.fp(L.cur_h), ew, X.ip(L.send), X.ip(L.recv), X.ip(L.order), X.ip(L.rowptr_dec), 1.0f,
                                     X.fp(L.div_node), X.ws + L.ws_dec, L.b_dec, X.prediction, X.fp(L.new_h), X.st(), &sc);
    }
};
}  // namespace

/* see include/aether_hip.h */
size_t aether_dyn_dnri_prior_workspace_bytes(int hidden, int rnn_hidden, int prior_hidden, int64_t n_nodes, int64_t n_edges) {
    if (hidden <= 0 || rnn_hidden <= 0 || prior_hidden < 0 || n_nodes <= 0 || n_edges <= 0) return 0;
    return DynDnriPriorLayout(hidden, rnn_hidden, prior_hidden, n_nodes, n_edges).total;
}

int aether_dyn_dnri_prior_step(const AetherDynDnriPriorParams* params, int hidden, int rnn_hidden, int prior_layers,
                               int prior_hidden, int num_edge_types, int polar, int64_t n_nodes, int64_t n_edges,
                               const float* inputs, const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                               const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                               float* logits, float* h1, float* c1, void* stream) {
    (void)polar;
    return dyn_dnri_prior_impl(params, hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, n_nodes, n_edges, inputs, h0,
                               c0, send, recv, order, rowptr, workspace, workspace_bytes, logits, h1, c1, (hipStream_t)stream);
}

size_t aether_dyn_dnri_decoder_workspace_bytes(int hidden, int num_edge_types, int64_t n_nodes, int64_t n_edges) {
    if (hidden <= 0 || num_edge_types < 1 || num_edge_types > 4 || n_nodes <= 0 || n_edges <= 0) return 0;
    return DynDnriDecLayout(hidden, num_edge_types, n_nodes, n_edges).total;
}

int aether_dyn_dnri_decoder_step_batched(const AetherDynDnriDecoderParams* params, int hidden, int num_edge_types, int skip_first,
                                         int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                                         const float* hidden_in, const float* edge_w, const int64_t* send, const int64_t* recv,
                                         const int64_t* agg_order, const int64_t* agg_rowptr, float agg_div,
                                         const float* agg_div_node, void* workspace, size_t workspace_bytes, float* outputs,
                                         float* hidden_out, void* stream) {
    (void)polar;
    return dyn_dnri_decoder_impl(params, hidden, num_edge_types, skip_first, n_nodes, n_edges, inputs, hidden_in, edge_w, send, recv,
                                 agg_order, agg_rowptr, agg_div, agg_div_node, workspace, workspace_bytes, outputs, hidden_out,
                                 (hipStream_t)stream, nullptr);
}

size_t aether_dyn_dnri_step_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max,
                                                    const int64_t* n_present, const int64_t* n_edges, const int* in_degree) {
    return dyn_step_bytes<DynDnriBatchLayout>(config, n_scenes, n_objects_max, n_present, n_edges, in_degree);
}

int aether_dyn_dnri_step_batched(const AetherDynDnriPriorParams* prior_params, const AetherDynDnriDecoderParams* decoder_params,
                                 const AetherDynStepConfig* config, int n_scenes, int n_objects_max, const int64_t* n_present,
                                 const int64_t* n_edges, const int* in_degree, const float* state, const float* mask,
                                 const int64_t* node_inds, const int64_t* graph_send, const int64_t* graph_recv,
                                 const int64_t* edge2node, float* prior_h, float* prior_c, float* decoder_hidden,
                                 const float* uniform, float* prediction, float* edge_types, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return dyn_step_run(DynDnriModel{prior_params, decoder_params}, config, n_scenes, n_objects_max, n_present, n_edges, in_degree,
                        state, mask, node_inds, graph_send, graph_recv, edge2node, prior_h, prior_c, decoder_hidden, uniform,
                        prediction, edge_types, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------ the prediction loop (predict_future, :152-175)
size_t aether_dyn_dnri_rollout_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max,
                                                       int n_steps, const int64_t* n_present, const int64_t* n_edges,
                                                       const int* in_degree) {
    return dyn_rollout_bytes<DynDnriBatchLayout>(config, n_scenes, n_objects_max, n_steps, n_present, n_edges, in_degree);
}

int aether_dyn_dnri_rollout_batched(const AetherDynDnriPriorParams* prior_params, const AetherDynDnriDecoderParams* decoder_params,
                                    const AetherDynStepConfig* config, int n_scenes, int n_objects_max, int n_steps,
                                    const float* inputs, const float* masks, const float* burn_in_masks, const int64_t* n_present,
                                    const int64_t* n_edges, const int* in_degree, const int64_t* const* node_inds,
                                    const int64_t* const* graph_send, const int64_t* const* graph_recv,
                                    const int64_t* const* edge2node, const float* const* uniform, float* prior_h, float* prior_c,
                                    float* decoder_hidden, float* predictions, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    return dyn_rollout_run(DynDnriModel{prior_params, decoder_params}, config, n_scenes, n_objects_max, n_steps, inputs, masks,
                           burn_in_masks, n_present, n_edges, in_degree, node_inds, graph_send, graph_recv, edge2node, uniform,
                           prior_h, prior_c, decoder_hidden, predictions, workspace, workspace_bytes, stream);
}
