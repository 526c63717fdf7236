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
                        float* h1, float* c1, hipStream_t st, const NriSeqTail* seq = nullptr) {
    // seq: null (one prior step from h0 / c0), or the sequence encoder's tail on the same rows -- the LSTM step from the zero
    // state and both heads (host_nri_chain.inc 3b); h0, c0 and c1 are not read or written then.
    if (!p || !inputs || !send || !recv || !order || !rowptr || !workspace || !logits || !h1 || (!seq && (!h0 || !c0 || !c1)))
        return fail(AETHER_EINVAL, "dyn_dnri_prior: null pointer");
    if (h < 128 || h % 128 != 0) return fail(AETHER_EINVAL, "dyn_dnri_prior: hidden must be a multiple of 128");
    if (R < 16 || R % 16 != 0) return fail(AETHER_EINVAL, "dyn_dnri_prior: rnn_hidden must be a multiple of 16");
    if (prior_layers < 1 || prior_layers > 4) return fail(AETHER_EINVAL, "dyn_dnri_prior: 1..4 prior layers");
    if (prior_layers > 1 && (ph < 16 || ph % 16 != 0))
        return fail(AETHER_EINVAL, "dyn_dnri_prior: prior_hidden must be a multiple of 16");
    if (K < 1 || K > 4 || Nn <= 0 || E <= 0 || E > INT32_MAX / 64) return fail(AETHER_EINVAL, "dyn_dnri_prior: bad sizes");
    const DynDnriPriorLayout L(h, R, ph, Nn, E);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "dyn_dnri_prior: workspace too small");
    const NriMem m{(char*)workspace, nullptr};                 // (no plan: no weight has an image)
    NriDnriPrior c{};                                          // (host_nri_chain.inc: plain receiver sum, BatchNorm where there is one)
    c.send = send; c.recv = recv; c.order = order; c.rowptr = rowptr; c.mean_div = 0.0f;
    c.X1a = m.wp(L.X1a); c.X1 = m.wp(L.X1); c.Ps = m.wp(L.Ps); c.Pr = m.wp(L.Pr); c.T2 = m.wp(L.T2); c.X2 = m.wp(L.X2);
    c.X2n = m.wp(L.X2n); c.X3a = m.wp(L.X3a); c.X3 = m.wp(L.X3); c.T4 = m.wp(L.T4); c.out = m.wp(L.X4);
    c.h = h; c.Nn = Nn; c.E = E;
    for (int l = 0; l < 4; ++l) {
        if (!p->mlp_w0[l] || !p->mlp_b0[l] || !p->mlp_w3[l] || !p->mlp_b3[l]) return fail(AETHER_EINVAL, "dyn_dnri_prior: null weight");
        if (!p->mlp_bn_w[l]) continue;                         // no_encoder_bn
        if (!p->mlp_bn_b[l] || !p->mlp_bn_mean[l] || !p->mlp_bn_var[l])
            return fail(AETHER_EINVAL, "dyn_dnri_prior: incomplete BatchNorm pointers");
        c.bn_scale[l] = m.wp(L.bn) + (size_t)2 * l * h; c.bn_shift[l] = c.bn_scale[l] + h;
    }
    if (!p->lstm_w_ih || !p->lstm_w_hh || !p->lstm_b_ih || !p->lstm_b_hh) return fail(AETHER_EINVAL, "dyn_dnri_prior: null LSTM weight");
    for (int l = 0; l < prior_layers; ++l)
        if (!p->prior_w[l] || !p->prior_b[l]) return fail(AETHER_EINVAL, "dyn_dnri_prior: null prior_fc_out weight");
    // ---- mlp1 on the raw 4 columns (:412): the first Linear in the node kernel (with the BatchNorm affines and the LSTM bias)
    {
        const int64_t work = std::max<int64_t>(std::max<int64_t>(Nn * (h / 4), (int64_t)4 * h), (int64_t)4 * R);
        k_dyn_dnri_node_in<<<nri_blocks(work), dim3(256), 0, st>>>(
            inputs, p->mlp_w0[0], p->mlp_b0[0], c.X1a, h, Nn, p->mlp_bn_w[0], p->mlp_bn_w[1], p->mlp_bn_w[2], p->mlp_bn_w[3],
            p->mlp_bn_b[0], p->mlp_bn_b[1], p->mlp_bn_b[2], p->mlp_bn_b[3], p->mlp_bn_mean[0], p->mlp_bn_mean[1], p->mlp_bn_mean[2],
            p->mlp_bn_mean[3], p->mlp_bn_var[0], p->mlp_bn_var[1], p->mlp_bn_var[2], p->mlp_bn_var[3], m.wp(L.bn), p->lstm_b_ih,
            p->lstm_b_hh, m.wp(L.lb), R);
    }
    // ---- mlp1's second layer .. mlp4 (:412-421): node products instead of [E, 2h] / [E, 3h] rows, index_add_ over the receiver
    if (int rc = nri_dnri_prior(p, c, [](S2SJobs&) { return (int)AETHER_OK; }, st)) return rc;
    if (seq) {   // ---- every frame from the zero state, prior_fc_out and encoder_fc_out (:499-541)
        if (int rc = nri_seq_tail(p->lstm_w_ih, p->lstm_b_ih, p->lstm_b_hh, p->prior_w, p->prior_b, prior_layers, ph, *seq, h, R, K,
                                  E, c.out, h1, m.wp(L.Y1), m.wp(L.Y2), logits, st)) return rc;
        HIP_OK(hipGetLastError());
        return AETHER_OK;
    }
    // ---- one LSTM step per edge (:558-560), prior_fc_out (:566): no images, so the fp32 job kernel with the summed bias, then the cell
    if (int rc = nri_lstm_head(NriLstmHead{p->lstm_w_ih, p->lstm_w_hh, m.wp(L.lb), nullptr, nullptr, nullptr, p->prior_w, p->prior_b,
                                           {nullptr, nullptr, nullptr, nullptr}, c.out, h0, c0, m.wp(L.G), h1, c1, m.wp(L.Y1),
                                           m.wp(L.Y2), logits, h, R, prior_layers, ph, K, E}, st)) return rc;
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
    const NriMem m{(char*)workspace, nullptr};
    int* counts = reinterpret_cast<int*>(m.ws + L.counts);
    int64_t* lists = reinterpret_cast<int64_t*>(m.ws + L.lists);
    if (!(sc && sc->counts_zeroed)) HIP_OK(hipMemsetAsync(counts, 0, 64 * sizeof(int), st));
    // ---- per-type edge lists of the (one-hot) sample (:635-638)
    k_s2s_select_all<<<nri_blocks(E), dim3(256), 0, st>>>(edge_w, K, k0, 1.0f, m.wp(L.ewn), lists, (size_t)E, counts, E);
    // ---- msg_fc1 .. out_fc2 (:652-680, host_nri_chain.inc): no images; / norm, sum over the edge2node rows / the scene's num_vars - 1
    NriDnriDecoder d{};
    d.x_in = inputs; d.dh_in = hidden_in; d.sample = edge_w; d.scale = m.wp(L.ewn);
    d.lists = lists; d.send = send; d.recv = recv; d.counts = counts;
    d.A = m.wp(L.A); d.S = m.wp(L.S); d.Tm = m.wp(L.Tm); d.M = m.wp(L.M); d.agg = m.wp(L.agg); d.hr = m.wp(L.hr); d.hi = m.wp(L.hi);
    d.hh = m.wp(L.hh); d.o1 = m.wp(L.o1); d.o2 = m.wp(L.o2); d.dh_out = hidden_out;
    d.ldx = 4; d.hd = h; d.K = K; d.k0 = k0; d.Nn = Nn; d.E = E; d.node_products = true;
    auto aggregate = [&] {
        k_dyn_dnri_aggregate<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(d.M, agg_order, agg_rowptr, d.agg, h, (float)(K - k0), agg_div,
                                                                      agg_div_node);
    };
    if (int rc = nri_dnri_decoder(p, d, aggregate, st)) return rc;
    // ---- last layer, residual and (the step) the rows back to their objects (:681-686)
    const int64_t rows = sc ? sc->n_rows : Nn;
    k_dyn_dnri_out<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st>>>(d.o2, p->out3_w, p->out3_b, h, inputs, outputs, rows,
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
    int decode(const Ctx& X, const float* ew, bool = true) const {      // (no frames: nothing of the prior step is read)
        const Layout& L = X.L;
        const AetherDynStepConfig& c = X.c;
        const DynDnriScatter sc{X.cidx(), X.status(), X.rows, X.decoder_hidden, true};
        return dyn_dnri_decoder_impl(decoder_params, c.decoder_hidden, c.num_edge_types, c.skip_first, X.n, X.E, X.fp(L.cur_in),
                                     X.fp(L.cur_h), ew, X.ip(L.send), X.ip(L.recv), X.ip(L.order), X.ip(L.rowptr_dec), 1.0f,
                                     X.fp(L.div_node), X.ws + L.ws_dec, L.b_dec, X.prediction, X.fp(L.new_h), X.st(), &sc);
    }
    // ---- the evaluation half of calculate_loss (host_dyn_loss.inc: dyn_seq_run, dyn_loss_run)
    static constexpr const char* seq_name = "dyn_dnri_sequence_logits";
    static constexpr const char* loss_name = "dyn_dnri_loss_rollout";
    bool seq_params_ok() const { return prior_params != nullptr; }
    bool loss_params_ok() const { return decoder_params != nullptr; }
    static size_t seq_field_bytes(const AetherDynStepConfig&, const DynBatchSizes&) { return 0; }
    static size_t seq_prior_bytes(const AetherDynStepConfig& c, const DynBatchSizes& Z) {
        return DynDnriPriorLayout(c.encoder_hidden, c.rnn_hidden, c.prior_hidden, Z.n_total, Z.e_total).total;
    }
    int seq_field(const DynSeqCtx&) const { return AETHER_OK; }
    int seq_prior(const DynSeqCtx& Q) const {
        const AetherDynStepConfig& c = Q.c;
        return dyn_dnri_prior_impl(prior_params, c.encoder_hidden, c.rnn_hidden, c.prior_layers, c.prior_hidden, c.num_edge_types,
                                   Q.n, Q.E, Q.fp(Q.L.cur_in), nullptr, nullptr, Q.ip(Q.L.ksend), Q.ip(Q.L.krecv), Q.ip(Q.L.korder),
                                   Q.ip(Q.L.krowptr), Q.ws + Q.L.ws_prior, Q.L.b_prior, Q.prior_logits, Q.fp(Q.L.h1), nullptr,
                                   (hipStream_t)Q.stream, &Q.tail);
    }
    void loss_graph(const Ctx& X) const {
        const Layout& L = X.L;
        k_dyn_loss_graph<<<dyn_blocks(std::max<int64_t>(X.E, X.Z.o_total)), dim3(256), 0, X.st()>>>(
            X.graph_send, X.graph_recv, X.edge2node, X.n, X.E, X.Z.o_total, X.S.n_max, X.ip(L.send), X.ip(L.recv), X.ip(L.order),
            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, X.status());
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
