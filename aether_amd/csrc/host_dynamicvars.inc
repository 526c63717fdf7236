// Host side of the C ABI: variable-N model steps and the kNN edge builder (SURVEY 8f N2).  Included by aether_hip.hip inside its extern "C" block (one translation
// unit: the kernels live in anonymous namespaces); not a stand-alone source file.

// ------------------------------------------------------------------ variable-N decoder step (N2)
namespace {
// The variable-N models' anisotropic filter (aether_dynamicvars.py: 15 edge features, ReLU hyper-network): the split-fp16
// filter GEMM of s2s_filter.h.  image: prepared (aether_s2s_filter_prepare) or NULL -> built into fimg for this call.
int dyn_filter(const float* w0, const float* b0, const float* w2, const float* b2, const void* image, const float* ea15,
               const float* epos, char* bimg_buf, char* fimg_buf, float* fpart, float* out, int h, int64_t E, hipStream_t st) {
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    const f16x8* img = reinterpret_cast<const f16x8*>(image);
    if (!img) {
        f16x8* mine = reinterpret_cast<f16x8*>(fimg_buf);
        filter_images_launch(w2, 15, h, mine, st);
        img = mine;
    }
    f16x8* bimg = reinterpret_cast<f16x8*>(bimg_buf);
    k_s2s_filter_bimg<3><<<filter_bimg_grid(E), dim3(256), 0, st>>>(epos, w0, b0, 1, h, E, bimg);
    const int splits = S2SPriorLayout::filter_splits(h, E);
    const int rs = S2SPriorLayout::filter_rsplits15(h, E), planes = splits * rs;
    const int64_t units = ((E + 255) / 256) * (h / 64) * planes;
    const dim3 grid((unsigned)(units < FILTER_WGS ? units : FILTER_WGS));
    float* dst = planes > 1 ? fpart : out;
    const size_t lds = filt_lds_bytes(15);
    if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_s2s_filter_split<15>), lds)) return AETHER_EHIP;
    k_s2s_filter_split<15><<<grid, dim3(512), lds, st>>>(img, b2, ea15, bimg, dst, h, E, splits, rs, (int)grid.x);
    if (planes > 1) k_s2s_sum_planes<<<blocks(E * h / 4), dim3(256), 0, st>>>(fpart, planes, E * (int64_t)h, out);
    return AETHER_OK;
}
}  // namespace
namespace {
struct DynDecLayout {
    size_t A[4], S[4], Tm, M, M2, agg_h, agg_p, ext, rel, Rinv, ea, ea15, epos, bimg, fimg, fout, fpart, ewn, rp, ip, np_, hh, o1,
        o2, list[4], counts, bimg_t[4], fpart_t[4], total;
    int splits;
    DynDecLayout(int h, int64_t Nn, int64_t E) {
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, hh_ = (size_t)h;
        for (auto& v : A) v = take(nn * hh_);
        for (auto& v : S) v = take(nn * hh_);
        Tm = take(ee * hh_ * 4); M = take(ee * hh_); M2 = take(ee * hh_);        // Tm: one plane per edge type
        agg_h = take(nn * hh_); agg_p = take(nn * hh_);
        ext = take(nn * 6); rel = take(nn * 15); Rinv = take(nn * 4);
        ea = take(ee * 24); ea15 = take(ee * 15); epos = take(ee * 3); bimg = take((ee + 15) / 16 * 16 * hh_ * 3 / 2);
        fimg = take((size_t)15 * hh_ * hh_ * 3 / 2); fout = take(ee * hh_);
        splits = S2SPriorLayout::filter_splits(h, E) * S2SPriorLayout::filter_rsplits15(h, E);     // planes of the filter GEMM
        fpart = take(splits > 1 ? ee * hh_ * splits : 0);
        ewn = take(ee * 4);
        rp = take(nn * hh_); ip = take(nn * hh_); np_ = take(nn * hh_); hh = take(nn * hh_);
        o1 = take(nn * hh_); o2 = take(nn * hh_);
        for (auto& v : list) v = take(ee * 2);
        counts = take(64);
        // all edge types' filters in one launch (k_s2s_filter_split_types): a B-operand image and the planes per type
        for (auto& v : bimg_t) v = take((ee + 15) / 16 * 16 * hh_ * 3 / 2);
        for (auto& v : fpart_t) v = take(ee * hh_ * (size_t)(splits > 1 ? splits : 1));
        total = off;
    }
};
}  // namespace

size_t aether_dyn_decoder_workspace_bytes(int hidden, int64_t n_nodes, int64_t n_edges) {
    if (hidden <= 0 || n_nodes <= 0 || n_edges < 0) return 0;
    return DynDecLayout(hidden, n_nodes, n_edges).total;
}

int aether_dyn_decoder_step(const AetherDynDecoderParams* p, int hidden, int num_edge_types, int skip_first, int polar,
                            int64_t n_nodes, int64_t n_edges, const float* inputs, const float* hidden_in,
                            const float* edge_w, const float* field, const float* edge_state, const int64_t* send,
                            const int64_t* recv, const int64_t* agg_order, const int64_t* agg_rowptr, float agg_div,
                            void* workspace, size_t workspace_bytes, float* outputs, float* hidden_out, void* stream) {
    return aether_dyn_decoder_step_batched(p, hidden, num_edge_types, skip_first, polar, n_nodes, n_edges, inputs, hidden_in,
                                           edge_w, field, edge_state, nullptr, nullptr, send, recv, agg_order, agg_rowptr,
                                           agg_div, nullptr, workspace, workspace_bytes, outputs, hidden_out, stream);
}

// Canonical state / frames of the present objects when another stage of the same step has them already (aether_dyn_step:
// the prior step computes exactly these from the same rows): [n][6], [n][15], [n][4]
// (ext == nullptr: the decoder computes its own, and only counts_zeroed is read)
struct DynSharedNodes { const float* ext; const float* rel; const float* Rinv; bool counts_zeroed; };
static int dyn_decoder_impl(const AetherDynDecoderParams* p, int hidden, int num_edge_types, int skip_first,
                            int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                            const float* hidden_in, const float* edge_w, const float* field,
                            const float* edge_state, const int64_t* state_send, const int64_t* state_recv,
                            const int64_t* send, const int64_t* recv, const int64_t* agg_order,
                            const int64_t* agg_rowptr, float agg_div, const float* agg_div_node, void* workspace,
                            size_t workspace_bytes, float* outputs, float* hidden_out, void* stream,
                            const DynSharedNodes* shared);

int aether_dyn_decoder_step_batched(const AetherDynDecoderParams* p, int hidden, int num_edge_types, int skip_first,
                                    int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                                    const float* hidden_in, const float* edge_w, const float* field,
                                    const float* edge_state, const int64_t* state_send, const int64_t* state_recv,
                                    const int64_t* send, const int64_t* recv, const int64_t* agg_order,
                                    const int64_t* agg_rowptr, float agg_div, const float* agg_div_node, void* workspace,
                                    size_t workspace_bytes, float* outputs, float* hidden_out, void* stream) {
    return dyn_decoder_impl(p, hidden, num_edge_types, skip_first, polar, n_nodes, n_edges, inputs, hidden_in, edge_w, field,
                            edge_state, state_send, state_recv, send, recv, agg_order, agg_rowptr, agg_div, agg_div_node,
                            workspace, workspace_bytes, outputs, hidden_out, stream, nullptr);
}

static int dyn_decoder_impl(const AetherDynDecoderParams* p, int hidden, int num_edge_types, int skip_first,
                            int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                            const float* hidden_in, const float* edge_w, const float* field,
                            const float* edge_state, const int64_t* state_send, const int64_t* state_recv,
                            const int64_t* send, const int64_t* recv, const int64_t* agg_order,
                            const int64_t* agg_rowptr, float agg_div, const float* agg_div_node, void* workspace,
                            size_t workspace_bytes, float* outputs, float* hidden_out, void* stream,
                            const DynSharedNodes* shared) {
    if (!p || !inputs || !hidden_in || !field || !workspace || !outputs || !hidden_out)
        return fail(AETHER_EINVAL, "dyn_decoder: null pointer");
    if (n_edges > 0 && (!edge_w || !send || !recv || !agg_order || !agg_rowptr))
        return fail(AETHER_EINVAL, "dyn_decoder: null edge pointer");
    if (hidden < 128 || hidden % 128 != 0) return fail(AETHER_EINVAL, "dyn_decoder: hidden must be a multiple of 128");
    if (num_edge_types < 1 || num_edge_types > 4) return fail(AETHER_EINVAL, "dyn_decoder: 1..4 edge types");
    if (skip_first && num_edge_types < 2) return fail(AETHER_EINVAL, "dyn_decoder: skip_first needs two edge types");
    if (n_nodes <= 0 || n_edges < 0) return fail(AETHER_EINVAL, "dyn_decoder: bad sizes");
    if (n_edges > 0 && !agg_div_node && !(agg_div > 0.0f)) return fail(AETHER_EINVAL, "dyn_decoder: agg_div must be positive");
    if ((state_send || state_recv) && !(edge_state && state_send && state_recv))
        return fail(AETHER_EINVAL, "dyn_decoder: state_send / state_recv come with edge_state, both or neither");
    constexpr int D = 2;
    const int h = hidden, K = num_edge_types, k0 = skip_first ? 1 : 0;
    DynDecLayout L(h, n_nodes, n_edges);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "dyn_decoder: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int64_t Nn = n_nodes, E = n_edges;
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    auto elist = [&](int k) { return reinterpret_cast<int64_t*>(ws + L.list[k]); };
    // ---- canonical state and frames of the present objects (:790)
    const float *n_ext = wp(L.ext), *n_rel = wp(L.rel), *n_Rinv = wp(L.Rinv);
    if (shared && shared->ext) { n_ext = shared->ext; n_rel = shared->rel; n_Rinv = shared->Rinv; }
    else k_s2s_aug_nodes<2><<<blocks(Nn), dim3(256), 0, st>>>(nullptr, wp(L.rel), wp(L.Rinv), Nn, inputs, field, wp(L.ext));
    S2SJobs T;
    if (E > 0) {
        if (!(shared && shared->counts_zeroed)) HIP_OK(hipMemsetAsync(counts, 0, 64 * sizeof(int), st));
        // the per-type edge lists and the weights / norm in one launch (lists are take()n back to back, one stride apart)
        const size_t list_stride = (L.list[1] - L.list[0]) / sizeof(int64_t);
        k_s2s_select_all<<<blocks(E), dim3(256), 0, st>>>(edge_w, K, k0, 1.0f / (float)(K - k0), wp(L.ewn), elist(0), list_stride,
                                                         counts, E);
        // ---- messages from the hidden states, each type / norm (:797-814): the receiver / sender halves of every
        // type's first layer in one launch (A[k], S[k] lie back to back), tanh of all types in one (it also clears M, M2)
        T.n = 0;
        for (int k = k0; k < K; ++k) {
            T.j[T.n++] = s2s_job(0, p->msg_fc1_w[k], 2 * h, p->msg_fc1_b[k], hidden_in, h, wp(L.A[k]), h, h, h, Nn);
            T.j[T.n++] = s2s_job(0, p->msg_fc1_w[k] + h, 2 * h, nullptr, hidden_in, h, wp(L.S[k]), h, h, h, Nn);
        }
        if (int rc = s2s_launch_jobs(T, st)) return rc;
        k_s2s_pair_tanh_all<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(wp(L.A[0]), wp(L.S[0]), Nn, send, recv, edge_w, K, k0, wp(L.Tm),
                                                                      wp(L.M), wp(L.M2), h, E, 1);
        // the second layer: one launch per type (the weights need not be one-hot: an edge can sit in several lists, and
        // the launches' accumulation into M is ordered by the stream)
        for (int k = k0; k < K; ++k)
            if (s2s_linear(3, p->msg_fc2_w[k], h, p->msg_fc2_b[k], wp(L.Tm) + (size_t)k * E * h, wp(L.M), h, h, E, h, wp(L.ewn) + k, K,
                           1, st, elist(k), elist(k), counts + k)) return AETHER_EINVAL;    // T rows are by edge id
        k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.M), agg_order, agg_rowptr, wp(L.agg_h), h, agg_div, agg_div_node);
        // ---- edge features [9 | canonical state of the receiver 6] and positions (:821-825): the first 15 of the
        // 24 columns aether_s2s_localize's edge kernel writes (edge | canonical | origin-edge features)
        k_s2s_aug_edges<2><<<blocks(E), dim3(256), 0, st>>>(edge_state ? edge_state : n_ext, send, recv, n_rel, polar,
                                                           wp(L.ea15), wp(L.epos), E, state_send, state_recv, 15);
        // ---- messages from the present state: one anisotropic filter per edge type, ReLU (:827-835)
        bool all_types_at_once = true;
        for (int k = k0; k < K; ++k) all_types_at_once = all_types_at_once && p->filt_image[k] != nullptr;
        if (all_types_at_once) {
            // three launches for all edge types (was four per type): B-operand images, the filter GEMMs, and the
            // weighted sum of their ReLUs (same order of additions as the per-type launches)
            FilterTypes T{};
            const int nT = K - k0;
            for (int t = 0; t < nT; ++t) {
                T.img[t] = reinterpret_cast<const f16x8*>(p->filt_image[k0 + t]);
                T.b2[t] = p->filt_b2[k0 + t]; T.w0[t] = p->filt_w0[k0 + t]; T.b0[t] = p->filt_b0[k0 + t];
                T.bimg[t] = reinterpret_cast<f16x8*>(ws + L.bimg_t[t]);
                T.out[t] = wp(L.fpart_t[t]);
            }
            const int splits = S2SPriorLayout::filter_splits(h, E), rs = S2SPriorLayout::filter_rsplits15(h, E);
            k_s2s_filter_bimg_types<3><<<filter_bimg_grid(E, nT), dim3(256), 0, st>>>(
                wp(L.epos), T, 1, h, E);
            const int64_t units = ((E + 255) / 256) * (h / 64) * splits * rs;
            const dim3 grid((unsigned)(units < FILTER_WGS ? units : FILTER_WGS), (unsigned)nT);
            const size_t lds = filt_lds_bytes(15);
            if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_s2s_filter_split_types<15>), lds)) return AETHER_EHIP;
            // All types' filter GEMMs as ONE launch.  Round 3 launched them per type: with this kernel as a graph node, replays
            // of a captured step enqueued behind a running one ended in a GPU memory access fault (20 of 20 runs).  The node
            // was the only one of the step that consumed implicit (hidden) kernel arguments -- gridDim.x, i.e.
            // hidden_block_count_x at the end of a 480-byte kernarg segment -- on a 2-D grid; with the workgroup count as an
            // explicit argument (no hidden_* entries left, 228-byte segment; tools/isa_check.py rule R4 keeps it so) the same
            // reproducer passes (DESIGN.md 4.11c, gpurun_out/r04_repro_types_explicit.txt).
            k_s2s_filter_split_types<15><<<grid, dim3(512), lds, st>>>(T, wp(L.ea15), h, E, splits, rs, (int)grid.x);
            k_dyn_filter_combine<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(T, nT, splits * rs, edge_w, K, k0, wp(L.M2), h, E);
        } else {
            for (int k = k0; k < K; ++k) {
                if (int rc = dyn_filter(p->filt_w0[k], p->filt_b0[k], p->filt_w2[k], p->filt_b2[k], p->filt_image[k], wp(L.ea15),
                                        wp(L.epos), ws + L.bimg, ws + L.fimg, wp(L.fpart), wp(L.fout), h, E, st)) return rc;
                k_s2s_relu_scale_acc<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(wp(L.fout), edge_w + k, K, wp(L.M2), h, E);
            }
        }
        k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.M2), agg_order, agg_rowptr, wp(L.agg_p), h, agg_div, agg_div_node);
    } else {
        HIP_OK(hipMemsetAsync(wp(L.agg_h), 0, (size_t)Nn * h * 4, st));
        HIP_OK(hipMemsetAsync(wp(L.agg_p), 0, (size_t)Nn * h * 4, st));
    }
    // ---- GRU-style gate (:845-852): input_* see the canonical state (6 columns of rel_feat)
    // two launches: the three input products, then [present | hidden] as a two-segment K on top of them and hidden_h
    {   // the three input products read the 6 canonical-state columns of rel_feat: one narrow launch, no padded copies
        NarrowLayers NL;
        NL.n = 3;
        NL.W[0] = p->input_r_w; NL.b[0] = p->input_r_b; NL.Y[0] = wp(L.rp);
        NL.W[1] = p->input_i_w; NL.b[1] = p->input_i_b; NL.Y[1] = wp(L.ip);
        NL.W[2] = p->input_n_w; NL.b[2] = p->input_n_b; NL.Y[2] = wp(L.np_);
        k_s2s_narrow_layers<<<blocks(Nn * (h / 4)), dim3(256), 0, st>>>(NL, n_rel, 15, 6, h, 0, Nn);
    }
    T.n = 0;
    auto two_seg = [&](const float* pw, const float* pb, const float* hw, float* y) {
        S2SJob J = s2s_job(0, pw, h, pb, wp(L.agg_p), h, y, h, h, h, Nn);
        J.accumulate = 1;
        if (hw) { J.W2 = hw; J.ldw2 = h; J.X2 = wp(L.agg_h); J.ldx2 = h; J.K2 = h; }
        return J;
    };
    T.j[T.n++] = two_seg(p->present_r_w, p->present_r_b, p->hidden_r_w, wp(L.rp));
    T.j[T.n++] = two_seg(p->present_i_w, p->present_i_b, p->hidden_i_w, wp(L.ip));
    T.j[T.n++] = two_seg(p->present_n_w, p->present_n_b, nullptr, wp(L.np_));
    T.j[T.n++] = s2s_job(0, p->hidden_h_w, h, nullptr, wp(L.agg_h), h, wp(L.hh), h, h, h, Nn);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    k_s2s_gate<<<blocks(Nn * h), dim3(256), 0, st>>>(wp(L.rp), wp(L.ip), wp(L.np_), wp(L.hh), hidden_in, hidden_out, Nn * h);
    // ---- output MLP, rotate back, residual (:855-861)
    if (s2s_linear(2, p->out1_w, h, p->out1_b, hidden_out, wp(L.o1), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(2, p->out2_w, h, p->out2_b, wp(L.o1), wp(L.o2), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    k_s2s_out_globalize<2><<<dim3((unsigned)((Nn + 3) / 4)), dim3(256), 0, st>>>(wp(L.o2), p->out3_w, p->out3_b, h, inputs, n_Rinv,
                                                                                outputs, Nn);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// ------------------------------------------------------------------ variable-N encoder prior step and field (N2)
namespace {
struct DynPriorLayout {
    size_t ext, rel, Rinv, ea, ea15, epos, bimg, fimg, eaf, fpart, X0, X1, X3, Ps, Pr, T1, X4, G, Y1, Y2, bn, total;
    int splits;
    DynPriorLayout(int h, int R, int ph, int64_t Nn, int64_t E) {
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, hh = (size_t)h;
        ext = take(nn * 6); rel = take(nn * 15); Rinv = take(nn * 4);
        ea = take(ee * 24); ea15 = take(ee * 15); epos = take(ee * 3); bimg = take((ee + 15) / 16 * 16 * hh * 3 / 2);
        fimg = take((size_t)15 * hh * hh * 3 / 2); eaf = take(ee * hh);
        splits = S2SPriorLayout::filter_splits(h, E) * S2SPriorLayout::filter_rsplits15(h, E);     // planes of the filter GEMM
        fpart = take(splits > 1 ? ee * hh * splits : 0);
        X0 = take(nn * hh); X1 = take(nn * hh); X3 = take(nn * hh); Ps = take(nn * hh); Pr = take(nn * hh);
        T1 = take(ee * hh); X4 = take(ee * hh); G = take(ee * 4 * (size_t)R);
        Y1 = take(ee * (size_t)(ph > 0 ? ph : 1)); Y2 = take(ee * (size_t)(ph > 0 ? ph : 1));
        bn = take(6 * hh);
        total = off;
    }
};
}  // namespace

size_t aether_dyn_prior_workspace_bytes(int hidden, int rnn_hidden, int prior_hidden, int64_t n_nodes, int64_t n_edges) {
    if (hidden <= 0 || rnn_hidden <= 0 || n_nodes <= 0 || n_edges < 0) return 0;
    return DynPriorLayout(hidden, rnn_hidden, prior_hidden, n_nodes, n_edges).total;
}

// seq: null (one prior step from h0 / c0), or the sequence encoder's tail on the same rows -- the LSTM step from the zero state
// and both heads (host_nri_chain.inc 3b); h0, c0 and c1 are not read or written then.
static int dyn_prior_impl(const AetherDynPriorParams* p, int hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                          int num_edge_types, int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                          const float* field, const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                          const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                          float* logits, float* h1, float* c1, void* stream, const NriSeqTail* seq);
int aether_dyn_prior_step(const AetherDynPriorParams* p, int hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                          int num_edge_types, int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                          const float* field, const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                          const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                          float* logits, float* h1, float* c1, void* stream) {
    return dyn_prior_impl(p, hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, polar, n_nodes, n_edges, inputs, field,
                          h0, c0, send, recv, order, rowptr, workspace, workspace_bytes, logits, h1, c1, stream, nullptr);
}
static int dyn_prior_impl(const AetherDynPriorParams* p, int hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                          int num_edge_types, int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                          const float* field, const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                          const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                          float* logits, float* h1, float* c1, void* stream, const NriSeqTail* seq) {
    if (!p || !inputs || !field || !send || !recv || !order || !rowptr || !workspace || !logits || !h1 ||
        (!seq && (!h0 || !c0 || !c1)))
        return fail(AETHER_EINVAL, "dyn_prior: null pointer");
    if (hidden < 128 || hidden % 128 != 0) return fail(AETHER_EINVAL, "dyn_prior: hidden must be a multiple of 128");
    if (rnn_hidden < 16 || rnn_hidden % 16 != 0) return fail(AETHER_EINVAL, "dyn_prior: rnn_hidden must be a multiple of 16");
    if (prior_layers < 1 || prior_layers > 4) return fail(AETHER_EINVAL, "dyn_prior: 1..4 prior layers");
    if (prior_layers > 1 && (prior_hidden < 16 || prior_hidden % 16 != 0))
        return fail(AETHER_EINVAL, "dyn_prior: prior_hidden must be a multiple of 16");
    if (num_edge_types < 1 || num_edge_types > 4 || n_nodes <= 0 || n_edges <= 0)
        return fail(AETHER_EINVAL, "dyn_prior: bad sizes");
    constexpr int D = 2;
    const int h = hidden, R = rnn_hidden, K = num_edge_types;
    DynPriorLayout L(h, R, prior_hidden, n_nodes, n_edges);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "dyn_prior: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int64_t Nn = n_nodes, E = n_edges;
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // ---- canonical states, edge features, anisotropic filter (:531-539)
    k_s2s_aug_nodes<2><<<blocks(Nn), dim3(256), 0, st>>>(nullptr, wp(L.rel), wp(L.Rinv), Nn, inputs, field, wp(L.ext));
    k_s2s_aug_edges<2><<<blocks(E), dim3(256), 0, st>>>(wp(L.ext), send, recv, wp(L.rel), polar, wp(L.ea15), wp(L.epos), E, nullptr,
                                                       nullptr, 15);
    if (int rc = dyn_filter(p->filt_w0, p->filt_b0, p->filt_w2, p->filt_b2, p->filt_image, wp(L.ea15), wp(L.epos), ws + L.bimg,
                            ws + L.fimg, wp(L.fpart), wp(L.eaf), h, E, st)) return rc;
    // ---- x = sum over in-edges + mlp1(canonical state) (:541-542); RefNRIMLP (eval): Linear-ELU-Linear-ELU-BatchNorm
    float* bns[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    const float* bnp[3][4] = {{p->mlp1_bn_w, p->mlp1_bn_b, p->mlp1_bn_mean, p->mlp1_bn_var},
                              {p->mlp3_bn_w, p->mlp3_bn_b, p->mlp3_bn_mean, p->mlp3_bn_var},
                              {p->mlp4_bn_w, p->mlp4_bn_b, p->mlp4_bn_mean, p->mlp4_bn_var}};
    BnSets BS{};
    bool any_bn = false;
    for (int j = 0; j < 3; ++j) {
        if (!bnp[j][0]) continue;
        if (!bnp[j][1] || !bnp[j][2] || !bnp[j][3]) return fail(AETHER_EINVAL, "dyn_prior: incomplete BatchNorm pointers");
        bns[j][0] = wp(L.bn) + 2 * j * h; bns[j][1] = wp(L.bn) + (2 * j + 1) * h;
        BS.w[j] = bnp[j][0]; BS.b[j] = bnp[j][1]; BS.mean[j] = bnp[j][2]; BS.var[j] = bnp[j][3];
        BS.scale[j] = bns[j][0]; BS.shift[j] = bns[j][1];
        any_bn = true;
    }
    if (any_bn) k_s2s_bn_affine_sets<<<dim3(blocks(h).x, 3), dim3(256), 0, st>>>(BS, h);      // the three layers in one launch
    k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.eaf), order, rowptr, wp(L.X0), h, 1.0f);
    {   // mlp1's first layer reads the 6 canonical-state columns: narrow launch instead of two padded copies + a GEMM
        NarrowLayers NL;
        NL.n = 1;
        NL.W[0] = p->mlp1_w0; NL.b[0] = p->mlp1_b0; NL.Y[0] = wp(L.X1);
        k_s2s_narrow_layers<<<blocks(Nn * (h / 4)), dim3(256), 0, st>>>(NL, wp(L.rel), 15, 6, h, 4, Nn);
    }
    if (s2s_linear(4, p->mlp1_w3, h, p->mlp1_b3, wp(L.X1), wp(L.X0), h, h, Nn, h, nullptr, 0, 1, st, nullptr, nullptr, nullptr,
                   bns[0][0], bns[0][1])) return AETHER_EINVAL;
    if (s2s_linear(4, p->mlp3_w0, h, p->mlp3_b0, wp(L.X0), wp(L.X1), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(4, p->mlp3_w3, h, p->mlp3_b3, wp(L.X1), wp(L.X3), h, h, Nn, h, nullptr, 0, 0, st, nullptr, nullptr, nullptr,
                   bns[1][0], bns[1][1])) return AETHER_EINVAL;
    // ---- mlp4 on [x_send | x_recv | edge] (:545-547)
    {                                                   // the three column blocks of the first layer in one launch
        S2SJobs T;
        T.n = 0;
        T.j[T.n++] = s2s_job(0, p->mlp4_w0, 3 * h, p->mlp4_b0, wp(L.X3), h, wp(L.Ps), h, h, h, Nn);
        T.j[T.n++] = s2s_job(0, p->mlp4_w0 + h, 3 * h, nullptr, wp(L.X3), h, wp(L.Pr), h, h, h, Nn);
        T.j[T.n++] = s2s_job(0, p->mlp4_w0 + 2 * h, 3 * h, nullptr, wp(L.eaf), h, wp(L.T1), h, h, h, E);
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    }
    k_s2s_edge_sum_elu<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(wp(L.T1), wp(L.Ps), wp(L.Pr), send, recv, h, E);
    if (s2s_linear(4, p->mlp4_w3, h, p->mlp4_b3, wp(L.T1), wp(L.X4), h, h, E, h, nullptr, 0, 0, st, nullptr, nullptr, nullptr,
                   bns[2][0], bns[2][1])) return AETHER_EINVAL;
    if (seq) {   // ---- every frame from the zero state, prior_fc_out and encoder_fc_out (:620-668)
        if (int rc = nri_seq_tail(p->lstm_w_ih, p->lstm_b_ih, p->lstm_b_hh, p->prior_w, p->prior_b, prior_layers, prior_hidden, *seq,
                                  h, R, K, E, wp(L.X4), h1, wp(L.Y1), wp(L.Y2), logits, st)) return rc;
        HIP_OK(hipGetLastError());
        return AETHER_OK;
    }
    // ---- one LSTM step per edge, prior_fc_out (:688-696)
    if (int rc = nri_lstm_two_launch(p->lstm_w_ih, p->lstm_w_hh, p->lstm_b_ih, p->lstm_b_hh, h, R, E, wp(L.X4), h0, c0, wp(L.G), h1,
                                     c1, st)) return rc;
    if (int rc = nri_head_linear(p->prior_w, p->prior_b, prior_layers, R, prior_hidden, K, E, h1, wp(L.Y1), wp(L.Y2), logits, st))
        return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_dyn_field_workspace_bytes(int64_t n_points, int hidden) {
    if (n_points <= 0 || hidden <= 0) return 0;
    const size_t n = (size_t)n_points, h = (size_t)hidden;
    return align_up(n * 16 * 4, 256) + align_up(h * 16 * 4, 256) + align_up(n * 2 * h * 4, 256) + 2 * align_up(n * h * 4, 256) + 256;
}

int aether_dyn_field(const AetherDynFieldQueryParams* p, int hidden, int64_t n_points, const float* x, void* workspace,
                     size_t workspace_bytes, float* field, void* stream) {
    if (!p || !x || !workspace || !field || !p->B || !p->ang_w || !p->ang_b || !p->w0 || !p->b0 || !p->w2 || !p->b2 ||
        !p->w4 || !p->b4)
        return fail(AETHER_EINVAL, "dyn_field: null pointer");
    if (hidden < 32 || hidden % 32 != 0) return fail(AETHER_EINVAL, "dyn_field: hidden must be a multiple of 32");
    if (n_points <= 0) return fail(AETHER_EINVAL, "dyn_field: bad sizes");
    if (workspace_bytes < aether_dyn_field_workspace_bytes(n_points, hidden))
        return fail(AETHER_ESPACE, "dyn_field: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int h = hidden, half = hidden / 2;
    const size_t n = (size_t)n_points;
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = ws + off; off += align_up(bytes, 256); return reinterpret_cast<float*>(q); };
    float* dir = take(n * 16 * 4);
    float* awp = take((size_t)h * 16 * 4);
    float* cat = take(n * 2 * h * 4);                               // [rff (h) | angular embedding (h)]
    float* h1 = take(n * h * 4);
    float* h2 = take(n * h * 4);
    auto blocks = [](int64_t c) { return dim3((unsigned)((c + 255) / 256)); };
    (void)dir; (void)awp; (void)half;
    k_dyn_field_embed<<<blocks(n_points * h), dim3(256), 0, st>>>(x, p->B, p->ang_w, p->ang_b, h, cat, n_points);
    if (s2s_linear(1, p->w0, 2 * h, p->b0, cat, h1, h, 2 * h, n_points, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(1, p->w2, h, p->b2, h1, h2, h, h, n_points, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->w4, h, p->b4, h2, field, 2, h, n_points, 2, nullptr, 0, 0, st)) return AETHER_EINVAL;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// ------------------------------------------------------------------ kNN edge builder (N2)
namespace {
struct KnnLayout {
    size_t nbr, cnt, node_off, edge_off, total;
    KnnLayout(int64_t S, int N, int k) {
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
        nbr = take((size_t)S * N * k * 4); cnt = take((size_t)S * N * 4);
        node_off = take((size_t)S * 8); edge_off = take((size_t)S * 8);
        total = off;
    }
};
}  // namespace

size_t aether_knn_workspace_bytes(int64_t n_scenes, int n_objects, int k) {
    if (n_scenes <= 0 || n_objects <= 0 || k <= 0) return 0;
    return KnnLayout(n_scenes, n_objects, k).total + 256;
}

static int knn_edges_impl(const float* x, int x_stride, const float* masks, int64_t n_scenes, int n_objects, int k,
                          int64_t* send, int64_t* recv, int64_t* scene_edges, int64_t* scene_nodes, int64_t* totals,
                          void* workspace, size_t workspace_bytes, void* stream, bool sums_zeroed);
int aether_knn_edges(const float* x, int x_stride, const float* masks, int64_t n_scenes, int n_objects, int k,
                     int64_t* send, int64_t* recv, int64_t* scene_edges, int64_t* scene_nodes, int64_t* totals,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return knn_edges_impl(x, x_stride, masks, n_scenes, n_objects, k, send, recv, scene_edges, scene_nodes, totals, workspace,
                          workspace_bytes, stream, false);
}
static int knn_edges_impl(const float* x, int x_stride, const float* masks, int64_t n_scenes, int n_objects, int k,
                          int64_t* send, int64_t* recv, int64_t* scene_edges, int64_t* scene_nodes, int64_t* totals,
                          void* workspace, size_t workspace_bytes, void* stream, bool sums_zeroed) {
    if (!x || !masks || !send || !recv || !scene_edges || !scene_nodes || !totals || !workspace)
        return fail(AETHER_EINVAL, "knn_edges: null pointer");
    if (n_scenes <= 0 || n_scenes > INT32_MAX || n_objects <= 0 || n_objects > KNN_MAX_OBJECTS || x_stride < 2)
        return fail(AETHER_EINVAL, "knn_edges: bad sizes (at most 8192 objects per scene, x_stride >= 2)");
    if (k < 1 || k > KNN_MAX_K) return fail(AETHER_EINVAL, "knn_edges: k must be in 1..16");
    const KnnLayout L(n_scenes, n_objects, k);
    if (workspace_bytes < L.total + 256) return fail(AETHER_ESPACE, "knn_edges: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    int* nbr = reinterpret_cast<int*>(ws + L.nbr);
    int* cnt = reinterpret_cast<int*>(ws + L.cnt);
    int64_t* node_off = reinterpret_cast<int64_t*>(ws + L.node_off);
    int64_t* edge_off = reinterpret_cast<int64_t*>(ws + L.edge_off);
    const int N = n_objects;
    const size_t lds_sel = (size_t)3 * N * 4 + 257 * 4, lds_wr = (size_t)2 * N * 4 + 257 * 4;
    if (ensure_dynamic_lds((const void*)k_knn_select, lds_sel) || ensure_dynamic_lds((const void*)k_knn_write, lds_wr))
        return AETHER_EHIP;
    if (sums_zeroed) {                                    // (aether_dyn_step_batched: k_dynb_present has cleared them)
    } else if (scene_nodes == scene_edges + n_scenes) {  // back to back: one memset node
        HIP_OK(hipMemsetAsync(scene_edges, 0, (size_t)2 * n_scenes * sizeof(int64_t), st));
    } else {
        HIP_OK(hipMemsetAsync(scene_nodes, 0, (size_t)n_scenes * sizeof(int64_t), st));
        HIP_OK(hipMemsetAsync(scene_edges, 0, (size_t)n_scenes * sizeof(int64_t), st));
    }
    // few large scenes: several workgroups per scene (each stages the scene and takes a slice of its objects)
    int per_scene = 1;
    while (per_scene * 256 < N && n_scenes * per_scene < 512) per_scene *= 2;
    k_knn_select<<<dim3((unsigned)n_scenes, (unsigned)per_scene), dim3(256), lds_sel, st>>>(x, x_stride, masks, N, k, nbr, cnt,
                                                                                           scene_nodes, scene_edges);
    if (n_scenes == 1 && scene_nodes == scene_edges + 1) {      // one scene: nothing to scan
        k_knn_write<<<dim3(1), dim3(256), lds_wr, st>>>(masks, nbr, cnt, N, k, nullptr, nullptr, send, recv, scene_edges, totals);
    } else {
        k_knn_scan<<<dim3(1), dim3(1024), 0, st>>>(scene_nodes, scene_edges, n_scenes, node_off, edge_off, totals);
        k_knn_write<<<dim3((unsigned)n_scenes), dim3(256), lds_wr, st>>>(masks, nbr, cnt, N, k, node_off, edge_off, send, recv);
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

