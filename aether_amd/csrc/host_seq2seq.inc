// Host side of the C ABI: seq2seq steps (SURVEY 8a rows A8-A10) and the seq2seq dynamic-field variant (8f N3).  Included by aether_hip.hip inside its extern "C" block (one translation
// unit: the kernels live in anonymous namespaces); not a stand-alone source file.

size_t aether_s2s_field_workspace_bytes(int64_t n_points, int hidden) {
    if (n_points <= 0 || hidden <= 0) return 0;
    return (size_t)3 * (size_t)n_points * (size_t)hidden * sizeof(float) + 768;
}

int aether_s2s_field(const AetherS2SFieldParams* p, int num_dims, int hidden, int64_t n_points, const float* x,
                     int x_stride, void* workspace, size_t workspace_bytes, float* field, void* stream) {
    if (!p || !x || !workspace || !field || !p->B || !p->w0 || !p->b0 || !p->w2 || !p->b2 || !p->w4 || !p->b4)
        return fail(AETHER_EINVAL, "s2s_field: null pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "s2s_field: num_dims must be 2 or 3");
    if (hidden < 32 || hidden % 32 != 0) return fail(AETHER_EINVAL, "s2s_field: hidden must be a multiple of 32");
    if (n_points <= 0 || x_stride < num_dims) return fail(AETHER_EINVAL, "s2s_field: bad sizes");
    if (workspace_bytes < aether_s2s_field_workspace_bytes(n_points, hidden))
        return fail(AETHER_ESPACE, "s2s_field: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = align_up((size_t)n_points * hidden * sizeof(float), 256);
    float* gamma = reinterpret_cast<float*>(workspace);
    float* h1 = reinterpret_cast<float*>((char*)workspace + plane);
    float* h2 = reinterpret_cast<float*>((char*)workspace + 2 * plane);
    const int half = hidden / 2;
    const unsigned rb = (unsigned)((n_points * half + 255) / 256);
    if (num_dims == 2) k_s2s_rff<2><<<dim3(rb), dim3(256), 0, st>>>(x, x_stride, p->B, half, gamma, n_points);
    else k_s2s_rff<3><<<dim3(rb), dim3(256), 0, st>>>(x, x_stride, p->B, half, gamma, n_points);
    if (s2s_linear(1, p->w0, hidden, p->b0, gamma, h1, hidden, hidden, n_points, hidden, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(1, p->w2, hidden, p->b2, h1, h2, hidden, hidden, n_points, hidden, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->w4, hidden, p->b4, h2, field, num_dims, hidden, n_points, num_dims, nullptr, 0, 0, st)) return AETHER_EINVAL;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_localize(int num_dims, int64_t n_nodes, int64_t n_edges, const float* x, const int64_t* send,
                        const int64_t* recv, int polar, float* rel_feat, float* Rinv, float* edge_attr,
                        float* edge_pos, void* stream) {
    if (!x || !rel_feat || !Rinv) return fail(AETHER_EINVAL, "s2s_localize: null pointer");
    if (n_edges > 0 && (!send || !recv || !edge_attr || !edge_pos))
        return fail(AETHER_EINVAL, "s2s_localize: null edge pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "s2s_localize: num_dims must be 2 or 3");
    if (n_nodes <= 0 || n_edges < 0) return fail(AETHER_EINVAL, "s2s_localize: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n_nodes + 255) / 256), eb = (unsigned)((n_edges + 255) / 256);
    if (num_dims == 2) {
        k_s2s_aug_nodes<2><<<dim3(nb), dim3(256), 0, st>>>(x, rel_feat, Rinv, n_nodes);
        if (n_edges > 0)
            k_s2s_aug_edges<2><<<dim3(eb), dim3(256), 0, st>>>(x, send, recv, rel_feat, polar, edge_attr, edge_pos, n_edges);
    } else {
        k_s2s_aug_nodes<3><<<dim3(nb), dim3(256), 0, st>>>(x, rel_feat, Rinv, n_nodes);
        if (n_edges > 0)
            k_s2s_aug_edges<3><<<dim3(eb), dim3(256), 0, st>>>(x, send, recv, rel_feat, polar, edge_attr, edge_pos, n_edges);
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

namespace {
// Y[N][ldy] = act(X[N][K] W^T + b) [* scale] [+ Y]; act: 0 none, 1 SiLU, 2 ReLU, 3 tanh, 4 ELU
int s2s_linear(int act, const float* W, int ldw, const float* b, const float* X, float* Y, int M, int K, int64_t N,
               int ldy, const float* scale, int sstride, int accumulate, hipStream_t st, const int64_t* xidx,
               const int64_t* yidx, const int* n_dev, const float* post_scale, const float* post_shift,
               const float* film_gamma, const float* film_beta, int film_rows) {
    if (K % 16 != 0) return fail(AETHER_EINVAL, "s2s_linear: K must be a multiple of 16");
    // A wave's k-step costs (MT x NT) MFMAs x 32 cycles whatever the problem size: with few rows (the reference's
    // 5-object graphs: 640 nodes, 2,560 edges) 64 x 32 blocks per wave leave most SIMDs idle and every GEMM takes the
    // 32 k-steps x 0.43 us of one wave; 16 x 32 blocks give four times the waves.
    const bool big = M >= 128 && ((N + 63) / 64) * ((M + 127) / 128) >= LINEAR_SMALL_WGS;
    const bool wide = big && N >= 16384;             // 64 points per wave once there are enough workgroups
    const int nt = wide ? 4 : 2;
    // ... and when even those are few (a node-level layer of 640 rows), the waves of a workgroup split the k-groups
    const bool ksplit = !big && g_linear_kwaves == 4 && K >= 128 && ((N + 63) / 64) * ((M + 31) / 32) < 1024;
    const dim3 grid(ksplit ? (unsigned)((N + 31) / 32) : (unsigned)((N + 32 * nt - 1) / (32 * nt)),
                    (unsigned)(big ? (M + 127) / 128 : ksplit ? (M + 15) / 16 : (M + 31) / 32));
#define S2S_ARGS W, b, X, Y, M, K, ldw, N, ldy, scale, sstride, accumulate, xidx, yidx, n_dev, post_scale, post_shift, \
                 film_gamma, film_beta, film_rows
#define S2S_CASE(A)                                                                     \
    if (wide) k_s2s_linear<A, 4, 4><<<grid, dim3(256), 0, st>>>(S2S_ARGS);              \
    else if (big) k_s2s_linear<A, 4, 2><<<grid, dim3(256), 0, st>>>(S2S_ARGS);          \
    else if (ksplit) k_s2s_linear<A, 1, 2, 2, 4><<<grid, dim3(256), 0, st>>>(S2S_ARGS);  \
    else k_s2s_linear<A, 1, 2><<<grid, dim3(256), 0, st>>>(S2S_ARGS)
    if (act == 0) { S2S_CASE(0); } else if (act == 1) { S2S_CASE(1); } else if (act == 2) { S2S_CASE(2); }
    else if (act == 3) { S2S_CASE(3); } else { S2S_CASE(4); }
#undef S2S_ARGS
#undef S2S_CASE
    return AETHER_OK;
}

struct S2SDecLayout {
    size_t A[4], S[4], T1, M, agg_h, agg_p, ext, rel, relp, Rinv, ea, eap, epos, rp, ip, np_, hh, o1, o2, pred,
        p1p[4], irp, iip, inp, list[4], counts, total;
    int RF, RFp, EA, EAp, EP;
    S2SDecLayout(int D, int h, int64_t Nn, int64_t E) {
        const int O = D * (D - 1) / 2, NF = 4 * D + O;
        RF = 3 * D + NF; EA = NF + RF; EP = D + O;
        RFp = (RF + 15) / 16 * 16; EAp = (EA + 15) / 16 * 16;
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, hh_ = (size_t)h;
        for (auto& v : A) v = take(nn * hh_);
        for (auto& v : S) v = take(nn * hh_);
        T1 = take(ee * hh_); M = take(ee * hh_);
        agg_h = take(nn * hh_); agg_p = take(nn * hh_);
        ext = take(nn * 3 * D); rel = take(nn * RF); relp = take(nn * RFp); Rinv = take(nn * D * D);
        ea = take(ee * EA); eap = take(ee * EAp); epos = take(ee * EP);
        rp = take(nn * hh_); ip = take(nn * hh_); np_ = take(nn * hh_); hh = take(nn * hh_);
        o1 = take(nn * hh_); o2 = take(nn * hh_); pred = take(nn * 2 * D);
        for (auto& v : p1p) v = take(hh_ * EAp);
        irp = take(hh_ * RFp); iip = take(hh_ * RFp); inp = take(hh_ * RFp);
        for (auto& v : list) v = take(ee * 2);           // int64 edge ids of one type
        counts = take(64);
        total = off;
    }
};
}  // namespace

size_t aether_s2s_decoder_workspace_bytes(int num_dims, int hidden, int64_t n_nodes, int64_t n_edges) {
    if ((num_dims != 2 && num_dims != 3) || hidden <= 0 || n_nodes <= 0 || n_edges < 0) return 0;
    return S2SDecLayout(num_dims, hidden, n_nodes, n_edges).total;
}

int aether_s2s_decoder_step(const AetherS2SDecoderParams* p, int num_dims, int hidden, int num_edge_types,
                            int skip_first, int64_t n_nodes, int64_t n_edges, const float* inputs,
                            const float* hidden_in, const float* edge_w, const float* field, const int64_t* send,
                            const int64_t* recv, const int64_t* order, const int64_t* rowptr, void* workspace,
                            size_t workspace_bytes, float* outputs, float* hidden_out, void* stream) {
    if (!p || !inputs || !hidden_in || !field || !workspace || !outputs || !hidden_out || !rowptr)
        return fail(AETHER_EINVAL, "s2s_decoder: null pointer");
    if (n_edges > 0 && (!edge_w || !send || !recv || !order)) return fail(AETHER_EINVAL, "s2s_decoder: null edge pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "s2s_decoder: num_dims must be 2 or 3");
    if (hidden < 32 || hidden % 32 != 0) return fail(AETHER_EINVAL, "s2s_decoder: hidden must be a multiple of 32");
    if (num_edge_types < 1 || num_edge_types > 4) return fail(AETHER_EINVAL, "s2s_decoder: 1..4 edge types");
    if (n_nodes <= 0 || n_edges < 0) return fail(AETHER_EINVAL, "s2s_decoder: bad sizes");
    const int D = num_dims, h = hidden, K = num_edge_types, k0 = skip_first ? 1 : 0;
    S2SDecLayout L(D, h, n_nodes, n_edges);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "s2s_decoder: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int64_t Nn = n_nodes, E = n_edges;
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // ---- edges per type: with one-hot types every edge is evaluated for its own type only (the other
    // term of the reference's sum is multiplied by zero, aether.py:613,632)
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    auto elist = [&](int k) { return reinterpret_cast<int64_t*>(ws + L.list[k]); };
    if (E > 0) {
        HIP_OK(hipMemsetAsync(counts, 0, 64 * sizeof(int), st));
        for (int k = k0; k < K; ++k)
            k_s2s_select<<<blocks(E), dim3(256), 0, st>>>(edge_w, K, k, E, elist(k), counts + k);
    }
    // ---- messages from the hidden states (aether.py:596-617)
    if (E > 0) {
        HIP_OK(hipMemsetAsync(wp(L.M), 0, (size_t)E * h * 4, st));
        for (int k = k0; k < K; ++k) {
            if (s2s_linear(0, p->msg_fc1_w[k], 2 * h, p->msg_fc1_b[k], hidden_in, wp(L.A[k]), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
            if (s2s_linear(0, p->msg_fc1_w[k] + h, 2 * h, nullptr, hidden_in, wp(L.S[k]), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
            k_s2s_pair_tanh<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(wp(L.A[k]), wp(L.S[k]), send, recv, elist(k), counts + k, wp(L.T1), h);
            if (s2s_linear(3, p->msg_fc2_w[k], h, p->msg_fc2_b[k], wp(L.T1), wp(L.M), h, h, E, h, edge_w + k, K, 1, st,
                           nullptr, elist(k), counts + k)) return AETHER_EINVAL;
        }
    }
    k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.M), order, rowptr, wp(L.agg_h), h, 0.0f);
    // ---- local frames of [inputs | field] (:620-622) and the messages from the present state (:624-635)
    k_s2s_extend<<<blocks(Nn * 3 * D), dim3(256), 0, st>>>(inputs, field, wp(L.ext), D, Nn);
    int rc = aether_s2s_localize(D, Nn, E, wp(L.ext), send, recv, 1, wp(L.rel), wp(L.Rinv), wp(L.ea), wp(L.epos), stream);
    if (rc != AETHER_OK) return rc;
    k_s2s_pad_rows<<<blocks(Nn * L.RFp), dim3(256), 0, st>>>(wp(L.rel), L.RF, L.RF, wp(L.relp), L.RFp, Nn);
    k_s2s_pad_rows<<<blocks((int64_t)h * L.RFp), dim3(256), 0, st>>>(p->input_r_w, L.RF, L.RF, wp(L.irp), L.RFp, h);
    k_s2s_pad_rows<<<blocks((int64_t)h * L.RFp), dim3(256), 0, st>>>(p->input_i_w, L.RF, L.RF, wp(L.iip), L.RFp, h);
    k_s2s_pad_rows<<<blocks((int64_t)h * L.RFp), dim3(256), 0, st>>>(p->input_n_w, L.RF, L.RF, wp(L.inp), L.RFp, h);
    if (E > 0) {
        k_s2s_pad_rows<<<blocks(E * L.EAp), dim3(256), 0, st>>>(wp(L.ea), L.EA, L.EA, wp(L.eap), L.EAp, E);
        HIP_OK(hipMemsetAsync(wp(L.M), 0, (size_t)E * h * 4, st));
        for (int k = k0; k < K; ++k) {
            k_s2s_pad_rows<<<blocks((int64_t)h * L.EAp), dim3(256), 0, st>>>(p->pmsg_fc1_w[k], L.EA, L.EA, wp(L.p1p[k]), L.EAp, h);
            if (s2s_linear(2, wp(L.p1p[k]), L.EAp, p->pmsg_fc1_b[k], wp(L.eap), wp(L.T1), h, L.EAp, E, h, nullptr, 0, 0, st,
                           elist(k), nullptr, counts + k)) return AETHER_EINVAL;
            if (s2s_linear(2, p->pmsg_fc2_w[k], h, p->pmsg_fc2_b[k], wp(L.T1), wp(L.M), h, h, E, h, edge_w + k, K, 1, st,
                           nullptr, elist(k), counts + k)) return AETHER_EINVAL;
        }
    }
    k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.M), order, rowptr, wp(L.agg_p), h, 0.0f);
    // ---- GRU-style gate (:638-646)
    struct Gate { const float *iw, *ib, *pw, *pb, *hw; float* y; };
    const Gate gates[3] = {{wp(L.irp), p->input_r_b, p->present_r_w, p->present_r_b, p->hidden_r_w, wp(L.rp)},
                           {wp(L.iip), p->input_i_b, p->present_i_w, p->present_i_b, p->hidden_i_w, wp(L.ip)},
                           {wp(L.inp), p->input_n_b, p->present_n_w, p->present_n_b, nullptr, wp(L.np_)}};
    for (const Gate& g : gates) {
        if (s2s_linear(0, g.iw, L.RFp, g.ib, wp(L.relp), g.y, h, L.RFp, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
        if (s2s_linear(0, g.pw, h, g.pb, wp(L.agg_p), g.y, h, h, Nn, h, nullptr, 0, 1, st)) return AETHER_EINVAL;
        if (g.hw && s2s_linear(0, g.hw, h, nullptr, wp(L.agg_h), g.y, h, h, Nn, h, nullptr, 0, 1, st)) return AETHER_EINVAL;
    }
    if (s2s_linear(0, p->hidden_h_w, h, nullptr, wp(L.agg_h), wp(L.hh), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    k_s2s_gate<<<blocks(Nn * h), dim3(256), 0, st>>>(wp(L.rp), wp(L.ip), wp(L.np_), wp(L.hh), hidden_in, hidden_out, Nn * h);
    // ---- output MLP, globalise, residual (:649-654)
    if (s2s_linear(2, p->out0_w, h, p->out0_b, hidden_out, wp(L.o1), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(2, p->out3_w, h, p->out3_b, wp(L.o1), wp(L.o2), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->out6_w, h, p->out6_b, wp(L.o2), wp(L.pred), 2 * D, h, Nn, 2 * D, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (D == 2) k_s2s_globalize<2><<<blocks(Nn), dim3(256), 0, st>>>(inputs, wp(L.pred), wp(L.Rinv), outputs, Nn);
    else k_s2s_globalize<3><<<blocks(Nn), dim3(256), 0, st>>>(inputs, wp(L.pred), wp(L.Rinv), outputs, Nn);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

namespace {
struct S2SPriorLayout {
    size_t ext, rel, relp, Rinv, ea, epos, bimg, eaf, X0, X1, X3, Ps, Pr, T1, X4, G, Y1, Y2, bn, res1p, fpart, fimg, total;
    int RF, RFp, EA, EP, splits;
    // k-splits of the filter GEMM (k_s2s_filter_split: persistent workgroups, 32 per XCD, an XCD walks (c block, split) pairs
    // xcd, xcd + 8, .. with one 256-edge tile per workgroup): the split count that minimises rounds x k range per unit on the
    // busiest XCD; ties go to fewer planes
    static int filter_splits(int h, int64_t E) {
        if (g_filter_splits > 0 && (h / 64) % g_filter_splits == 0) return g_filter_splits;
        const int64_t eb = (E + 255) / 256;
        int best = 1;
        int64_t best_cost = INT64_MAX;
        for (int s = 1; s <= 8 && (h / 64) % s == 0; s *= 2) {
            const int64_t pairs_per_xcd = ((h / 64) * s + 7) / 8;              // the busiest XCD
            const int64_t cost = ((pairs_per_xcd * eb + 31) / 32) * (h / s + 8);    // + the fixed work of a unit
            if (cost < best_cost) { best_cost = cost; best = s; }
        }
        return best;
    }
    // Few edges (variable-N steps, 15 features): the features are divided over rs units as well (s2s_filter.h) until the
    // launch has ~a third of the CUs' worth of workgroups per filter; rs divides 15.
    static int filter_rsplits15(int h, int64_t E) {
        const int64_t units = ((E + 255) / 256) * (h / 64) * filter_splits(h, E);
        int rs = 1;
        for (int cand : {3, 5})
            if (units * cand <= 96) rs = cand;
        return rs;
    }
    S2SPriorLayout(int D, int h, int R, int ph, int64_t Nn, int64_t E, bool with_image = true) {
        const int O = D * (D - 1) / 2, NF = 4 * D + O;
        RF = 3 * D + NF; EA = NF + RF; EP = D + O;
        RFp = (RF + 15) / 16 * 16;
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, hh = (size_t)h;
        ext = take(nn * 3 * D); rel = take(nn * RF); relp = take(nn * RFp); Rinv = take(nn * D * D);
        ea = take(ee * EA); epos = take(ee * EP); bimg = take((filt_bimg_bytes(E, (int)hh) + 3) / 4); eaf = take(ee * hh);
        X0 = take(nn * hh); X1 = take(nn * hh); X3 = take(nn * hh); Ps = take(nn * hh); Pr = take(nn * hh);
        T1 = take(ee * hh); X4 = take(ee * hh); G = take(ee * 4 * (size_t)R);
        Y1 = take(ee * (size_t)(ph > 0 ? ph : 1)); Y2 = take(ee * (size_t)(ph > 0 ? ph : 1));
        bn = take(4 * hh); res1p = take(hh * RFp);
        splits = filter_splits(h, E);
        fpart = take(splits > 1 ? ee * hh * splits : 0);
        fimg = take(with_image ? (filt_image_bytes(EA, (int)hh) + 3) / 4 : 0);       // fp16 x 2 pieces of filt_w2, when the caller has none
        total = off;
    }
};
}  // namespace

size_t aether_s2s_filter_image_bytes(int n_features, int hidden) {
    if (n_features <= 0 || hidden < 128 || hidden % 128 != 0) return 0;
    return filt_image_bytes(n_features, hidden);
}

int aether_s2s_filter_prepare(const float* filt_w2, int n_features, int hidden, void* image, size_t image_bytes,
                              void* stream) {
    if (!filt_w2 || !image) return fail(AETHER_EINVAL, "s2s_filter_prepare: null pointer");
    if (n_features <= 0 || hidden < 128 || hidden % 128 != 0)
        return fail(AETHER_EINVAL, "s2s_filter_prepare: hidden must be a multiple of 128");
    if (image_bytes < aether_s2s_filter_image_bytes(n_features, hidden) || ((size_t)image & 15))
        return fail(AETHER_ESPACE, "s2s_filter_prepare: image buffer too small or not 16-byte aligned");
    filter_images_launch(filt_w2, n_features, hidden, image, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_prior_workspace_bytes(int num_dims, int hidden, int rnn_hidden, int prior_hidden,
                                        int64_t n_nodes, int64_t n_edges) {
    if ((num_dims != 2 && num_dims != 3) || hidden <= 0 || rnn_hidden <= 0 || n_nodes <= 0 || n_edges < 0) return 0;
    return S2SPriorLayout(num_dims, hidden, rnn_hidden, prior_hidden, n_nodes, n_edges).total;
}

namespace {
// Encoder.single_step_forward / Encoder.forward up to mlp4 (aether.py:385-398 / :354-369): per-edge features x4 [E][h]
int s2s_prior_features(const AetherS2SPriorParams* p, int D, int h, int polar, int num_vars, int64_t Nn, int64_t E,
                       const float* inputs, const float* field, const int64_t* send, const int64_t* recv,
                       const int64_t* order, const int64_t* rowptr, const S2SPriorLayout& L, char* ws, float* x4,
                       void* stream) {
    hipStream_t st = (hipStream_t)stream;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // ---- local frames (:385-388) and the anisotropic edge filter (:391)
    k_s2s_extend<<<blocks(Nn * 3 * D), dim3(256), 0, st>>>(inputs, field, wp(L.ext), D, Nn);
    int rc = aether_s2s_localize(D, Nn, E, wp(L.ext), send, recv, polar, wp(L.rel), wp(L.Rinv), wp(L.ea), wp(L.epos), stream);
    if (rc != AETHER_OK) return rc;
    {
        const f16x8* image = reinterpret_cast<const f16x8*>(p->filt_image);
        if (!image) {                                          // no prepared image: build it here (41 | 25 MB read per call)
            f16x8* mine = reinterpret_cast<f16x8*>(ws + L.fimg);
            filter_images_launch(p->filt_w2, L.EA, h, mine, st);
            image = mine;
        }
        f16x8* bimg = reinterpret_cast<f16x8*>(ws + L.bimg);
        if (D == 2) k_s2s_filter_bimg<3><<<filter_bimg_grid(E), dim3(256), 0, st>>>(wp(L.epos), p->filt_w0, p->filt_b0, 0, h, E, bimg);
        else k_s2s_filter_bimg<6><<<filter_bimg_grid(E), dim3(256), 0, st>>>(wp(L.epos), p->filt_w0, p->filt_b0, 0, h, E, bimg);
        const int64_t units = ((E + 255) / 256) * (h / 64) * L.splits;
        const dim3 grid((unsigned)(units < FILTER_WGS ? units : FILTER_WGS));
        float* dst = L.splits > 1 ? wp(L.fpart) : wp(L.eaf);
        s2s_stats_filter(L.splits);
#define FILT_LAUNCH(RR)                                                                                                  \
    do {                                                                                                                 \
        const size_t lds = filt_lds_bytes(RR);                                                                           \
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_s2s_filter_split<RR>), lds)) return AETHER_EHIP;          \
        k_s2s_filter_split<RR><<<grid, dim3(512), lds, st>>>(image, p->filt_b2, wp(L.ea), bimg, dst, h, E, L.splits, 1, (int)grid.x);    \
    } while (0)
        if (D == 2) FILT_LAUNCH(24); else FILT_LAUNCH(39);
#undef FILT_LAUNCH
        if (L.splits > 1) k_s2s_sum_planes<<<blocks(E * h / 4), dim3(256), 0, st>>>(dst, L.splits, E * (int64_t)h, wp(L.eaf));
    }
    // ---- x = edge2node(edge_attr) + res1(rel_feat) (:393-395): sum over in-edges / (num_vars - 1)
    k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.eaf), order, rowptr, wp(L.X0), h, (float)(num_vars - 1));
    k_s2s_pad_rows<<<blocks(Nn * L.RFp), dim3(256), 0, st>>>(wp(L.rel), L.RF, L.RF, wp(L.relp), L.RFp, Nn);
    k_s2s_pad_rows<<<blocks((int64_t)h * L.RFp), dim3(256), 0, st>>>(p->res1_w, L.RF, L.RF, wp(L.res1p), L.RFp, h);
    if (s2s_linear(0, wp(L.res1p), L.RFp, p->res1_b, wp(L.relp), wp(L.X0), h, L.RFp, Nn, h, nullptr, 0, 1, st)) return AETHER_EINVAL;
    // ---- mlp3 (RefNRIMLP, eval): Linear-ELU-Linear-ELU-BatchNorm
    float *bn3s = wp(L.bn), *bn3b = wp(L.bn) + h, *bn4s = wp(L.bn) + 2 * h, *bn4b = wp(L.bn) + 3 * h;
    k_s2s_bn_affine<<<blocks(h), dim3(256), 0, st>>>(p->mlp3_bn_w, p->mlp3_bn_b, p->mlp3_bn_mean, p->mlp3_bn_var, bn3s, bn3b, h);
    k_s2s_bn_affine<<<blocks(h), dim3(256), 0, st>>>(p->mlp4_bn_w, p->mlp4_bn_b, p->mlp4_bn_mean, p->mlp4_bn_var, bn4s, bn4b, h);
    if (s2s_linear(4, p->mlp3_w0, h, p->mlp3_b0, wp(L.X0), wp(L.X1), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(4, p->mlp3_w3, h, p->mlp3_b3, wp(L.X1), wp(L.X3), h, h, Nn, h, nullptr, 0, 0, st, nullptr, nullptr, nullptr, bn3s, bn3b)) return AETHER_EINVAL;
    // ---- mlp4 on [x_send | x_recv | edge] (:396-398): the first Linear split per node / per edge
    if (s2s_linear(0, p->mlp4_w0, 3 * h, p->mlp4_b0, wp(L.X3), wp(L.Ps), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->mlp4_w0 + h, 3 * h, nullptr, wp(L.X3), wp(L.Pr), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->mlp4_w0 + 2 * h, 3 * h, nullptr, wp(L.eaf), wp(L.T1), h, h, E, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    k_s2s_edge_sum_elu<<<blocks(E * (h / 4)), dim3(256), 0, st>>>(wp(L.T1), wp(L.Ps), wp(L.Pr), send, recv, h, E);
    if (s2s_linear(4, p->mlp4_w3, h, p->mlp4_b3, wp(L.T1), x4, h, h, E, h, nullptr, 0, 0, st, nullptr, nullptr, nullptr, bn4s, bn4b)) return AETHER_EINVAL;
    return AETHER_OK;
}

int s2s_prior_check(const AetherS2SPriorParams* p, int num_dims, int hidden, int num_vars, int64_t n_nodes, int64_t n_edges) {
    if (!p) return fail(AETHER_EINVAL, "s2s_prior: null pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "s2s_prior: num_dims must be 2 or 3");
    if (hidden < 128 || hidden % 128 != 0) return fail(AETHER_EINVAL, "s2s_prior: hidden must be a multiple of 128");
    if (num_vars < 2 || n_nodes <= 0 || n_edges <= 0) return fail(AETHER_EINVAL, "s2s_prior: bad sizes");
    return AETHER_OK;
}
}  // namespace

int aether_s2s_encoder_features(const AetherS2SPriorParams* p, int num_dims, int hidden, int polar, int num_vars,
                                int64_t n_nodes, int64_t n_edges, const float* inputs, const float* field,
                                const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                                void* workspace, size_t workspace_bytes, float* features, void* stream) {
    if (!inputs || !field || !send || !recv || !order || !rowptr || !workspace || !features)
        return fail(AETHER_EINVAL, "s2s_encoder_features: null pointer");
    if (int rc = s2s_prior_check(p, num_dims, hidden, num_vars, n_nodes, n_edges)) return rc;
    S2SPriorLayout L(num_dims, hidden, 16, 0, n_nodes, n_edges);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "s2s_encoder_features: workspace too small");
    int rc = s2s_prior_features(p, num_dims, hidden, polar, num_vars, n_nodes, n_edges, inputs, field, send, recv, order, rowptr,
                                L, (char*)workspace, features, stream);
    if (rc != AETHER_OK) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_lstm_step(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int in_size,
                         int rnn_hidden, int64_t n_rows, const float* x, const float* h0, const float* c0, float* gates,
                         float* h1, float* c1, void* stream) {
    if (!w_ih || !w_hh || !b_ih || !b_hh || !x || !h0 || !c0 || !gates || !h1 || !c1)
        return fail(AETHER_EINVAL, "s2s_lstm_step: null pointer");
    if (in_size < 16 || in_size % 16 != 0 || rnn_hidden < 16 || rnn_hidden % 16 != 0 || n_rows <= 0)
        return fail(AETHER_EINVAL, "s2s_lstm_step: sizes must be multiples of 16");
    if (int rc = nri_lstm_two_launch(w_ih, w_hh, b_ih, b_hh, in_size, rnn_hidden, n_rows, x, h0, c0, gates, h1, c1,
                                     (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_mlp_head(const float* const* w, const float* const* b, int layers, int in_size, int hidden_size,
                        int out_size, int64_t n_rows, const float* x, float* scratch, float* out, void* stream) {
    if (!w || !b || !x || !out || (layers > 1 && !scratch)) return fail(AETHER_EINVAL, "s2s_mlp_head: null pointer");
    if (layers < 1 || layers > 4 || in_size % 16 != 0 || (layers > 1 && hidden_size % 16 != 0) || out_size < 1 || n_rows <= 0)
        return fail(AETHER_EINVAL, "s2s_mlp_head: 1..4 layers, input / hidden sizes multiples of 16");
    for (int l = 0; l < layers; ++l)
        if (!w[l] || !b[l]) return fail(AETHER_EINVAL, "s2s_mlp_head: null layer pointer");
    float* second = layers > 2 ? scratch + (size_t)n_rows * hidden_size : nullptr;     // (three layers and more ping-pong)
    if (int rc = nri_head_linear(w, b, layers, in_size, hidden_size, out_size, n_rows, x, scratch, second, out,
                                 (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_prior_step(const AetherS2SPriorParams* p, int num_dims, int hidden, int rnn_hidden, int prior_layers,
                          int prior_hidden, int num_edge_types, int polar, int num_vars, int64_t n_nodes,
                          int64_t n_edges, const float* inputs, const float* field, const float* h0, const float* c0,
                          const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                          void* workspace, size_t workspace_bytes, float* logits, float* h1, float* c1, void* stream) {
    if (!p || !inputs || !field || !h0 || !c0 || !send || !recv || !order || !rowptr || !workspace || !logits || !h1 || !c1)
        return fail(AETHER_EINVAL, "s2s_prior: null pointer");
    if (int rc = s2s_prior_check(p, num_dims, hidden, num_vars, n_nodes, n_edges)) return rc;
    if (rnn_hidden < 16 || rnn_hidden % 16 != 0) return fail(AETHER_EINVAL, "s2s_prior: rnn_hidden must be a multiple of 16");
    if (prior_layers < 1 || prior_layers > 4) return fail(AETHER_EINVAL, "s2s_prior: 1..4 prior layers");
    if (prior_layers > 1 && (prior_hidden < 16 || prior_hidden % 16 != 0))
        return fail(AETHER_EINVAL, "s2s_prior: prior_hidden must be a multiple of 16");
    if (num_edge_types < 1 || num_edge_types > 4) return fail(AETHER_EINVAL, "s2s_prior: bad sizes");
    const int D = num_dims, h = hidden, R = rnn_hidden, K = num_edge_types;
    S2SPriorLayout L(D, h, R, prior_hidden, n_nodes, n_edges);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "s2s_prior: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int64_t E = n_edges;
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    if (int rc = s2s_prior_features(p, D, h, polar, num_vars, n_nodes, n_edges, inputs, field, send, recv, order, rowptr, L, ws,
                                    wp(L.X4), stream)) return rc;
    // ---- one LSTM step per edge (:400-407), prior_fc_out (:408)
    if (int rc = nri_lstm_two_launch(p->lstm_w_ih, p->lstm_w_hh, p->lstm_b_ih, p->lstm_b_hh, h, R, E, wp(L.X4), h0, c0, wp(L.G), h1,
                                     c1, st)) return rc;
    if (int rc = nri_head_linear(p->prior_w, p->prior_b, prior_layers, R, prior_hidden, K, E, h1, wp(L.Y1), wp(L.Y2), logits, st))
        return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// ------------------------------------------------------------------ seq2seq dynamic-field variant (N3)
namespace {
struct S2SSummaryLayout {
    size_t xp, wep, emb, gi, gh, h, aug, g0p, n0p, gate, total;
    int inp, Kp;
    S2SSummaryLayout(int64_t B, int N, int T, int in, int H) {
        inp = (in + 15) / 16 * 16; Kp = (in + H + 15) / 16 * 16;
        const size_t S = (size_t)B * N, R = S * T, hh = (size_t)H;
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        xp = take(R * inp); wep = take(hh * inp); emb = take(R * hh);
        gi = take(R * 3 * hh);                  // after the GRU: T1 | T2 | V of the attention nets
        gh = take(S * 3 * hh); h = take(S * hh);
        aug = take(R * Kp); g0p = take(hh * Kp); n0p = take(hh * Kp); gate = take(R);
        total = off;
    }
};
}  // namespace

size_t aether_s2s_graph_summary_workspace_bytes(int64_t batch, int num_objects, int timesteps, int input_size,
                                                int hidden) {
    if (batch <= 0 || num_objects <= 0 || timesteps <= 0 || input_size <= 0 || hidden <= 0) return 0;
    return S2SSummaryLayout(batch, num_objects, timesteps, input_size, hidden).total + 256;
}

int aether_s2s_graph_summary(const AetherS2SGraphSummaryParams* p, int64_t batch, int num_objects, int timesteps,
                             int input_size, int hidden, int pe_len, const float* x, void* workspace,
                             size_t workspace_bytes, float* summary, void* stream) {
    if (!p || !x || !workspace || !summary || !p->emb_w || !p->emb_b || !p->gru_w_ih || !p->gru_w_hh || !p->gru_b_ih ||
        !p->gru_b_hh || !p->pe || !p->gate_w0 || !p->gate_b0 || !p->gate_w2 || !p->gate_b2 || !p->nn_w0 || !p->nn_b0 ||
        !p->nn_w2 || !p->nn_b2)
        return fail(AETHER_EINVAL, "s2s_graph_summary: null pointer");
    if (batch <= 0 || num_objects <= 0 || timesteps <= 0 || input_size <= 0)
        return fail(AETHER_EINVAL, "s2s_graph_summary: bad sizes");
    if (hidden < 16 || hidden % 16 != 0) return fail(AETHER_EINVAL, "s2s_graph_summary: hidden must be a multiple of 16");
    if (timesteps > pe_len)
        return fail(AETHER_EINVAL, "s2s_graph_summary: more time steps than rows of the positional encoding");
    const S2SSummaryLayout L(batch, num_objects, timesteps, input_size, hidden);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "s2s_graph_summary: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    auto wp = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
    const int in = input_size, H = hidden, T = timesteps;
    const int64_t S = batch * num_objects, R = S * T;
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // particle embedding and the input half of the GRU for every time step at once (graph_pool.py:62-63)
    k_s2s_pad_rows<<<blocks(R * L.inp), dim3(256), 0, st>>>(x, in, in, wp(L.xp), L.inp, R);
    k_s2s_pad_rows<<<blocks((int64_t)H * L.inp), dim3(256), 0, st>>>(p->emb_w, in, in, wp(L.wep), L.inp, H);
    if (s2s_linear(0, wp(L.wep), L.inp, p->emb_b, wp(L.xp), wp(L.emb), H, L.inp, R, H, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->gru_w_ih, H, p->gru_b_ih, wp(L.emb), wp(L.gi), 3 * H, H, R, 3 * H, nullptr, 0, 0, st)) return AETHER_EINVAL;
    HIP_OK(hipMemsetAsync(wp(L.h), 0, (size_t)S * H * sizeof(float), st));
    for (int t = 0; t < T; ++t) {
        if (s2s_linear(0, p->gru_w_hh, H, p->gru_b_hh, wp(L.h), wp(L.gh), 3 * H, H, S, 3 * H, nullptr, 0, 0, st)) return AETHER_EINVAL;
        k_s2s_gru_gate<<<blocks(S * H), dim3(256), 0, st>>>(wp(L.gi) + (size_t)t * 3 * H, (int64_t)T * 3 * H, wp(L.gh),
                                                            wp(L.h), H, S);
    }
    // [x | last hidden] + pe, then the two nets of the attention pooling (:66-70)
    k_s2s_augment<<<blocks(R * L.Kp), dim3(256), 0, st>>>(x, wp(L.h), p->pe, wp(L.aug), in, H, L.Kp, T, R);
    k_s2s_pad_rows<<<blocks((int64_t)H * L.Kp), dim3(256), 0, st>>>(p->gate_w0, in + H, in + H, wp(L.g0p), L.Kp, H);
    k_s2s_pad_rows<<<blocks((int64_t)H * L.Kp), dim3(256), 0, st>>>(p->nn_w0, in + H, in + H, wp(L.n0p), L.Kp, H);
    float* T1 = wp(L.gi);
    float* T2 = T1 + (size_t)R * H;
    float* V = T2 + (size_t)R * H;
    if (s2s_linear(1, wp(L.g0p), L.Kp, p->gate_b0, wp(L.aug), T1, H, L.Kp, R, H, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->gate_w2, H, p->gate_b2, T1, wp(L.gate), 1, H, R, 1, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(1, wp(L.n0p), L.Kp, p->nn_b0, wp(L.aug), T2, H, L.Kp, R, H, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, p->nn_w2, H, p->nn_b2, T2, V, H, H, R, H, nullptr, 0, 0, st)) return AETHER_EINVAL;
    k_s2s_attn_pool<<<dim3((unsigned)batch, (unsigned)((H + 255) / 256)), dim3(256), 0, st>>>(
        wp(L.gate), V, summary, num_objects * T, H);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_film_modulation_bytes(int64_t batch, int mlp_hidden) {
    if (batch <= 0 || mlp_hidden <= 0) return 0;
    return (size_t)5 * (size_t)batch * (size_t)mlp_hidden * sizeof(float);
}

int aether_s2s_film_modulation(const AetherS2SFilmParams* p, int graph_hidden, int mlp_hidden, int64_t batch,
                               const float* summary, float* mod, size_t mod_bytes, void* stream) {
    if (!p || !summary || !mod) return fail(AETHER_EINVAL, "s2s_film_modulation: null pointer");
    for (int k = 0; k < 4; ++k)
        if (!p->mod_w0[k] || !p->mod_b0[k] || !p->mod_w2[k] || !p->mod_b2[k])
            return fail(AETHER_EINVAL, "s2s_film_modulation: null pointer");
    if (batch <= 0 || graph_hidden < 16 || graph_hidden % 16 != 0 || mlp_hidden < 16 || mlp_hidden % 16 != 0)
        return fail(AETHER_EINVAL, "s2s_film_modulation: graph_hidden and mlp_hidden must be multiples of 16");
    if (mod_bytes < aether_s2s_film_modulation_bytes(batch, mlp_hidden))
        return fail(AETHER_ESPACE, "s2s_film_modulation: mod buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = (size_t)batch * mlp_hidden;
    float* tmp = mod + 4 * plane;
    for (int k = 0; k < 4; ++k) {
        if (s2s_linear(1, p->mod_w0[k], graph_hidden, p->mod_b0[k], summary, tmp, mlp_hidden, graph_hidden, batch,
                       mlp_hidden, nullptr, 0, 0, st)) return AETHER_EINVAL;
        if (s2s_linear(0, p->mod_w2[k], mlp_hidden, p->mod_b2[k], tmp, mod + k * plane, mlp_hidden, mlp_hidden, batch,
                       mlp_hidden, nullptr, 0, 0, st)) return AETHER_EINVAL;
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_film_field_workspace_bytes(int64_t n_points, int hidden, int mlp_hidden) {
    if (n_points <= 0 || hidden <= 0 || mlp_hidden <= 0) return 0;
    return align_up((size_t)n_points * hidden * 4, 256) + 2 * align_up((size_t)n_points * mlp_hidden * 4, 256) + 256;
}

int aether_s2s_film_field(const AetherS2SFilmParams* p, int num_dims, int hidden, int mlp_hidden, int64_t n_points,
                          int64_t rows_per_graph, const float* x, int x_stride, const float* mod, int64_t batch,
                          void* workspace, size_t workspace_bytes, float* field, void* stream) {
    if (!p || !x || !mod || !workspace || !field || !p->B || !p->lin1_w || !p->lin1_b || !p->lin2_w || !p->lin2_b ||
        !p->lin3_w || !p->lin3_b)
        return fail(AETHER_EINVAL, "s2s_film_field: null pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "s2s_film_field: num_dims must be 2 or 3");
    if (hidden < 32 || hidden % 32 != 0) return fail(AETHER_EINVAL, "s2s_film_field: hidden must be a multiple of 32");
    if (mlp_hidden < 16 || mlp_hidden % 16 != 0) return fail(AETHER_EINVAL, "s2s_film_field: mlp_hidden must be a multiple of 16");
    if (n_points <= 0 || x_stride < num_dims || rows_per_graph <= 0 || batch <= 0 ||
        (n_points + rows_per_graph - 1) / rows_per_graph > batch || rows_per_graph > INT32_MAX)
        return fail(AETHER_EINVAL, "s2s_film_field: bad sizes (n_points must fit batch * rows_per_graph)");
    if (workspace_bytes < aether_s2s_film_field_workspace_bytes(n_points, hidden, mlp_hidden))
        return fail(AETHER_ESPACE, "s2s_film_field: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    const size_t gplane = align_up((size_t)n_points * hidden * 4, 256), hplane = align_up((size_t)n_points * mlp_hidden * 4, 256);
    float* gamma = reinterpret_cast<float*>(ws);
    float* h1 = reinterpret_cast<float*>(ws + gplane);
    float* h2 = reinterpret_cast<float*>(ws + gplane + hplane);
    const size_t plane = (size_t)batch * mlp_hidden;
    const int half = hidden / 2, rows = (int)rows_per_graph;
    const unsigned rb = (unsigned)((n_points * half + 255) / 256);
    if (num_dims == 2) k_s2s_rff<2><<<dim3(rb), dim3(256), 0, st>>>(x, x_stride, p->B, half, gamma, n_points);
    else k_s2s_rff<3><<<dim3(rb), dim3(256), 0, st>>>(x, x_stride, p->B, half, gamma, n_points);
    if (s2s_linear(1, p->lin1_w, hidden, p->lin1_b, gamma, h1, mlp_hidden, hidden, n_points, mlp_hidden, nullptr, 0, 0, st,
                   nullptr, nullptr, nullptr, nullptr, nullptr, mod, mod + plane, rows)) return AETHER_EINVAL;
    if (s2s_linear(1, p->lin2_w, mlp_hidden, p->lin2_b, h1, h2, mlp_hidden, mlp_hidden, n_points, mlp_hidden, nullptr, 0, 0, st,
                   nullptr, nullptr, nullptr, nullptr, nullptr, mod + 2 * plane, mod + 3 * plane, rows)) return AETHER_EINVAL;
    if (s2s_linear(0, p->lin3_w, mlp_hidden, p->lin3_b, h2, field, num_dims, mlp_hidden, n_points, num_dims, nullptr, 0, 0, st))
        return AETHER_EINVAL;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_gumbel_hard(const float* logits, const float* uniform, float tau, int num_edge_types, int64_t n_edges,
                           float* edges, void* stream) {
    if (!logits || !uniform || !edges) return fail(AETHER_EINVAL, "s2s_gumbel: null pointer");
    if (num_edge_types < 1 || num_edge_types > 4 || n_edges <= 0 || !(tau > 0.0f)) return fail(AETHER_EINVAL, "s2s_gumbel: bad sizes");
    k_s2s_gumbel_hard<<<dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        logits, uniform, tau, num_edge_types, edges, n_edges);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

