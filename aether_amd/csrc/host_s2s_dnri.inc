// Host side of the C ABI: the seq2seq dNRI baseline (nn/seq2seq/dnri.py) on the job-table engine of host_s2s_step.inc -- plan,
// step (also as the decoder on given logits), device rollout and the encoder's per-time-step features, one set of entries for
// both decoders: exactly one of dp (DNRI_Decoder) and mp (DNRI_MLP_Decoder) is given.  The model has no frames: no localizer,
// edge-attribute, filter or globalise launch is made and no buffer is sized for one (s2s_dnri.h).  Included by aether_hip.hip
// inside its extern "C" block after host_s2s_locs.inc; not a stand-alone source file.

namespace {

struct DnriSizes {
    int D, he, hd, R, prior_layers, ph, K, skip_first, num_vars;
    float tau;
    int64_t Nn, E;
};

// Prepared weights (device).  ku >= 1: the MLP decoder with that many used edge types; -1: the recurrent decoder.
struct DnriPlanLayout {
    size_t bn, lb, lbp, o1p, total;
    size_t i_w3[4], i_m2s, i_m2r, i_m3_0, i_ps, i_pr, i_m4e, i_ih, i_hh, i_prior[4];                  // fp16 x 2 images (0: none)
    size_t i_a[4], i_s[4], i_msg2[4], i_hr, i_hi, i_hh2, i_out1, i_out2;
    int ldo1;                                   // row stride of the padded out_fc1: S2S_RFG + hd
    DnriPlanLayout(int he, int hd, int K, int R, int prior_layers, int ph, int ku) {
        const bool rec = ku < 0;
        ldo1 = S2S_RFG + hd;
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
        auto image = [&](int M, int Kk) { return S2SPlanLayout::splittable(M, Kk) ? take((size_t)M * Kk * 4) : (size_t)0; };
        bn = take((size_t)8 * he * 4);                       // scale | shift of mlp1 .. mlp4
        lb = take((size_t)4 * R * 4);
        lbp = take((size_t)4 * R * 4);                       // gates interleaved by unit (the fused LSTM cell of the split GEMM)
        o1p = take(rec ? 0 : (size_t)hd * ldo1 * 4);
        for (int l = 0; l < 4; ++l) i_w3[l] = image(he, he);
        i_m2s = image(he, he); i_m2r = image(he, he); i_m3_0 = image(he, he); i_ps = image(he, he); i_pr = image(he, he);
        i_m4e = image(he, he); i_ih = image(4 * R, he); i_hh = image(4 * R, R);
        for (int l = 0; l < 4; ++l) i_prior[l] = l + 1 < prior_layers ? image(ph, l == 0 ? R : ph) : 0;
        for (int k = 0; k < 4; ++k) {
            i_a[k] = rec && k < K ? image(hd, hd) : 0; i_s[k] = rec && k < K ? image(hd, hd) : 0;
            i_msg2[k] = k < K ? image(hd, hd) : 0;
        }
        if (rec) { i_hr = image(hd, hd); i_hi = image(hd, hd); i_hh2 = image(hd, hd); i_out1 = image(hd, hd); }
        else { i_hr = i_hi = i_hh2 = 0; i_out1 = image(hd, ldo1); }
        i_out2 = image(hd, hd);
        total = off;
    }
};

// The workspace of a step / rollout: node rows of the prior, its edge rows, the sample, the decoder's rows and the ping-pong
// state of the rollout.  Nothing of a frame: no rel_feat, Rinv, edge_attr, edge_pos, filter image / planes, present messages.
struct DnriStepLayout {
    size_t X1a, X1, PsPr, T2, X2, X2n, X3a, X3, T4, X4, G, Y1, Y2, logits, edges, lists, counts, A, S, Tm, M, agg, hr, hi, hh, o1,
        o2, xa, da, db, ha, hb, ca, cb, total;
    int ldagg;
    DnriStepLayout(int D, int he, int hd, int R, int ph, int K, int64_t Nn, int64_t E) {
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, h = (size_t)he, g = (size_t)hd;
        ldagg = S2S_RFG + hd;
        X1a = take(nn * h); X1 = take(nn * h); PsPr = take(2 * nn * h); T2 = take(ee * h); X2 = take(ee * h); X2n = take(nn * h);
        X3a = take(nn * h); X3 = take(nn * h); T4 = take(ee * h); X4 = take(ee * h); G = take(ee * 4 * (size_t)R);
        Y1 = take(ee * (size_t)(ph > 0 ? ph : 1)); Y2 = take(ee * (size_t)(ph > 0 ? ph : 1));
        logits = take(ee * K); edges = take(ee * K); lists = take(ee * K * 2); counts = take(64);
        A = take((size_t)K * nn * g); S = take((size_t)K * nn * g); Tm = take((size_t)K * ee * g); M = take(ee * g);
        agg = take(nn * (size_t)ldagg);                      // [inputs, 0 .. | agg] (MLP decoder); the recurrent one uses hd columns
        hr = take(nn * g); hi = take(nn * g); hh = take(nn * g); o1 = take(nn * g); o2 = take(nn * g);
        xa = take(nn * 2 * D); da = take(nn * g); db = take(nn * g);
        ha = take(ee * (size_t)R); hb = take(ee * (size_t)R); ca = take(ee * (size_t)R); cb = take(ee * (size_t)R);
        total = off;
    }
};

// The field of the ablation DNRIAether (host_s2s_dnri_aether.inc): its parameters, the images of field_net.0 / .2 in the plan
// and the field query's rows in the workspace (byte offsets behind DnriPlanLayout / DnriStepLayout)
struct DnriFieldArgs {
    const AetherS2SFieldParams* fp;
    size_t i_f0, i_f2, gamma, fh1, fh2, field, ext;
};

struct DnriArgs : DnriSizes {
    const AetherS2SDnriPriorParams* pp; const AetherS2SDnriDecoderParams* dp; const AetherS2SDnriMlpParams* mp;
    const char* plan;
    const int64_t *send, *recv, *order, *rowptr;
    DnriPlanLayout P;
    DnriStepLayout L;
    const float* ext_logits = nullptr;          // the decoder on given logits: the prior is skipped
    float* features_out = nullptr;              // the prior stops behind mlp4 and leaves its rows there
    // DNRIAether (null: dNRI): every layer on the raw state reads ext = [inputs | field] (3D columns) instead.  ext_field
    // [Nn][D] (or null: the step queries the field) and field_out (or null) are those of the step at hand
    const DnriFieldArgs* fld = nullptr;
    const float* ext_field = nullptr;
    float* field_out = nullptr;
};

// The node side of a DNRIAether step (host_s2s_dnri_aether.inc): field query, ext, edge counters, the MLP decoder's node rows
int s2s_dnria_node_side(const DnriArgs& a, char* ws, const float* x_in, const AetherS2SDnriMlpParams* mp, hipStream_t st);

// Used edge types of the MLP decoder (-1: the recurrent decoder; 0: no decoder, both, or no used type)
int s2s_dnri_ku(const void* dp, const void* mp, int K, int skip_first) {
    if ((dp != nullptr) == (mp != nullptr)) return 0;
    if (K - (skip_first ? 1 : 0) < 1) return 0;
    return dp ? -1 : K - (skip_first ? 1 : 0);
}

bool s2s_dnri_sizes_ok(int D, int he, int hd, int R, int prior_layers, int ph, int K) {
    return (D == 2 || D == 3) && he >= 128 && he % 128 == 0 && hd >= 32 && hd % 32 == 0 && R >= 16 && R % 16 == 0 && K >= 1 &&
           K <= 4 && prior_layers >= 1 && prior_layers <= 4 && (prior_layers == 1 || (ph >= 16 && ph % 16 == 0));
}

// The checks every step / rollout / features entry makes before anything is queued, but the workspace's size
int s2s_dnri_entry_check(const char* what, const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp,
                         const AetherS2SDnriMlpParams* mp, const void* plan, const DnriSizes& z, bool pointers, int burn_in_steps,
                         int steps) {
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    if (!pp || !plan) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if (!s2s_dnri_sizes_ok(z.D, z.he, z.hd, z.R, z.prior_layers, z.ph, z.K))
        return s2s_fail(AETHER_EINVAL, what, "num_dims 2 | 3, encoder_hidden % 128, decoder_hidden % 32, rnn / prior hidden % 16");
    if (z.K - (z.skip_first ? 1 : 0) < 1) return s2s_fail(AETHER_EINVAL, what, "no used edge type");
    if (z.num_vars < 2 || z.Nn <= 0 || z.E <= 0) return s2s_fail(AETHER_EINVAL, what, "bad sizes");
    if (!pointers) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if (burn_in_steps < 0 || steps < 0 || burn_in_steps + steps == 0) return s2s_fail(AETHER_EINVAL, what, "no steps");
    if (!(z.tau > 0.0f)) return s2s_fail(AETHER_EINVAL, what, "tau must be positive");
    return AETHER_OK;
}

// (after s2s_dnri_entry_check: the layouts take the sizes as valid)
extern "C++" DnriArgs s2s_dnri_args(const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp,
                                    const AetherS2SDnriMlpParams* mp, const void* plan, const DnriSizes& z, const int64_t* send,
                                    const int64_t* recv, const int64_t* order, const int64_t* rowptr) {
    return DnriArgs{z, pp, dp, mp, (const char*)plan, send, recv, order, rowptr,
                    DnriPlanLayout(z.he, z.hd, z.K, z.R, z.prior_layers, z.ph, s2s_dnri_ku(dp, mp, z.K, z.skip_first)),
                    DnriStepLayout(z.D, z.he, z.hd, z.R, z.ph, z.K, z.Nn, z.E)};
}

// The prior step (dnri.py:403-424) and the hard Gumbel sample (:62-67) up to the per-type edge lists.  x_in [Nn][2D], h0 / c0
// [E][R], uniform [E][K] -> h1, c1 and, when `edges` is not null, the sample [E][K] with its lists / counts in the workspace.
// first_jobs(T): the recurrent decoder's first-layer products of its state, which share the launch of mlp1's second layer.
extern "C++" template <class FirstJobs>
int s2s_dnri_front(const DnriArgs& a, char* ws, const float* x_in, const float* h0, const float* c0, const float* uniform,
                   float* h1, float* c1, float* edges, FirstJobs&& first_jobs, hipStream_t st) {
    const int D = a.D, he = a.he, K = a.K, k0 = a.skip_first ? 1 : 0;
    const int64_t Nn = a.Nn, E = a.E;
    const DnriPlanLayout& P = a.P;
    const DnriStepLayout& L = a.L;
    const NriMem m{ws, a.plan};
    const AetherS2SDnriPriorParams* p = a.pp;
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int64_t* lists = reinterpret_cast<int64_t*>(ws + L.lists);
    // the step's edge counters; for the MLP decoder (when the step decodes) the raw state where out_fc1 reads it and the node
    // products of its first message layer
    if (a.fld) {
        if (int rc = s2s_dnria_node_side(a, ws, x_in, edges != nullptr ? a.mp : nullptr, st)) return rc;
    } else {
        const AetherS2SDnriMlpParams* mp = edges != nullptr ? a.mp : nullptr;
        const int per = a.hd / 4 > S2S_RFG ? a.hd / 4 : S2S_RFG;
        const float* none = nullptr;
        k_s2s_dnri_node_prep<<<mp ? nri_blocks(Nn * per) : dim3(1), dim3(256), 0, st>>>(
            x_in, 2 * D, mp ? m.wp(L.agg) : nullptr, L.ldagg, counts, Nn, mp ? mp->msg_fc1_w[0] : none, mp ? mp->msg_fc1_w[1] : none,
            mp ? mp->msg_fc1_w[2] : none, mp ? mp->msg_fc1_w[3] : none, mp ? mp->msg_fc1_b[0] : none, mp ? mp->msg_fc1_b[1] : none,
            mp ? mp->msg_fc1_b[2] : none, mp ? mp->msg_fc1_b[3] : none, K, k0, m.wp(L.A), m.wp(L.S), a.hd, per);
    }
    if (a.ext_logits == nullptr) {
        // mlp1 on the raw state (:405): its first Linear has 2D columns -- a narrow layer (DNRIAether: 3D columns of ext)
        if (a.fld)
            k_s2s_dnria_narrow_elu<<<nri_blocks(Nn * (he / 4)), dim3(256), 0, st>>>(p->mlp_w0[0], p->mlp_b0[0], m.wp(a.fld->ext), 3 * D,
                                                                                    m.wp(L.X1a), he, Nn);
        else
        { NarrowLayers N1{};
          N1.W[0] = p->mlp_w0[0]; N1.b[0] = p->mlp_b0[0]; N1.Y[0] = m.wp(L.X1a); N1.n = 1;
          k_s2s_narrow_layers<<<nri_blocks(Nn * (he / 4)), dim3(256), 0, st>>>(N1, x_in, 2 * D, 2 * D, he, 4, Nn); }
        // mlp1's second layer .. mlp4 (:405-413): in-edge sum / (num_vars - 1) between mlp2 and mlp3 (:344-351)
        const float* bn = m.pl(P.bn);                          // scale | shift of mlp1 .. mlp4
        float* Ps = m.wp(L.PsPr);
        float* x4 = a.features_out ? a.features_out : m.wp(L.X4);
        const NriDnriPrior c{{bn, bn + 2 * he, bn + 4 * he, bn + 6 * he}, {bn + he, bn + 3 * he, bn + 5 * he, bn + 7 * he},
                             {m.im(P.i_w3[0]), m.im(P.i_w3[1]), m.im(P.i_w3[2]), m.im(P.i_w3[3])}, m.im(P.i_m2s), m.im(P.i_m2r),
                             m.im(P.i_m3_0), m.im(P.i_ps), m.im(P.i_pr), m.im(P.i_m4e), a.send, a.recv, a.order, a.rowptr,
                             (float)(a.num_vars - 1), m.wp(L.X1a), m.wp(L.X1), Ps, Ps + (size_t)Nn * he, m.wp(L.T2), m.wp(L.X2),
                             m.wp(L.X2n), m.wp(L.X3a), m.wp(L.X3), m.wp(L.T4), x4, he, Nn, E};
        if (int rc = nri_dnri_prior(p, c, first_jobs, st)) return rc;
        if (a.features_out) return AETHER_OK;
        // one LSTM step per edge (:415-421), prior_fc_out (:422)
        if (int rc = nri_lstm_head(NriLstmHead{p->lstm_w_ih, p->lstm_w_hh, m.pl(P.lb), m.pl(P.lbp), m.im(P.i_ih), m.im(P.i_hh),
                                               p->prior_w, p->prior_b,
                                               {m.im(P.i_prior[0]), m.im(P.i_prior[1]), m.im(P.i_prior[2]), m.im(P.i_prior[3])},
                                               x4, h0, c0, m.wp(L.G), h1, c1, m.wp(L.Y1), m.wp(L.Y2), m.wp(L.logits), he, a.R,
                                               a.prior_layers, a.ph, K, E}, st)) return rc;
    } else {                           // (given logits: what rides in mlp1's launch goes alone)
        S2SJobs T;
        T.n = 0;
        if (int rc = first_jobs(T)) return rc;
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    }
    if (edges != nullptr)
        k_s2s_gumbel_select<<<nri_blocks(E), dim3(256), 0, st>>>(a.ext_logits ? a.ext_logits : m.wp(L.logits), uniform, a.tau, K, k0,
                                                                edges, lists, counts, E);
    return AETHER_OK;
}

// One step.  x_in [Nn][2D], dh_in [Nn][hd] (recurrent decoder), h0 / c0 [E][R], uniform [E][K] -> x_out, dh_out, h1, c1 (+
// edges_out [E][K] when not null).  decode = false (MLP decoder only): the prior alone -- no sample, no decoder.
int s2s_dnri_step_impl(const DnriArgs& a, char* ws, const float* x_in, const float* dh_in, const float* h0, const float* c0,
                       const float* uniform, float* x_out, float* dh_out, float* h1, float* c1, float* edges_out, bool decode,
                       hipStream_t st) {
    const int D = a.D, hd = a.hd, K = a.K, k0 = a.skip_first ? 1 : 0;
    const int64_t Nn = a.Nn, E = a.E;
    const DnriPlanLayout& P = a.P;
    const DnriStepLayout& L = a.L;
    const NriMem m{ws, a.plan};
    const AetherS2SDnriDecoderParams* q = a.dp;
    const AetherS2SDnriMlpParams* mp = a.mp;
    float* edges = !decode ? nullptr : edges_out ? edges_out : m.wp(L.edges);
    // what either decoder's message layers and the recurrent decoder's chain (host_nri_chain.inc) use; the sample is its own scale
    const NriDnriDecoder d{{m.im(P.i_a[0]), m.im(P.i_a[1]), m.im(P.i_a[2]), m.im(P.i_a[3])},
                           {m.im(P.i_s[0]), m.im(P.i_s[1]), m.im(P.i_s[2]), m.im(P.i_s[3])},
                           {m.im(P.i_msg2[0]), m.im(P.i_msg2[1]), m.im(P.i_msg2[2]), m.im(P.i_msg2[3])}, m.im(P.i_hr), m.im(P.i_hi),
                           m.im(P.i_hh2), m.im(P.i_out1), m.im(P.i_out2), a.fld ? m.wp(a.fld->ext) : x_in, dh_in, edges, edges,
                           reinterpret_cast<const int64_t*>(ws + L.lists), a.send, a.recv, reinterpret_cast<const int*>(ws + L.counts),
                           m.wp(L.A), m.wp(L.S), m.wp(L.Tm), m.wp(L.M), m.wp(L.agg), m.wp(L.hr), m.wp(L.hi), m.wp(L.hh), m.wp(L.o1),
                           m.wp(L.o2), dh_out, a.fld ? 3 * D : 2 * D, hd, K, k0, Nn, E, false};
    // the receiver | sender halves of msg_fc1 on the hidden state (:489-493, :508) ride in mlp1's launch
    auto first_jobs = [&](S2SJobs& F) {
        if (q == nullptr) return (int)AETHER_OK;
        for (int k = k0; k < K; ++k) {
            if (F.n > S2S_MAX_JOBS - 2) { if (int rc = s2s_launch_jobs(F, st)) return rc; F.n = 0; }
            nri_dnri_msg1_pair(q, d, k, F);
        }
        return (int)AETHER_OK;
    };
    if (int rc = s2s_dnri_front(a, ws, x_in, h0, c0, uniform, h1, c1, edges, first_jobs, st)) return rc;
    if (!decode) return AETHER_OK;
    if (q) {
        // / norm, sum per receiver / (N - 1) (:512-516) between the messages and the GRU gate (:519-525)
        auto aggregate = [&] {
            k_s2s_dnri_aggregate<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(d.M, a.order, a.rowptr, d.agg, hd, hd, (float)(K - k0),
                                                                          (float)(a.num_vars - 1));
        };
        if (int rc = nri_dnri_decoder(q, d, aggregate, st)) return rc;
    } else {
        // ReLU pair, second layer without tanh, plain sum per receiver behind the staged inputs (:612-616): [inputs, 0 .. | agg]
        k_s2s_dnri_pair<true><<<nri_blocks(E * (hd / 4)), dim3(256), 0, st>>>(d.A, d.S, Nn, a.send, a.recv, edges, K, k0, d.Tm, d.M,
                                                                              hd, E);
        if (int rc = nri_dnri_msg2(2, mp->msg_fc2_w, mp->msg_fc2_b, d, st)) return rc;
        k_s2s_dnri_aggregate<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(d.M, a.order, a.rowptr, d.agg + S2S_RFG, L.ldagg, hd, 1.0f,
                                                                      1.0f);
        if (int rc = nri_one(st, s2s_job(2, m.pl(P.o1p), P.ldo1, mp->out1_b, d.agg, L.ldagg, d.o1, hd, hd, P.ldo1, Nn), d.img_out1))
            return rc;
        if (int rc = nri_one(st, s2s_job(2, mp->out2_w, hd, mp->out2_b, d.o1, hd, d.o2, hd, hd, hd, Nn), d.img_out2)) return rc;
    }
    // ---- last layer of the output MLP and residual (:528-532, :619-624)
    const float* w3 = q ? q->out3_w : mp->out3_w;
    const float* b3 = q ? q->out3_b : mp->out3_b;
    dispatch_dim(D, [&](auto DD) {
        k_s2s_dnri_out<decltype(DD)::value><<<dim3((unsigned)((Nn + 3) / 4)), dim3(256), 0, st>>>(d.o2, w3, b3, hd, x_in, x_out, Nn);
    });
    return AETHER_OK;
}

DnriSizes s2s_dnri_sizes(int D, int he, int hd, int R, int prior_layers, int ph, int K, int skip_first, int num_vars, float tau,
                         int64_t Nn, int64_t E) {
    return DnriSizes{D, he, hd, R, prior_layers, ph, K, skip_first, num_vars, tau, Nn, E};
}
}  // namespace

/* see include/aether_hip.h */
size_t aether_s2s_dnri_plan_bytes(const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, int num_dims,
                                  int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                  int num_edge_types, int skip_first) {
    const int ku = s2s_dnri_ku(dp, mp, num_edge_types, skip_first);
    if (ku == 0 || !s2s_dnri_sizes_ok(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types))
        return 0;
    return DnriPlanLayout(encoder_hidden, decoder_hidden, num_edge_types, rnn_hidden, prior_layers, prior_hidden, ku).total;
}

namespace {
// The plan's contents (after the entry's checks).  xcols: the columns of out_fc1 in front of the aggregated messages -- 2D, or
// the 3D of DNRIAether's [inputs | field]
int s2s_dnri_plan_fill(const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp,
                       int xcols, int he, int hd, int R, int prior_layers, int prior_hidden, int K, int skip_first, char* base,
                       hipStream_t st) {
    const DnriPlanLayout P(he, hd, K, R, prior_layers, prior_hidden, s2s_dnri_ku(dp, mp, K, skip_first));
    auto fl = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    for (int l = 0; l < 4; ++l) {
        k_s2s_bn_affine<<<blocks(he), dim3(256), 0, st>>>(pp->mlp_bn_w[l], pp->mlp_bn_b[l], pp->mlp_bn_mean[l], pp->mlp_bn_var[l],
                                                         fl(P.bn) + (size_t)2 * l * he, fl(P.bn) + (size_t)(2 * l + 1) * he, he);
        s2s_image(base, st, P.i_w3[l], pp->mlp_w3[l], he, he, he);
    }
    k_s2s_add_vec<<<blocks(4 * R), dim3(256), 0, st>>>(pp->lstm_b_ih, pp->lstm_b_hh, fl(P.lb), 4 * R);
    k_s2s_lstm_bias_interleave<<<blocks(4 * R), dim3(256), 0, st>>>(pp->lstm_b_ih, pp->lstm_b_hh, fl(P.lbp), R);
    s2s_image(base, st, P.i_m2s, pp->mlp_w0[1], he, he, 2 * he);
    s2s_image(base, st, P.i_m2r, pp->mlp_w0[1] + he, he, he, 2 * he);
    s2s_image(base, st, P.i_m3_0, pp->mlp_w0[2], he, he, he);
    s2s_image(base, st, P.i_ps, pp->mlp_w0[3], he, he, 3 * he);
    s2s_image(base, st, P.i_pr, pp->mlp_w0[3] + he, he, he, 3 * he);
    s2s_image(base, st, P.i_m4e, pp->mlp_w0[3] + 2 * he, he, he, 3 * he);
    s2s_image(base, st, P.i_ih, pp->lstm_w_ih, 4 * R, he, he, R);                  // gates interleaved by unit (S2SJob act 5)
    s2s_image(base, st, P.i_hh, pp->lstm_w_hh, 4 * R, R, R, R);
    for (int l = 0; l + 1 < prior_layers; ++l)
        s2s_image(base, st, P.i_prior[l], pp->prior_w[l], prior_hidden, l == 0 ? R : prior_hidden, l == 0 ? R : prior_hidden);
    if (dp) {
        for (int k = 0; k < K; ++k) {
            s2s_image(base, st, P.i_a[k], dp->msg_fc1_w[k], hd, hd, 2 * hd);
            s2s_image(base, st, P.i_s[k], dp->msg_fc1_w[k] + hd, hd, hd, 2 * hd);
            s2s_image(base, st, P.i_msg2[k], dp->msg_fc2_w[k], hd, hd, hd);
        }
        s2s_image(base, st, P.i_hr, dp->hidden_r_w, hd, hd, hd);
        s2s_image(base, st, P.i_hi, dp->hidden_i_w, hd, hd, hd);
        s2s_image(base, st, P.i_hh2, dp->hidden_h_w, hd, hd, hd);
        s2s_image(base, st, P.i_out1, dp->out1_w, hd, hd, hd);
        s2s_image(base, st, P.i_out2, dp->out2_w, hd, hd, hd);
    } else {
        for (int k = skip_first ? 1 : 0; k < K; ++k) s2s_image(base, st, P.i_msg2[k], mp->msg_fc2_w[k], hd, hd, hd);
        k_s2s_dnri_pad_front<<<blocks((int64_t)hd * P.ldo1), dim3(256), 0, st>>>(mp->out1_w, xcols, S2S_RFG, hd, fl(P.o1p), hd);
        s2s_image(base, st, P.i_out1, fl(P.o1p), hd, P.ldo1, P.ldo1);
        s2s_image(base, st, P.i_out2, mp->out2_w, hd, hd, hd);
    }
    return AETHER_OK;
}
}  // namespace

int aether_s2s_dnri_plan_build(const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp,
                               const AetherS2SDnriMlpParams* mp, int num_dims, int encoder_hidden, int decoder_hidden,
                               int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first, void* plan,
                               size_t plan_bytes, void* stream) {
    const char* what = "s2s_dnri_plan_build";
    if (!pp || !plan) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    const size_t need = aether_s2s_dnri_plan_bytes(dp, mp, num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers,
                                                   prior_hidden, num_edge_types, skip_first);
    if (int rc = s2s_plan_buffer_check(what, need, plan, plan_bytes)) return rc;
    if (int rc = s2s_dnri_plan_fill(pp, dp, mp, 2 * num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                    num_edge_types, skip_first, (char*)plan, (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_dnri_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                       int num_edge_types, int64_t n_nodes, int64_t n_edges) {
    if ((num_dims != 2 && num_dims != 3) || encoder_hidden <= 0 || decoder_hidden <= 0 || rnn_hidden <= 0 || prior_hidden < 0 ||
        num_edge_types < 1 || num_edge_types > 4 || n_nodes <= 0 || n_edges <= 0)
        return 0;
    return DnriStepLayout(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden, num_edge_types, n_nodes, n_edges).total;
}

int aether_s2s_dnri_step(const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp,
                         const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                         int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                         int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                         const float* inputs, const float* ext_logits, const float* decoder_hidden_in, const float* h0,
                         const float* c0, const float* uniform, void* workspace, size_t workspace_bytes, float* outputs,
                         float* decoder_hidden_out, float* h1, float* c1, float* edges_out, float* logits_out, void* stream) {
    (void)polar;
    const char* what = "s2s_dnri_step";
    const DnriSizes z = s2s_dnri_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                       num_edge_types, skip_first, num_vars, tau, n_nodes, n_edges);
    if (int rc = s2s_dnri_entry_check(what, pp, dp, mp, plan, z,
                                      send && recv && order && rowptr && inputs && uniform && workspace && outputs &&
                                          (ext_logits || (h0 && c0 && h1 && c1)) && (mp || (decoder_hidden_in && decoder_hidden_out)),
                                      0, 1)) return rc;
    if (logits_out && ext_logits) return s2s_fail(AETHER_EINVAL, what, "logits_out is the prior's logits: not with ext_logits");
    DnriArgs a = s2s_dnri_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    if (workspace_bytes < a.L.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    a.ext_logits = ext_logits;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = s2s_dnri_step_impl(a, (char*)workspace, inputs, mp ? nullptr : decoder_hidden_in, h0, c0, uniform, outputs,
                                    mp ? nullptr : decoder_hidden_out, h1, c1, edges_out, true, st)) return rc;
    if (logits_out)
        HIP_OK(hipMemcpyAsync(logits_out, (const char*)workspace + a.L.logits, (size_t)n_edges * num_edge_types * sizeof(float),
                              hipMemcpyDeviceToDevice, st));
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_dnri_rollout(const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp,
                            const AetherS2SDnriMlpParams* mp, const void* plan, int num_dims, int encoder_hidden, int decoder_hidden,
                            int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first, int polar,
                            int num_vars, float tau, int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv,
                            const int64_t* order, const int64_t* rowptr, int burn_in_steps, const float* burn_in, int steps,
                            const float* inputs, float* decoder_state, float* h, float* c, const float* uniform, void* workspace,
                            size_t workspace_bytes, float* predictions, float* edges_out, void* stream) {
    (void)polar;
    const char* what = "s2s_dnri_rollout";
    const DnriSizes z = s2s_dnri_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                       num_edge_types, skip_first, num_vars, tau, n_nodes, n_edges);
    if (int rc = s2s_dnri_entry_check(what, pp, dp, mp, plan, z,
                                      send && recv && order && rowptr && inputs && h && c && uniform && workspace &&
                                          (mp || decoder_state) && (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                      burn_in_steps, steps)) return rc;
    const DnriArgs a = s2s_dnri_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    if (workspace_bytes < a.L.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const DnriStepLayout& L = a.L;
    auto step = [&](int, bool, const S2SStateIn& cur, const float* u, const S2SStateOut& next, float* eout, bool decode) {
        return s2s_dnri_step_impl(a, ws, cur.x, cur.dh, cur.h, cur.c, u, next.x, next.dh, next.h, next.c, eout, decode, st);
    };
    return nri_rollout(ws, NriRolloutWs{L.xa, L.da, L.db, L.ha, L.hb, L.ca, L.cb, a.D, a.hd, a.R, a.K, a.Nn, a.E}, burn_in_steps,
                       burn_in, steps, inputs, dp ? decoder_state : nullptr, h, c, uniform, predictions, edges_out, step, st);
}

int aether_s2s_dnri_encoder_features(const AetherS2SDnriPriorParams* pp, const AetherS2SDnriDecoderParams* dp,
                                     const AetherS2SDnriMlpParams* mp, const void* plan, int num_dims, int encoder_hidden,
                                     int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                                     int skip_first, int polar, int num_vars, int64_t n_nodes, int64_t n_edges, const int64_t* send,
                                     const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                                     void* workspace, size_t workspace_bytes, float* features, void* stream) {
    (void)polar;
    const char* what = "s2s_dnri_encoder_features";
    const DnriSizes z = s2s_dnri_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                       num_edge_types, skip_first, num_vars, 1.0f, n_nodes, n_edges);
    if (int rc = s2s_dnri_entry_check(what, pp, dp, mp, plan, z,
                                      send && recv && order && rowptr && inputs && workspace && features, 0, 1)) return rc;
    DnriArgs a = s2s_dnri_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    if (workspace_bytes < a.L.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    a.features_out = features;
    auto no_jobs = [](S2SJobs&) { return (int)AETHER_OK; };
    if (int rc = s2s_dnri_front(a, (char*)workspace, inputs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, no_jobs,
                                (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
