// Host side of the C ABI: the seq2seq ablation DNRIAether (nn/seq2seq/ablations/dnri_aether.py) -- the dNRI engine of
// host_s2s_dnri.inc with the field query of the seq2seq Aether in front of it.  A step is k_s2s_rff, field_net.0 / .2 as
// job-table layers, one node kernel (last field layer, ext = [inputs | field], the MLP decoder's node rows), then the dNRI
// step on ext: mlp1's first Linear, the gate and the MLP decoder's msg_fc1 / out_fc1 read 3D columns, everything else is the
// shared chain (host_nri_chain.inc) unchanged.  With the field handed in, no field launch is made.  The plan is dNRI's plus the
// images of the two hidden field layers, the workspace dNRI's plus the field query's rows; nothing of a frame in either.
// Included by aether_hip.hip inside its extern "C" block after host_s2s_dnri.inc; not a stand-alone source file.

namespace {

// Where the field's part lies behind dNRI's plan (plan_base bytes) and workspace (ws_base bytes)
struct DnriFieldLayout {
    DnriFieldArgs f;
    size_t plan_total, ws_total;
    DnriFieldLayout(const AetherS2SFieldParams* fp, size_t plan_base, size_t ws_base, int D, int he, int64_t Nn) {
        size_t off = plan_base;
        auto image = [&](int M, int Kk) {
            if (!S2SPlanLayout::splittable(M, Kk)) return (size_t)0;
            size_t o = off; off = align_up(off + (size_t)M * Kk * 4, 256); return o;
        };
        f.fp = fp;
        f.i_f0 = image(he, he); f.i_f2 = image(he, he);
        plan_total = off;
        off = ws_base;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, h = (size_t)he;
        f.gamma = take(nn * h); f.fh1 = take(nn * h); f.fh2 = take(nn * h); f.field = take(nn * D); f.ext = take(nn * 3 * D);
        ws_total = off;
    }
};

// s2s_dnri_entry_check and what the field adds: its parameters unless every step's field is handed in
int s2s_dnria_entry_check(const char* what, const AetherS2SFieldParams* fp, bool field_given, const AetherS2SDnriPriorParams* pp,
                          const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, const void* plan,
                          const DnriSizes& z, bool pointers, int burn_in_steps, int steps) {
    if (int rc = s2s_dnri_entry_check(what, pp, dp, mp, plan, z, pointers, burn_in_steps, steps)) return rc;
    if (!fp && !field_given) return s2s_fail(AETHER_EINVAL, what, "no field parameters and no field handed in");
    return AETHER_OK;
}

// (declared in host_s2s_dnri.inc, whose front calls it where dNRI runs k_s2s_dnri_node_prep)
int s2s_dnria_node_side(const DnriArgs& a, char* ws, const float* x_in, const AetherS2SDnriMlpParams* mp, hipStream_t st) {
    const int D = a.D, he = a.he;
    const int64_t Nn = a.Nn;
    const DnriFieldArgs& f = *a.fld;
    const NriMem m{ws, a.plan};
    const bool query = a.ext_field == nullptr;
    if (query) {
        // predict_field (dnri_aether.py:81-85): RFF of the positions, field_net.0 / .2 with SiLU; field_net.4 in the node kernel
        const int half = he / 2;
        dispatch_dim(D, [&](auto DD) {
            k_s2s_rff<decltype(DD)::value><<<nri_blocks(Nn * half), dim3(256), 0, st>>>(x_in, 2 * D, f.fp->B, half, m.wp(f.gamma), Nn);
        });
        if (int rc = nri_one(st, s2s_job(1, f.fp->w0, he, f.fp->b0, m.wp(f.gamma), he, m.wp(f.fh1), he, he, he, Nn), m.im(f.i_f0)))
            return rc;
        if (int rc = nri_one(st, s2s_job(1, f.fp->w2, he, f.fp->b2, m.wp(f.fh1), he, m.wp(f.fh2), he, he, he, Nn), m.im(f.i_f2)))
            return rc;
    }
    const float* none = nullptr;
    float* fout = a.field_out ? a.field_out : query ? m.wp(f.field) : nullptr;
    dispatch_dim(D, [&](auto DD) {
        k_s2s_dnria_node_prep<decltype(DD)::value><<<dim3((unsigned)((Nn + 3) / 4)), dim3(256), 0, st>>>(
            x_in, a.ext_field, query ? m.wp(f.fh2) : none, query ? f.fp->w4 : none, query ? f.fp->b4 : none, he, fout, m.wp(f.ext),
            mp ? m.wp(a.L.agg) : nullptr, a.L.ldagg, reinterpret_cast<int*>(ws + a.L.counts), Nn, mp ? mp->msg_fc1_w[0] : none,
            mp ? mp->msg_fc1_w[1] : none, mp ? mp->msg_fc1_w[2] : none, mp ? mp->msg_fc1_w[3] : none, mp ? mp->msg_fc1_b[0] : none,
            mp ? mp->msg_fc1_b[1] : none, mp ? mp->msg_fc1_b[2] : none, mp ? mp->msg_fc1_b[3] : none, a.K, a.skip_first ? 1 : 0,
            m.wp(a.L.A), m.wp(a.L.S), a.hd);
    });
    return AETHER_OK;
}

// The field's layout behind dNRI's plan and workspace (after the entry's checks)
extern "C++" DnriFieldLayout s2s_dnria_layout(const AetherS2SFieldParams* fp, const DnriArgs& a) {
    return DnriFieldLayout(fp, a.P.total, a.L.total, a.D, a.he, a.Nn);
}
}  // namespace

/* see include/aether_hip.h */
size_t aether_s2s_dnri_aether_plan_bytes(const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, int num_dims,
                                         int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                         int num_edge_types, int skip_first) {
    const size_t base = aether_s2s_dnri_plan_bytes(dp, mp, num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers,
                                                   prior_hidden, num_edge_types, skip_first);
    if (base == 0) return 0;
    return DnriFieldLayout(nullptr, base, 0, num_dims, encoder_hidden, 1).plan_total;
}

int aether_s2s_dnri_aether_plan_build(const AetherS2SFieldParams* fp, const AetherS2SDnriPriorParams* pp,
                                      const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, int num_dims,
                                      int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                      int num_edge_types, int skip_first, void* plan, size_t plan_bytes, void* stream) {
    const char* what = "s2s_dnri_aether_plan_build";
    if (!fp || !pp || !plan) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    const int D = num_dims, he = encoder_hidden;
    const size_t need = aether_s2s_dnri_aether_plan_bytes(dp, mp, D, he, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                                          num_edge_types, skip_first);
    if (int rc = s2s_plan_buffer_check(what, need, plan, plan_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)plan;
    // dNRI's plan with out_fc1 padded from 3D + hd columns (:608), then the images of field_net.0 / .2
    if (int rc = s2s_dnri_plan_fill(pp, dp, mp, 3 * D, he, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types,
                                    skip_first, base, st)) return rc;
    const size_t dnri = aether_s2s_dnri_plan_bytes(dp, mp, D, he, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                                   num_edge_types, skip_first);
    const DnriFieldLayout F(fp, dnri, 0, D, he, 1);
    s2s_image(base, st, F.f.i_f0, fp->w0, he, he, he);
    s2s_image(base, st, F.f.i_f2, fp->w2, he, he, he);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_dnri_aether_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                              int num_edge_types, int64_t n_nodes, int64_t n_edges) {
    const size_t base = aether_s2s_dnri_workspace_bytes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden,
                                                        num_edge_types, n_nodes, n_edges);
    if (base == 0) return 0;
    return DnriFieldLayout(nullptr, 0, base, num_dims, encoder_hidden, n_nodes).ws_total;
}

int aether_s2s_dnri_aether_step(const AetherS2SFieldParams* fp, const AetherS2SDnriPriorParams* pp,
                                const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, const void* plan,
                                int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                                int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order,
                                const int64_t* rowptr, const float* inputs, const float* ext_field, const float* ext_logits,
                                const float* decoder_hidden_in, const float* h0, const float* c0, const float* uniform,
                                void* workspace, size_t workspace_bytes, float* outputs, float* decoder_hidden_out, float* h1,
                                float* c1, float* edges_out, float* logits_out, float* field_out, void* stream) {
    (void)polar;
    const char* what = "s2s_dnri_aether_step";
    const DnriSizes z = s2s_dnri_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                       num_edge_types, skip_first, num_vars, tau, n_nodes, n_edges);
    if (int rc = s2s_dnria_entry_check(what, fp, ext_field != nullptr, pp, dp, mp, plan, z,
                                       send && recv && order && rowptr && inputs && uniform && workspace && outputs &&
                                           (ext_logits || (h0 && c0 && h1 && c1)) && (mp || (decoder_hidden_in && decoder_hidden_out)),
                                       0, 1)) return rc;
    if (logits_out && ext_logits) return s2s_fail(AETHER_EINVAL, what, "logits_out is the prior's logits: not with ext_logits");
    DnriArgs a = s2s_dnri_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    const DnriFieldLayout F = s2s_dnria_layout(fp, a);
    if (workspace_bytes < F.ws_total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    a.fld = &F.f; a.ext_field = ext_field; a.field_out = field_out; a.ext_logits = ext_logits;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = s2s_dnri_step_impl(a, (char*)workspace, inputs, mp ? nullptr : decoder_hidden_in, h0, c0, uniform, outputs,
                                    mp ? nullptr : decoder_hidden_out, h1, c1, edges_out, true, st)) return rc;
    if (logits_out)
        HIP_OK(hipMemcpyAsync(logits_out, (const char*)workspace + a.L.logits, (size_t)n_edges * num_edge_types * sizeof(float),
                              hipMemcpyDeviceToDevice, st));
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_dnri_aether_rollout(const AetherS2SFieldParams* fp, const AetherS2SDnriPriorParams* pp,
                                   const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, const void* plan,
                                   int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                   int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                                   int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order,
                                   const int64_t* rowptr, int burn_in_steps, const float* burn_in, const float* burn_in_field,
                                   int steps, const float* inputs, float* decoder_state, float* h, float* c, const float* uniform,
                                   void* workspace, size_t workspace_bytes, float* predictions, float* edges_out, void* stream) {
    (void)polar;
    const char* what = "s2s_dnri_aether_rollout";
    const DnriSizes z = s2s_dnri_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                       num_edge_types, skip_first, num_vars, tau, n_nodes, n_edges);
    // (the predicted steps always query their field: the parameters are needed unless there is none)
    if (int rc = s2s_dnria_entry_check(what, fp, steps <= 0 && burn_in_field != nullptr, pp, dp, mp, plan, z,
                                       send && recv && order && rowptr && inputs && h && c && uniform && workspace &&
                                           (mp || decoder_state) && (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                       burn_in_steps, steps)) return rc;
    DnriArgs a = s2s_dnri_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    const DnriFieldLayout F = s2s_dnria_layout(fp, a);
    if (workspace_bytes < F.ws_total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    a.fld = &F.f;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const DnriStepLayout& L = a.L;
    // burn_in_field [T0][Nn][D] (or null): the field of the burn-in frames, known before the loop starts (:147-149)
    auto step = [&](int t, bool teacher, const S2SStateIn& cur, const float* u, const S2SStateOut& next, float* eout, bool decode) {
        a.ext_field = teacher && burn_in_field ? burn_in_field + (size_t)t * a.Nn * a.D : nullptr;
        return s2s_dnri_step_impl(a, ws, cur.x, cur.dh, cur.h, cur.c, u, next.x, next.dh, next.h, next.c, eout, decode, st);
    };
    return nri_rollout(ws, NriRolloutWs{L.xa, L.da, L.db, L.ha, L.hb, L.ca, L.cb, a.D, a.hd, a.R, a.K, a.Nn, a.E}, burn_in_steps,
                       burn_in, steps, inputs, dp ? decoder_state : nullptr, h, c, uniform, predictions, edges_out, step, st);
}

int aether_s2s_dnri_aether_encoder_features(const AetherS2SFieldParams* fp, const AetherS2SDnriPriorParams* pp,
                                            const AetherS2SDnriDecoderParams* dp, const AetherS2SDnriMlpParams* mp, const void* plan,
                                            int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                            int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars,
                                            int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv,
                                            const int64_t* order, const int64_t* rowptr, const float* inputs, const float* field,
                                            void* workspace, size_t workspace_bytes, float* features, void* stream) {
    (void)polar;
    const char* what = "s2s_dnri_aether_encoder_features";
    const DnriSizes z = s2s_dnri_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                       num_edge_types, skip_first, num_vars, 1.0f, n_nodes, n_edges);
    if (int rc = s2s_dnria_entry_check(what, fp, field != nullptr, pp, dp, mp, plan, z,
                                       send && recv && order && rowptr && inputs && workspace && features, 0, 1)) return rc;
    DnriArgs a = s2s_dnri_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    const DnriFieldLayout F = s2s_dnria_layout(fp, a);
    if (workspace_bytes < F.ws_total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    a.fld = &F.f; a.ext_field = field; a.features_out = features;
    auto no_jobs = [](S2SJobs&) { return (int)AETHER_OK; };
    if (int rc = s2s_dnri_front(a, (char*)workspace, inputs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, no_jobs,
                                (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
