// Host side of the C ABI: the Markov decoder of the seq2seq Aether (decoder_type 'ref_mlp'), per module and fused.
// Included by aether_hip.hip inside its extern "C" block after host_s2s_step.inc; not a stand-alone source file.

namespace {

struct S2SMarkovLayout {
    size_t ext, rel, relp, Rinv, ea, eap, epos, l1p, r1p, b2, T1, M, aug, o1, o2, lists, counts, total;
    S2SMarkovLayout(int D, int h, int64_t Nn, int64_t E) {
        const S2SDims d(D);
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, g = (size_t)h;
        ext = take(nn * 3 * D); rel = take(nn * d.RF); relp = take(nn * d.RFp); Rinv = take(nn * D * D);
        ea = take(ee * d.EA); eap = take(ee * d.EAp); epos = take(ee * d.EP);
        l1p = take(g * d.EAp); r1p = take(g * d.RFp); b2 = take(4 * g);
        T1 = take(ee * g); M = take(ee * g); aug = take(nn * g); o1 = take(nn * g); o2 = take(nn * g);
        lists = take(ee * 4 * 2); counts = take(64);
        total = off;
    }
};

int s2s_markov_check(const AetherS2SMarkovParams* mp, int D, int h, int K, int skip_first) {
    if (!mp || !mp->lin1_w || !mp->lin1_b || !mp->lin2_w || !mp->lin2_b || !mp->res1_w || !mp->res1_b || !mp->out0_w ||
        !mp->out0_b || !mp->out3_w || !mp->out3_b || !mp->out6_w || !mp->out6_b)
        return fail(AETHER_EINVAL, "s2s_markov: null parameter pointer");
    if (D != 2 && D != 3) return fail(AETHER_EINVAL, "s2s_markov: num_dims must be 2 or 3");
    if (h < 32 || h % 32 != 0) return fail(AETHER_EINVAL, "s2s_markov: hidden must be a multiple of 32");
    if (K < 1 || K > 4 || K - (skip_first ? 1 : 0) < 1) return fail(AETHER_EINVAL, "s2s_markov: 1..4 edge types, at least one used");
    return AETHER_OK;
}

// Hard samples of the fused step: the sample, its lists / counts and the local frames are in the step's workspace (S2SStepLayout).
// decode = false: the prior only (burn-in).  x_in [Nn][2D], h0 / c0 [E][R], uniform [E][K] -> x_out, h1, c1 (+ edges_out).
int s2s_markov_step_impl(const S2SStepArgs& a, char* ws, const float* x_in, const float* ext_field, const float* h0,
                         const float* c0, const float* uniform, float* x_out, float* h1, float* c1, float* edges_out,
                         bool decode, hipStream_t st) {
    const int D = a.D, hd = a.hd, K = a.K, k0 = a.skip_first ? 1 : 0, ku = K - k0;
    const int64_t Nn = a.Nn, E = a.E;
    const S2SDims d(D, a.locs);
    const AetherS2SMarkovParams* mp = a.mp;
    const S2SPlanLayout& P = a.P;
    const S2SStepLayout& L = a.L;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto pl = [&](size_t off) { return reinterpret_cast<const float*>(a.plan + off); };
    auto im = [&](size_t off) { return off ? reinterpret_cast<const void*>(a.plan + off) : nullptr; };
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int64_t* lists = reinterpret_cast<int64_t*>(ws + L.lists);
    float* edges = edges_out ? edges_out : wp(L.edges);
    float* T1 = wp(L.Tm);               // relu(lin1(edge_attr)) [E][hd]
    float* M = wp(L.M1);                // messages [E][hd] (rows of listed edges only)
    float* aug = wp(L.rp);              // res1(rel_feat), then + the receiver mean [Nn][hd]
    auto no_jobs = [](S2SJobs&) { return (int)AETHER_OK; };
    // lin1 on every edge and the decoder's res1 ride in the prior's res1 launch (all three read only the local frames)
    auto res1_jobs = [&](S2SJobs& T) {
        T.j[T.n++] = s2s_job(2, pl(P.m_l1p), d.EAp, mp->lin1_b, wp(L.eap), d.EAp, T1, hd, hd, d.EAp, E);
        T.j[T.n++] = s2s_job(0, pl(P.m_r1p), d.RFp, mp->res1_b, wp(L.relp), d.RFp, aug, hd, hd, d.RFp, Nn);
        return (int)AETHER_OK;
    };
    if (!decode) return s2s_front_impl(a, L, P, ws, x_in, ext_field, h0, c0, uniform, h1, c1, nullptr, no_jobs, no_jobs, st);
    if (int rc = s2s_front_impl(a, L, P, ws, x_in, ext_field, h0, c0, uniform, h1, c1, edges, no_jobs, res1_jobs, st)) return rc;
    // second layer per used type on that type's edge list only, scaled by the edge's weight; rows written, not accumulated
    // (an edge sits in at most one list)
    S2SJobs T;
    T.n = 0;
    for (int k = k0; k < K; ++k) {
        S2SJob J = s2s_job(2, mp->lin2_w + (size_t)(k - k0) * hd, ku * hd, pl(P.m_b2) + (size_t)(k - k0) * hd, T1, hd, M, hd, hd,
                           hd, E);
        J.xidx = lists + (size_t)k * E; J.yidx = lists + (size_t)k * E; J.n_dev = counts + k;
        J.scale = edges + k; J.sstride = K; J.Wimg = im(P.m_i_l2[k - k0]);
        T.j[T.n++] = J;
    }
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    k_s2s_markov_agg<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(M, a.order, a.rowptr, edges, K, k0, aug, hd);
    return s2s_out_tail(a, ws, mp, aug, x_in, x_out, st);
}

// The Markov decoder's prepared weights (ku used edge types) into a plan of its layout.
void s2s_plan_build_markov(const AetherS2SMarkovParams* mp, int D, int hd, int ku, const S2SPlanLayout& P, char* base,
                           hipStream_t st, int locs = 0) {
    const S2SDims d(D, locs);
    auto fl = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    k_s2s_pad_rows<<<blocks((int64_t)hd * d.EAp), dim3(256), 0, st>>>(mp->lin1_w, d.EA, d.EA, fl(P.m_l1p), d.EAp, hd);
    k_s2s_pad_rows<<<blocks((int64_t)hd * d.RFp), dim3(256), 0, st>>>(mp->res1_w, d.RF, d.RF, fl(P.m_r1p), d.RFp, hd);
    k_s2s_markov_bias<<<blocks((int64_t)ku * hd), dim3(256), 0, st>>>(mp->lin2_b, ku, hd, fl(P.m_b2));
    s2s_out_images(base, st, P, mp->out0_w, mp->out3_w, hd);
    for (int k = 0; k < ku; ++k) s2s_image(base, st, P.m_i_l2[k], mp->lin2_w + (size_t)k * hd, hd, hd, ku * hd);    // type k's rows c Ku + k
}
}  // namespace

size_t aether_s2s_markov_decoder_workspace_bytes(int num_dims, int hidden, int64_t n_nodes, int64_t n_edges) {
    if ((num_dims != 2 && num_dims != 3) || hidden <= 0 || n_nodes <= 0 || n_edges < 0) return 0;
    return S2SMarkovLayout(num_dims, hidden, n_nodes, n_edges).total;
}

int aether_s2s_markov_decoder_step(const AetherS2SMarkovParams* p, int num_dims, int hidden, int num_edge_types,
                                   int skip_first, int64_t n_nodes, int64_t n_edges, const float* inputs,
                                   const float* edge_w, const float* field, const int64_t* send, const int64_t* recv,
                                   const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                                   float* outputs, void* stream) {
    if (int rc = s2s_markov_check(p, num_dims, hidden, num_edge_types, skip_first)) return rc;
    if (!inputs || !field || !workspace || !outputs || !rowptr) return fail(AETHER_EINVAL, "s2s_markov: null pointer");
    if (n_edges > 0 && (!edge_w || !send || !recv || !order)) return fail(AETHER_EINVAL, "s2s_markov: null edge pointer");
    if (n_nodes <= 0 || n_edges < 0) return fail(AETHER_EINVAL, "s2s_markov: bad sizes");
    const int D = num_dims, h = hidden, K = num_edge_types, k0 = skip_first ? 1 : 0, ku = K - k0;
    const S2SDims d(D);
    const S2SMarkovLayout L(D, h, n_nodes, n_edges);
    if (workspace_bytes < L.total) return fail(AETHER_ESPACE, "s2s_markov: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    const int64_t Nn = n_nodes, E = n_edges;
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    auto elist = [&](int k) { return reinterpret_cast<int64_t*>(ws + L.lists) + (size_t)k * E; };
    // ---- local frames of [inputs | field] (:465-470), the kernels of aether_s2s_localize (the per-module recurrent step's), and
    // the zero-padded rows the dense layers read.  (Every node's origin edge has an Euler angle on its branch cut, +-pi by one
    // rounding; these kernels land where the reference's fp32 evaluation does, tests/test_gpu_seq2seq.py localizer tests.)
    HIP_OK(hipMemsetAsync(counts, 0, 64 * sizeof(int), st));
    dispatch_dim(D, [&](auto DD) {
        constexpr int Dc = decltype(DD)::value;
        k_s2s_aug_nodes<Dc><<<blocks(Nn), dim3(256), 0, st>>>(nullptr, wp(L.rel), wp(L.Rinv), Nn, inputs, field, wp(L.ext));
        if (E > 0) k_s2s_aug_edges<Dc><<<blocks(E), dim3(256), 0, st>>>(wp(L.ext), send, recv, wp(L.rel), 1, wp(L.ea), wp(L.epos), E);
    });
    k_s2s_pad_rows<<<blocks(Nn * d.RFp), dim3(256), 0, st>>>(wp(L.rel), d.RF, d.RF, wp(L.relp), d.RFp, Nn);
    if (E > 0) k_s2s_pad_rows<<<blocks(E * d.EAp), dim3(256), 0, st>>>(wp(L.ea), d.EA, d.EA, wp(L.eap), d.EAp, E);
    // ---- padded lin1 / res1 and lin2's bias per type (the plan's preparation, per call here)
    k_s2s_pad_rows<<<blocks((int64_t)h * d.EAp), dim3(256), 0, st>>>(p->lin1_w, d.EA, d.EA, wp(L.l1p), d.EAp, h);
    k_s2s_pad_rows<<<blocks((int64_t)h * d.RFp), dim3(256), 0, st>>>(p->res1_w, d.RF, d.RF, wp(L.r1p), d.RFp, h);
    k_s2s_markov_bias<<<blocks((int64_t)ku * h), dim3(256), 0, st>>>(p->lin2_b, ku, h, wp(L.b2));
    // ---- lin1 (:482) on every edge and res1 (:492) in one launch
    S2SJobs T;
    T.n = 0;
    if (E > 0) T.j[T.n++] = s2s_job(2, wp(L.l1p), d.EAp, p->lin1_b, wp(L.eap), d.EAp, wp(L.T1), h, h, d.EAp, E);
    T.j[T.n++] = s2s_job(0, wp(L.r1p), d.RFp, p->res1_b, wp(L.relp), d.RFp, wp(L.aug), h, h, d.RFp, Nn);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    // ---- lin2 per used type on the edges whose weight for it is not zero, times that weight, summed over types (:483-486)
    if (E > 0) {
        HIP_OK(hipMemsetAsync(wp(L.M), 0, (size_t)E * h * 4, st));
        for (int k = k0; k < K; ++k) {
            k_s2s_select<<<blocks(E), dim3(256), 0, st>>>(edge_w, K, k, E, elist(k), counts + k);
            if (s2s_linear(2, p->lin2_w + (size_t)(k - k0) * h, ku * h, wp(L.b2) + (size_t)(k - k0) * h, wp(L.T1), wp(L.M), h, h, E,
                           h, edge_w + k, K, 1, st, elist(k), elist(k), counts + k)) return AETHER_EINVAL;
        }
    }
    // ---- receiver mean + res1 (:487-493), output MLP, globalise, residual (:495-503)
    k_s2s_markov_agg<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(wp(L.M), order, rowptr, nullptr, K, k0, wp(L.aug), h);
    if (s2s_linear(2, p->out0_w, h, p->out0_b, wp(L.aug), wp(L.o1), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(2, p->out3_w, h, p->out3_b, wp(L.o1), wp(L.o2), h, h, Nn, h, nullptr, 0, 0, st)) return AETHER_EINVAL;
    dispatch_dim(D, [&](auto DD) {
        k_s2s_out_globalize<decltype(DD)::value><<<dim3((unsigned)((Nn + 3) / 4)), dim3(256), 0, st>>>(
            wp(L.o2), p->out6_w, p->out6_b, h, inputs, wp(L.Rinv), outputs, Nn);
    });
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_markov_plan_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                    int prior_hidden, int num_edge_types, int skip_first) {
    const int ku = num_edge_types - (skip_first ? 1 : 0);
    return ku < 1 ? 0 : s2s_plan_size(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                      num_edge_types, ku);
}

int aether_s2s_markov_plan_build(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp,
                                 const AetherS2SMarkovParams* mp, int num_dims, int encoder_hidden, int decoder_hidden,
                                 int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first,
                                 void* plan, size_t plan_bytes, void* stream) {
    if (!pp || !plan) return fail(AETHER_EINVAL, "s2s_markov_plan_build: null pointer");
    if (int rc = s2s_markov_check(mp, num_dims, decoder_hidden, num_edge_types, skip_first)) return rc;
    const int D = num_dims, he = encoder_hidden, hd = decoder_hidden, K = num_edge_types, ku = K - (skip_first ? 1 : 0);
    if (int rc = s2s_plan_buffer_check("s2s_markov_plan_build",
                                       s2s_plan_size(D, he, hd, rnn_hidden, prior_layers, prior_hidden, K, ku), plan, plan_bytes))
        return rc;
    const S2SPlanLayout P(D, he, hd, K, rnn_hidden, prior_layers, prior_hidden, ku);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)plan;
    s2s_plan_build_front(fp, pp, D, he, rnn_hidden, prior_layers, prior_hidden, P, base, st);
    s2s_plan_build_markov(mp, D, hd, ku, P, base, st);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int aether_s2s_markov_step(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SMarkovParams* mp,
                           const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden,
                           int prior_layers, int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars,
                           float tau, int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv,
                           const int64_t* order, const int64_t* rowptr, const float* inputs, const float* ext_field,
                           const float* h0, const float* c0, const float* uniform, void* workspace, size_t workspace_bytes,
                           float* outputs, float* h1, float* c1, float* edges_out, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    if (int rc = s2s_entry_check("s2s_markov_step", true, fp, pp, nullptr, mp, plan, z, ext_field == nullptr,
                                 send && recv && order && rowptr && inputs && h0 && c0 && uniform && workspace && outputs && h1 && c1,
                                 0, 1)) return rc;
    return s2s_run_step("s2s_markov_step", s2s_step_args(fp, pp, nullptr, mp, plan, z, send, recv, order, rowptr), workspace,
                        workspace_bytes, {inputs, nullptr, h0, c0}, ext_field, uniform, {outputs, nullptr, h1, c1}, edges_out,
                        stream);
}

int aether_s2s_markov_rollout(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SMarkovParams* mp,
                              const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden,
                              int prior_layers, int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars,
                              float tau, int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv,
                              const int64_t* order, const int64_t* rowptr, int burn_in_steps, const float* burn_in, int steps,
                              const float* inputs, float* h, float* c, const float* uniform, void* workspace,
                              size_t workspace_bytes, float* predictions, float* edges_out, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    if (int rc = s2s_entry_check("s2s_markov_rollout", true, fp, pp, nullptr, mp, plan, z, true,
                                 send && recv && order && rowptr && inputs && h && c && uniform && workspace &&
                                     (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                 burn_in_steps, steps)) return rc;
    return s2s_run_rollout("s2s_markov_rollout", s2s_step_args(fp, pp, nullptr, mp, plan, z, send, recv, order, rowptr),
                           workspace, workspace_bytes, burn_in_steps, burn_in, steps, inputs, nullptr, h, c, uniform,
                           predictions, edges_out, stream);
}
