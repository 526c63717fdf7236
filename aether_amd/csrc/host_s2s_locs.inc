// Host side of the C ABI: the seq2seq LoCS baseline (nn/seq2seq/locs.py) -- the fused step of host_s2s_step.inc /
// host_s2s_markov.inc behind the plain localizer (s2s_locs.h): plan, step (also as the decoder on given logits), device
// rollout and the encoder's per-time-step features.  One set of entries for both decoders: exactly one of dp (recurrent)
// and mp (Markov) is given, as for the dynamic-field model.  The model has no field: nothing of the field query is in the
// plan or the workspace, and no launch of it is made.  Included by aether_hip.hip inside its extern "C" block after
// host_s2s_dynfield.inc; not a stand-alone source file.

namespace {

int s2s_locs_entry_check(const char* what, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                         const AetherS2SMarkovParams* mp, const void* plan, const S2SSizes& z, bool pointers, int burn_in_steps,
                         int steps) {
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    return s2s_entry_check(what, mp != nullptr, nullptr, pp, dp, mp, plan, z, false, pointers, burn_in_steps, steps);
}

S2SSizes s2s_locs_sizes(int D, int he, int hd, int R, int prior_layers, int ph, int K, int skip_first, int polar, int num_vars,
                        float tau, int64_t Nn, int64_t E) {
    S2SSizes z{D, he, hd, R, prior_layers, ph, K, skip_first, polar, num_vars, tau, Nn, E};
    z.locs = 1;
    return z;
}

// (after s2s_locs_entry_check: the layouts take the sizes as valid)
extern "C++" S2SStepArgs s2s_locs_step_args(const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                                            const AetherS2SMarkovParams* mp, const void* plan, const S2SSizes& z,
                                            const int64_t* send, const int64_t* recv, const int64_t* order,
                                            const int64_t* rowptr) {
    return S2SStepArgs{z, nullptr, pp, dp, mp, (const char*)plan, send, recv, order, rowptr, false,
                       S2SPlanLayout(z.D, z.he, z.hd, z.K, z.R, z.prior_layers, z.ph, dp ? -1 : z.K - (z.skip_first ? 1 : 0), 0, 0, 1),
                       S2SStepLayout(z.D, z.he, z.hd, z.R, z.ph, z.K, z.Nn, z.E, 0, 1)};
}
}  // namespace

/* see include/aether_hip.h */
size_t aether_s2s_locs_plan_bytes(const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, int num_dims,
                                  int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                  int num_edge_types, int skip_first) {
    const int ku = s2s_dynfield_ku(dp, mp, num_edge_types, skip_first);
    if (ku == 0) return 0;
    if (s2s_plan_size(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, ku) == 0)
        return 0;
    return S2SPlanLayout(num_dims, encoder_hidden, decoder_hidden, num_edge_types, rnn_hidden, prior_layers, prior_hidden, ku, 0, 0,
                         1).total;
}

int aether_s2s_locs_plan_build(const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp,
                               int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                               int prior_hidden, int num_edge_types, int skip_first, void* plan, size_t plan_bytes, void* stream) {
    const char* what = "s2s_locs_plan_build";
    if (!pp || !plan) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    if (mp)
        if (int rc = s2s_markov_check(mp, num_dims, decoder_hidden, num_edge_types, skip_first)) return rc;
    const int D = num_dims, he = encoder_hidden, hd = decoder_hidden, K = num_edge_types;
    const size_t need = aether_s2s_locs_plan_bytes(dp, mp, D, he, hd, rnn_hidden, prior_layers, prior_hidden, K, skip_first);
    if (int rc = s2s_plan_buffer_check(what, need, plan, plan_bytes)) return rc;
    const S2SPlanLayout P(D, he, hd, K, rnn_hidden, prior_layers, prior_hidden, s2s_dynfield_ku(dp, mp, K, skip_first), 0, 0, 1);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)plan;
    s2s_plan_build_front(nullptr, pp, D, he, rnn_hidden, prior_layers, prior_hidden, P, base, st, 0, 1);
    if (dp) s2s_plan_build_recurrent(dp, D, hd, K, P, base, st, 1);
    else s2s_plan_build_markov(mp, D, hd, K - (skip_first ? 1 : 0), P, base, st, 1);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_locs_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                       int num_edge_types, int64_t n_nodes, int64_t n_edges) {
    if (aether_s2s_step_workspace_bytes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden, num_edge_types, n_nodes,
                                        n_edges) == 0)
        return 0;
    return S2SStepLayout(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden, num_edge_types, n_nodes, n_edges, 0,
                         1).total;
}

int aether_s2s_locs_step(const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp,
                         const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                         int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                         int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                         const float* inputs, const float* ext_logits, const float* decoder_hidden_in, const float* h0,
                         const float* c0, const float* uniform, void* workspace, size_t workspace_bytes, float* outputs,
                         float* decoder_hidden_out, float* h1, float* c1, float* edges_out, float* logits_out, void* stream) {
    const char* what = "s2s_locs_step";
    const S2SSizes z = s2s_locs_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                      num_edge_types, skip_first, polar, num_vars, tau, n_nodes, n_edges);
    if (int rc = s2s_locs_entry_check(what, pp, dp, mp, plan, z,
                                      send && recv && order && rowptr && inputs && uniform && workspace && outputs &&
                                          (ext_logits || (h0 && c0 && h1 && c1)) && (mp || (decoder_hidden_in && decoder_hidden_out)),
                                      0, 1)) return rc;
    if (logits_out && ext_logits) return s2s_fail(AETHER_EINVAL, what, "logits_out is the prior's logits: not with ext_logits");
    S2SStepArgs a = s2s_locs_step_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    a.ext_logits = ext_logits;
    if (int rc = s2s_run_step(what, a, workspace, workspace_bytes, {inputs, mp ? nullptr : decoder_hidden_in, h0, c0}, nullptr,
                              uniform, {outputs, mp ? nullptr : decoder_hidden_out, h1, c1}, edges_out, stream)) return rc;
    if (logits_out)
        HIP_OK(hipMemcpyAsync(logits_out, (const char*)workspace + a.L.logits, (size_t)n_edges * num_edge_types * sizeof(float),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AETHER_OK;
}

int aether_s2s_locs_rollout(const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp,
                            const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                            int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                            int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order,
                            const int64_t* rowptr, int burn_in_steps, const float* burn_in, int steps, const float* inputs,
                            float* decoder_state, float* h, float* c, const float* uniform, void* workspace,
                            size_t workspace_bytes, float* predictions, float* edges_out, void* stream) {
    const char* what = "s2s_locs_rollout";
    const S2SSizes z = s2s_locs_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                      num_edge_types, skip_first, polar, num_vars, tau, n_nodes, n_edges);
    if (int rc = s2s_locs_entry_check(what, pp, dp, mp, plan, z,
                                      send && recv && order && rowptr && inputs && h && c && uniform && workspace &&
                                          (mp || decoder_state) && (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                      burn_in_steps, steps)) return rc;
    return s2s_run_rollout(what, s2s_locs_step_args(pp, dp, mp, plan, z, send, recv, order, rowptr), workspace, workspace_bytes,
                           burn_in_steps, burn_in, steps, inputs, mp ? nullptr : decoder_state, h, c, uniform, predictions,
                           edges_out, stream);
}

int aether_s2s_locs_encoder_features(const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                                     const AetherS2SMarkovParams* mp, const void* plan, int num_dims, int encoder_hidden,
                                     int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                                     int skip_first, int polar, int num_vars, int64_t n_nodes, int64_t n_edges, const int64_t* send,
                                     const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                                     void* workspace, size_t workspace_bytes, float* features, void* stream) {
    const char* what = "s2s_locs_encoder_features";
    const S2SSizes z = s2s_locs_sizes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden,
                                      num_edge_types, skip_first, polar, num_vars, 1.0f, n_nodes, n_edges);
    if (int rc = s2s_locs_entry_check(what, pp, dp, mp, plan, z,
                                      send && recv && order && rowptr && inputs && workspace && features, 0, 1)) return rc;
    S2SStepArgs a = s2s_locs_step_args(pp, dp, mp, plan, z, send, recv, order, rowptr);
    if (workspace_bytes < a.L.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    a.features_out = features;
    auto no_jobs = [](S2SJobs&) { return (int)AETHER_OK; };
    if (int rc = s2s_front_impl(a, a.L, a.P, (char*)workspace, inputs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, no_jobs, no_jobs, (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
