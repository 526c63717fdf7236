// Host side of the C ABI: the fused step and the device rollout of the seq2seq DynamicFieldAether (the gravitational model,
// nn/seq2seq/dynamic_field_aether.py) -- the step of host_s2s_step.inc / host_s2s_markov.inc with the FiLM field query
// (predict_field, :117-134) as its built-in field source.  One set of entries for both decoders: exactly one of dp
// (recurrent) and mp (Markov) is given.  Included by aether_hip.hip inside its extern "C" block after host_s2s_markov.inc;
// not a stand-alone source file.

namespace {

// The FiLM half of an entry's arguments
struct S2SDynfieldArgs {
    const AetherS2SFilmParams* film;
    int mlp_hidden;
    const float* mod;
    size_t mod_bytes;
    int64_t batch;
    int num_objects;
};

int s2s_dynfield_film_check(const char* what, const AetherS2SFilmParams* film, int mlp_hidden) {
    if (!film || !film->B || !film->lin1_w || !film->lin1_b || !film->lin2_w || !film->lin2_b || !film->lin3_w || !film->lin3_b)
        return s2s_fail(AETHER_EINVAL, what, "null FiLM parameter pointer");
    if (mlp_hidden < 16 || mlp_hidden % 16 != 0) return s2s_fail(AETHER_EINVAL, what, "mlp_hidden must be a multiple of 16");
    return AETHER_OK;
}

// The checks of the step / rollout entries: those of s2s_entry_check (the field net replaced by the FiLM one) and the ones of
// the modulation buffer.  gamma / beta are read at row n / num_objects for n < n_nodes, so n_nodes must be batch * num_objects
// and the buffer must hold batch rows: anything else would be a read out of bounds on the device.
int s2s_dynfield_entry_check(const char* what, const S2SDynfieldArgs& f, const AetherS2SPriorParams* pp,
                             const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, const void* plan,
                             const S2SSizes& z, bool pointers, int burn_in_steps, int steps) {
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    if (int rc = s2s_dynfield_film_check(what, f.film, f.mlp_hidden)) return rc;
    if (int rc = s2s_entry_check(what, mp != nullptr, nullptr, pp, dp, mp, plan, z, false, pointers, burn_in_steps, steps)) return rc;
    if (!f.mod) return s2s_fail(AETHER_EINVAL, what, "null modulation buffer");
    if (f.batch <= 0 || f.num_objects <= 0 || z.Nn != f.batch * (int64_t)f.num_objects)
        return s2s_fail(AETHER_EINVAL, what, "n_nodes must be batch * num_objects");
    if (f.mod_bytes < aether_s2s_film_modulation_bytes(f.batch, f.mlp_hidden))
        return s2s_fail(AETHER_ESPACE, what, "modulation buffer too small");
    return AETHER_OK;
}

// (after s2s_dynfield_entry_check: the layouts take the sizes as valid)
extern "C++" S2SStepArgs s2s_dynfield_step_args(const S2SDynfieldArgs& f, const AetherS2SPriorParams* pp,
                                                const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp,
                                                const void* plan, const S2SSizes& z, const int64_t* send, const int64_t* recv,
                                                const int64_t* order, const int64_t* rowptr) {
    S2SStepArgs a{z, nullptr, pp, dp, mp, (const char*)plan, send, recv, order, rowptr, false,
                  S2SPlanLayout(z.D, z.he, z.hd, z.K, z.R, z.prior_layers, z.ph, dp ? -1 : z.K - (z.skip_first ? 1 : 0), f.mlp_hidden),
                  S2SStepLayout(z.D, z.he, z.hd, z.R, z.ph, z.K, z.Nn, z.E, f.mlp_hidden)};
    a.film = f.film; a.mlp_hidden = f.mlp_hidden; a.mod = f.mod; a.batch = f.batch; a.num_objects = f.num_objects;
    return a;
}

// Count of the Markov decoder's used edge types, -1 for the recurrent decoder, 0 (no plan) when not exactly one decoder is given
int s2s_dynfield_ku(const void* dp, const void* mp, int num_edge_types, int skip_first) {
    if ((dp != nullptr) == (mp != nullptr)) return 0;
    if (dp) return -1;
    const int ku = num_edge_types - (skip_first ? 1 : 0);
    return ku < 1 ? 0 : ku;
}
}  // namespace

/* see include/aether_hip.h */
size_t aether_s2s_dynfield_plan_bytes(const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, int num_dims,
                                      int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                      int prior_hidden, int num_edge_types, int skip_first, int mlp_hidden) {
    const int ku = s2s_dynfield_ku(dp, mp, num_edge_types, skip_first);
    if (ku == 0 || mlp_hidden < 16 || mlp_hidden % 16 != 0) return 0;
    if (s2s_plan_size(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, ku) == 0)
        return 0;
    return S2SPlanLayout(num_dims, encoder_hidden, decoder_hidden, num_edge_types, rnn_hidden, prior_layers, prior_hidden, ku,
                         mlp_hidden).total;
}

int aether_s2s_dynfield_plan_build(const AetherS2SFilmParams* film, const AetherS2SPriorParams* pp,
                                   const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, int num_dims,
                                   int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                   int num_edge_types, int skip_first, int mlp_hidden, void* plan, size_t plan_bytes,
                                   void* stream) {
    const char* what = "s2s_dynfield_plan_build";
    if (!pp || !plan) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if ((dp != nullptr) == (mp != nullptr)) return s2s_fail(AETHER_EINVAL, what, "exactly one of the two decoders must be given");
    if (int rc = s2s_dynfield_film_check(what, film, mlp_hidden)) return rc;
    if (mp)
        if (int rc = s2s_markov_check(mp, num_dims, decoder_hidden, num_edge_types, skip_first)) return rc;
    const int D = num_dims, he = encoder_hidden, hd = decoder_hidden, K = num_edge_types, mh = mlp_hidden;
    const size_t need = aether_s2s_dynfield_plan_bytes(dp, mp, D, he, hd, rnn_hidden, prior_layers, prior_hidden, K, skip_first, mh);
    if (int rc = s2s_plan_buffer_check(what, need, plan, plan_bytes)) return rc;
    const S2SPlanLayout P(D, he, hd, K, rnn_hidden, prior_layers, prior_hidden, s2s_dynfield_ku(dp, mp, K, skip_first), mh);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)plan;
    s2s_plan_build_front(nullptr, pp, D, he, rnn_hidden, prior_layers, prior_hidden, P, base, st);
    // the FiLM net's two hidden layers, when the split GEMM can take them (mlp_hidden a multiple of 128); the layout has no
    // images otherwise and the jobs run on the fp32 MFMA job kernel
    s2s_image(base, st, P.i_film1, film->lin1_w, mh, he, he);
    s2s_image(base, st, P.i_film2, film->lin2_w, mh, mh, mh);
    if (dp) s2s_plan_build_recurrent(dp, D, hd, K, P, base, st);
    else s2s_plan_build_markov(mp, D, hd, K - (skip_first ? 1 : 0), P, base, st);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_dynfield_step_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden,
                                                int prior_hidden, int num_edge_types, int mlp_hidden, int64_t n_nodes,
                                                int64_t n_edges) {
    if (mlp_hidden < 16 || mlp_hidden % 16 != 0 ||
        aether_s2s_step_workspace_bytes(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden, num_edge_types, n_nodes,
                                        n_edges) == 0)
        return 0;
    return S2SStepLayout(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden, num_edge_types, n_nodes, n_edges,
                         mlp_hidden).total;
}

int aether_s2s_dynfield_step(const AetherS2SFilmParams* film, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                             const AetherS2SMarkovParams* mp, const void* plan, int num_dims, int encoder_hidden,
                             int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                             int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges, int mlp_hidden,
                             const float* mod, size_t mod_bytes, int64_t batch, int num_objects, const int64_t* send,
                             const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                             const float* ext_field, const float* decoder_hidden_in, const float* h0, const float* c0,
                             const float* uniform, void* workspace, size_t workspace_bytes, float* outputs,
                             float* decoder_hidden_out, float* h1, float* c1, float* edges_out, float* field_out, void* stream) {
    const char* what = "s2s_dynfield_step";
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    const S2SDynfieldArgs f{film, mlp_hidden, mod, mod_bytes, batch, num_objects};
    if (int rc = s2s_dynfield_entry_check(what, f, pp, dp, mp, plan, z,
                                          send && recv && order && rowptr && inputs && h0 && c0 && uniform && workspace && outputs &&
                                              h1 && c1 && (mp || (decoder_hidden_in && decoder_hidden_out)),
                                          0, 1)) return rc;
    if (field_out && ext_field) return s2s_fail(AETHER_EINVAL, what, "field_out is the built-in query's field: not with ext_field");
    const S2SStepArgs a = s2s_dynfield_step_args(f, pp, dp, mp, plan, z, send, recv, order, rowptr);
    if (int rc = s2s_run_step(what, a, workspace, workspace_bytes, {inputs, mp ? nullptr : decoder_hidden_in, h0, c0}, ext_field,
                              uniform, {outputs, mp ? nullptr : decoder_hidden_out, h1, c1}, edges_out, stream)) return rc;
    if (field_out)
        HIP_OK(hipMemcpyAsync(field_out, (const char*)workspace + a.L.field, (size_t)n_nodes * num_dims * sizeof(float),
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AETHER_OK;
}

int aether_s2s_dynfield_rollout(const AetherS2SFilmParams* film, const AetherS2SPriorParams* pp,
                                const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, const void* plan, int num_dims,
                                int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                                int64_t n_edges, int mlp_hidden, const float* mod, size_t mod_bytes, int64_t batch,
                                int num_objects, const int64_t* send, const int64_t* recv, const int64_t* order,
                                const int64_t* rowptr, int burn_in_steps, const float* burn_in, const float* burn_in_field,
                                int steps, const float* inputs,
                                float* decoder_state, float* h, float* c, const float* uniform, void* workspace,
                                size_t workspace_bytes, float* predictions, float* edges_out, void* stream) {
    const char* what = "s2s_dynfield_rollout";
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    const S2SDynfieldArgs f{film, mlp_hidden, mod, mod_bytes, batch, num_objects};
    if (int rc = s2s_dynfield_entry_check(what, f, pp, dp, mp, plan, z,
                                          send && recv && order && rowptr && inputs && h && c && uniform && workspace &&
                                              (mp || decoder_state) && (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                          burn_in_steps, steps)) return rc;
    return s2s_run_rollout(what, s2s_dynfield_step_args(f, pp, dp, mp, plan, z, send, recv, order, rowptr), workspace,
                           workspace_bytes, burn_in_steps, burn_in, steps, inputs, mp ? nullptr : decoder_state, h, c, uniform,
                           predictions, edges_out, stream, burn_in_field);
}
