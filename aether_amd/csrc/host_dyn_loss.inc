// Host side of the C ABI: the evaluation half of calculate_loss of the variable-N models (dyn_loss.h has the kernels) -- the
// sequence encoder over all frames as scenes of one prior stage, and the teacher-forced decoding loop of one sequence as one
// call.  Both are templates over the models of the scene engine (dyn_seq_run, dyn_loss_run), which supply their stages as
// they do for dyn_step_run / dyn_rollout_run.  Included by aether_hip.hip inside its extern "C" block, after
// host_dyn_dnri.inc; not a stand-alone source file.

namespace {
// Every frame has 2 <= n <= n_max present objects and the edge count of the encoder's own kNN graph.
int dyn_frames_check(const char* name, const AetherDynStepConfig* c, int F, int n_max, const int64_t* n_present,
                     const int64_t* n_edges, const int* in_degree, DynScenes* S, DynBatchSizes* Z) {
    if (!c || !n_present || !n_edges) return dyn_fail(AETHER_EINVAL, name, "null size array");
    if (F < 1 || F > DYN_MAX_SCENES) return dyn_fail(AETHER_EINVAL, name, "1..256 frames per call");
    if ((int64_t)F * n_max > (int64_t)1 << 24) return dyn_fail(AETHER_EINVAL, name, "too many object rows");
    Z->n_total = Z->e_total = Z->o_total = 0;
    S->n_scenes = F; S->n_max = n_max; S->knn_k = std::min(c->knn_k, n_max - 1);
    for (int t = 0; t < F; ++t) {
        const int64_t n = n_present[t];
        if (n < 2)
            return dyn_fail(AETHER_EINVAL, name, "a frame with fewer than two present objects (the reference's encoder drops such "
                                                 "a frame from the logits and its loss loop does not; the runner skips the sequence)");
        if (int rc = dyn_step_check(c, n_max, n, n_edges[t])) return rc;
        int deg = 0;
        if (in_degree) {
            deg = in_degree[t];
            if (deg < 1 || deg > 255 || (int64_t)deg * n > n_edges[t])
                return dyn_fail(AETHER_EINVAL, name, "edge2node of a step is [n_present][in_degree] edge ids, in_degree <= 255");
        }
        S->n[t] = (short)n; S->deg[t] = (unsigned char)deg;
        Z->n_total += n; Z->e_total += n_edges[t]; Z->o_total += n * deg;
    }
    if (Z->e_total > INT32_MAX / 64) return dyn_fail(AETHER_EINVAL, name, "too many edges");
    return AETHER_OK;
}

int dyn_posterior_check(const char* name, const AetherDynPosteriorParams* q, int layers, int hidden) {
    if (!q) return dyn_fail(AETHER_EINVAL, name, "null pointer");
    if (layers < 1 || layers > 4 || (layers > 1 && (hidden < 16 || hidden % 16 != 0)))
        return dyn_fail(AETHER_EINVAL, name, "1..4 encoder_fc_out layers, their hidden size a multiple of 16");
    for (int l = 0; l < layers; ++l)
        if (!q->w[l] || !q->b[l]) return dyn_fail(AETHER_EINVAL, name, "null encoder_fc_out weight");
    return AETHER_OK;
}
}  // namespace

extern "C++" {
namespace {
template <class Model>
size_t dyn_seq_bytes(const AetherDynStepConfig* config, int posterior_layers, int posterior_hidden, int F, int n_max,
                     const int64_t* n_present, const int64_t* n_edges) {
    DynScenes S; DynBatchSizes Z;
    if (dyn_frames_check(Model::seq_name, config, F, n_max, n_present, n_edges, nullptr, &S, &Z)) return 0;
    if (posterior_layers < 1 || posterior_layers > 4 || (posterior_layers > 1 && (posterior_hidden < 16 || posterior_hidden % 16 != 0))) {
        dyn_fail(AETHER_EINVAL, Model::seq_name, "1..4 encoder_fc_out layers, their hidden size a multiple of 16");
        return 0;
    }
    return DynSeqLayout(*config, F, n_max, Z, Model::seq_field_bytes(*config, Z), Model::seq_prior_bytes(*config, Z),
                        posterior_layers > 1 ? posterior_hidden : 0).total + 256;
}

// The sequence encoder over F frames as F scenes: present rows, (field), the encoder's kNN graphs and their receiver CSR, the
// model's feature transform, then the zero-state LSTM step and both heads.  A Model adds seq_name / loss_name,
// seq_field_bytes / seq_prior_bytes, seq_field(Q) and seq_prior(Q) to what dyn_step_run asks of it.
template <class Model>
int dyn_seq_run(const Model& M, const AetherDynPosteriorParams* posterior, const AetherDynStepConfig* config, int posterior_layers,
                int posterior_hidden, int F, int n_max, const int64_t* n_present, const int64_t* n_edges, const float* frames,
                const float* masks, float* prior_logits, float* posterior_logits, void* workspace, size_t workspace_bytes,
                void* stream) {
    const char* name = Model::seq_name;
    if (!M.seq_params_ok() || !posterior || !config || !frames || !masks || !prior_logits || !posterior_logits || !workspace)
        return dyn_fail(AETHER_EINVAL, name, "null pointer");
    DynScenes S; DynBatchSizes Z;
    if (int rc = dyn_frames_check(name, config, F, n_max, n_present, n_edges, nullptr, &S, &Z)) return rc;
    if (int rc = dyn_posterior_check(name, posterior, posterior_layers, posterior_hidden)) return rc;
    const AetherDynStepConfig& c = *config;
    if (int rc = M.config_check(name, c)) return rc;
    const DynSeqLayout L(c, F, n_max, Z, Model::seq_field_bytes(c, Z), Model::seq_prior_bytes(c, Z),
                         posterior_layers > 1 ? posterior_hidden : 0);
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    if (workspace_bytes < L.total + 256) return dyn_fail(AETHER_ESPACE, name, "workspace too small");
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    int* status = reinterpret_cast<int*>(ws + L.status);
    const NriSeqTail tail{posterior->w, posterior->b, posterior_layers, posterior_hidden, reinterpret_cast<float*>(ws + L.P1),
                          reinterpret_cast<float*>(ws + L.P2), posterior_logits, status};
    const DynSeqCtx Q{c, L, ws, stream, (int)Z.n_total, Z.e_total, tail, prior_logits};
    {   // the present rows of every frame (no decoder hidden rows: h = 0)
        const size_t lds = ((size_t)3 * (DYN_MAX_SCENES + 1) + 257 + 2 * (size_t)n_max) * 4;
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_dynb_present), lds)) return AETHER_EHIP;
        k_dynb_present<<<dim3((unsigned)F), dim3(256), lds, st>>>(S, frames, masks, nullptr, 0, Q.ip(L.idx),
                                                                 reinterpret_cast<int*>(ws + L.cidx), Q.fp(L.cur_in), Q.fp(L.cur_h),
                                                                 Q.ip(L.rowptr_dec), Q.fp(L.div_node), status, async_error_word(),
                                                                 Q.ip(L.ksums), reinterpret_cast<int*>(ws + L.counts));
    }
    if (int rc = M.seq_field(Q)) return rc;
    int64_t* ksums = Q.ip(L.ksums);
    if (int rc = knn_edges_impl(frames, 4, masks, F, n_max, L.knn_k, Q.ip(L.ksend), Q.ip(L.krecv), ksums, ksums + F, Q.ip(L.ktot),
                                ws + L.ws_knn, L.b_knn, stream, true)) return rc;
    {
        const size_t lds = ((size_t)3 * (DYN_MAX_SCENES + 1) + 257 + 256 + (size_t)n_max) * 4;
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_dynb_csr), lds)) return AETHER_EHIP;
        k_dynb_csr<<<dim3((unsigned)F), dim3(256), lds, st>>>(S, Q.ip(L.ksend), Q.ip(L.krecv), status, Q.ip(L.korder), Q.ip(L.krowptr));
    }
    if (int rc = M.seq_prior(Q)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// ------------------------------------------------------------------ the decoding loop of calculate_loss (:171-193 / :83-100)
template <class Layout>
size_t dyn_loss_bytes(const char* name, const AetherDynStepConfig* config, int n_max, int n_steps, const int64_t* n_present,
                      const int64_t* n_edges, const int* in_degree) {
    if (!config || !n_present || !n_edges || !in_degree || n_steps <= 0) { dyn_fail(AETHER_EINVAL, name, "bad sizes"); return 0; }
    size_t need = 0;
    for (int t = 0; t < n_steps; ++t) {
        DynScenes S; DynBatchSizes Z;
        if (dyn_frames_check(name, config, 1, n_max, n_present + t, n_edges + t, in_degree + t, &S, &Z)) return 0;
        need = std::max(need, Layout(*config, 1, n_max, Z).total + 256);
    }
    return need + align_up((size_t)n_max * config->decoder_hidden * 4, 256) + 256;
}

// For step t the state is inputs[t] when teacher-forced or t == 0, else predictions[t - 1]; the model's field at its present
// rows; the hard Gumbel sample of logits[offset of t] with uniform[t]; the decoder step on the data set's graph of the step.
// No prior stage, no LSTM slots, no kNN.  A Model adds loss_graph(X) and decode(X, edge types, false) -- the decoder computes
// its own node frames: no prior workspace was filled.
template <class Model>
int dyn_loss_run(const Model& M, const AetherDynStepConfig* config, int n_max, int n_steps, int teacher_forcing_steps,
                 const float* inputs, const float* masks, const int64_t* n_present, const int64_t* n_edges, const int* in_degree,
                 const int64_t* const* graph_send, const int64_t* const* graph_recv, const int64_t* const* edge2node,
                 const float* logits, const float* const* uniform, float* predictions, float* edge_types, void* workspace,
                 size_t workspace_bytes, void* stream) {
    const char* name = Model::loss_name;
    if (!M.loss_params_ok() || !config || !inputs || !masks || !n_present || !n_edges || !in_degree || !graph_send || !graph_recv ||
        !edge2node || !logits || !uniform || !predictions || !workspace)
        return dyn_fail(AETHER_EINVAL, name, "null pointer");
    if (n_steps <= 0) return dyn_fail(AETHER_EINVAL, name, "n_steps must be positive");
    if (teacher_forcing_steps < -1) return dyn_fail(AETHER_EINVAL, name, "teacher_forcing_steps is -1 (always) or a step count");
    // every step is validated on the host before anything is queued
    for (int t = 0; t < n_steps; ++t) {
        DynScenes S; DynBatchSizes Z;
        if (int rc = dyn_frames_check(name, config, 1, n_max, n_present + t, n_edges + t, in_degree + t, &S, &Z)) return rc;
        if (!graph_send[t] || !graph_recv[t] || !edge2node[t] || !uniform[t])
            return dyn_fail(AETHER_EINVAL, name, "a step's graph / uniform pointer is null");
    }
    const AetherDynStepConfig& c = *config;
    if (int rc = M.config_check(name, c)) return rc;
    const size_t need = dyn_loss_bytes<typename Model::Layout>(name, config, n_max, n_steps, n_present, n_edges, in_degree);
    if (need == 0) return AETHER_EINVAL;
    if (workspace_bytes < need) return dyn_fail(AETHER_ESPACE, name, "workspace too small");
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    float* decoder_hidden = reinterpret_cast<float*>(base);                  // [n_max][hd], get_initial_hidden: zeros
    const size_t hidden_bytes = (size_t)n_max * c.decoder_hidden * 4;
    char* ws = base + align_up(hidden_bytes, 256);
    HIP_OK(hipMemsetAsync(decoder_hidden, 0, hidden_bytes, st));
    const size_t row = (size_t)n_max * 4;
    int64_t edge0 = 0;
    for (int t = 0; t < n_steps; ++t) {
        DynScenes S; DynBatchSizes Z;
        dyn_frames_check(name, config, 1, n_max, n_present + t, n_edges + t, in_degree + t, &S, &Z);
        const bool teacher = t == 0 || teacher_forcing_steps < 0 || t < teacher_forcing_steps;
        const float* state = teacher ? inputs + (size_t)t * row : predictions + (size_t)(t - 1) * row;
        const float* mask = masks + (size_t)t * n_max;
        float* prediction = predictions + (size_t)t * row;
        const typename Model::Layout L(c, 1, n_max, Z);
        const DynStepCtx<typename Model::Layout> X{c, S, Z, L, ws, stream, (int)Z.n_total, Z.e_total, (int64_t)n_max, state, nullptr,
                                                   graph_send[t], graph_recv[t], edge2node[t], nullptr, nullptr, decoder_hidden,
                                                   prediction};
        {
            const size_t lds = ((size_t)3 * (DYN_MAX_SCENES + 1) + 257 + 2 * (size_t)n_max) * 4;
            if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_dynb_present), lds)) return AETHER_EHIP;
            k_dynb_present<<<dim3(1), dim3(256), lds, st>>>(S, state, mask, decoder_hidden, c.decoder_hidden, X.ip(L.idx), X.cidx(),
                                                           X.fp(L.cur_in), X.fp(L.cur_h), X.ip(L.rowptr_dec), X.fp(L.div_node),
                                                           X.status(), async_error_word(), X.ip(L.ksums),
                                                           reinterpret_cast<int*>(ws + M.counts_offset(X)));
        }
        if (int rc = M.field(X)) return rc;
        M.loss_graph(X);
        float* ew = (t + 1 == n_steps && edge_types) ? edge_types : X.fp(L.ew);
        // the sample alone: no LSTM rows go back into slots (R = 0: the scatter half of the kernel has no work)
        k_dyn_scatter_sample<<<dyn_blocks(X.E), dim3(256), 0, st>>>(nullptr, nullptr, nullptr, X.E, 0, nullptr, nullptr,
                                                                   logits + (size_t)edge0 * c.num_edge_types, uniform[t],
                                                                   c.gumbel_tau, c.num_edge_types, ew, nullptr, 0);
        if (int rc = M.decode(X, ew, false)) return rc;
        edge0 += n_edges[t];
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
}  // namespace
}  // extern "C++"

/* see include/aether_hip.h */
size_t aether_dyn_sequence_logits_workspace_bytes(const AetherDynStepConfig* config, int posterior_layers, int posterior_hidden,
                                                  int n_frames, int n_objects_max, const int64_t* n_present,
                                                  const int64_t* n_edges) {
    return dyn_seq_bytes<DynAetherModel>(config, posterior_layers, posterior_hidden, n_frames, n_objects_max, n_present, n_edges);
}

int aether_dyn_sequence_logits(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                               const AetherDynPosteriorParams* posterior_params, const AetherDynStepConfig* config,
                               int posterior_layers, int posterior_hidden, int n_frames, int n_objects_max,
                               const int64_t* n_present, const int64_t* n_edges, const float* frames, const float* masks,
                               float* prior_logits, float* posterior_logits, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return dyn_seq_run(DynAetherModel{field_params, prior_params, nullptr}, posterior_params,
                       config, posterior_layers, posterior_hidden, n_frames, n_objects_max, n_present, n_edges, frames, masks,
                       prior_logits, posterior_logits, workspace, workspace_bytes, stream);
}

size_t aether_dyn_dnri_sequence_logits_workspace_bytes(const AetherDynStepConfig* config, int posterior_layers,
                                                       int posterior_hidden, int n_frames, int n_objects_max,
                                                       const int64_t* n_present, const int64_t* n_edges) {
    return dyn_seq_bytes<DynDnriModel>(config, posterior_layers, posterior_hidden, n_frames, n_objects_max, n_present, n_edges);
}

int aether_dyn_dnri_sequence_logits(const AetherDynDnriPriorParams* prior_params, const AetherDynPosteriorParams* posterior_params,
                                    const AetherDynStepConfig* config, int posterior_layers, int posterior_hidden, int n_frames,
                                    int n_objects_max, const int64_t* n_present, const int64_t* n_edges, const float* frames,
                                    const float* masks, float* prior_logits, float* posterior_logits, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return dyn_seq_run(DynDnriModel{prior_params, nullptr}, posterior_params, config,
                       posterior_layers, posterior_hidden, n_frames, n_objects_max, n_present, n_edges, frames, masks, prior_logits,
                       posterior_logits, workspace, workspace_bytes, stream);
}

size_t aether_dyn_loss_rollout_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int n_steps,
                                               const int64_t* n_present, const int64_t* n_edges, const int* in_degree) {
    return dyn_loss_bytes<DynBatchLayout>(DynAetherModel::loss_name, config, n_objects_max, n_steps, n_present, n_edges, in_degree);
}

int aether_dyn_loss_rollout(const AetherDynFieldQueryParams* field_params, const AetherDynDecoderParams* decoder_params,
                            const AetherDynStepConfig* config, int n_objects_max, int n_steps, int teacher_forcing_steps,
                            const float* inputs, const float* masks, const int64_t* n_present, const int64_t* n_edges,
                            const int* in_degree, const int64_t* const* graph_send, const int64_t* const* graph_recv,
                            const int64_t* const* edge2node, const float* logits, const float* const* uniform,
                            float* predictions, float* edge_types, void* workspace, size_t workspace_bytes, void* stream) {
    return dyn_loss_run(DynAetherModel{field_params, nullptr, decoder_params}, config,
                        n_objects_max, n_steps, teacher_forcing_steps, inputs, masks, n_present, n_edges, in_degree, graph_send,
                        graph_recv, edge2node, logits, uniform, predictions, edge_types, workspace, workspace_bytes, stream);
}

size_t aether_dyn_dnri_loss_rollout_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int n_steps,
                                                    const int64_t* n_present, const int64_t* n_edges, const int* in_degree) {
    return dyn_loss_bytes<DynDnriBatchLayout>(DynDnriModel::loss_name, config, n_objects_max, n_steps, n_present, n_edges,
                                              in_degree);
}

int aether_dyn_dnri_loss_rollout(const AetherDynDnriDecoderParams* decoder_params, const AetherDynStepConfig* config,
                                 int n_objects_max, int n_steps, int teacher_forcing_steps, const float* inputs,
                                 const float* masks, const int64_t* n_present, const int64_t* n_edges, const int* in_degree,
                                 const int64_t* const* graph_send, const int64_t* const* graph_recv,
                                 const int64_t* const* edge2node, const float* logits, const float* const* uniform,
                                 float* predictions, float* edge_types, void* workspace, size_t workspace_bytes, void* stream) {
    return dyn_loss_run(DynDnriModel{nullptr, decoder_params}, config, n_objects_max,
                        n_steps, teacher_forcing_steps, inputs, masks, n_present, n_edges, in_degree, graph_send, graph_recv,
                        edge2node, logits, uniform, predictions, edge_types, workspace, workspace_bytes, stream);
}
