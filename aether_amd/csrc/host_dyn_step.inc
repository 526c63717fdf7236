// Host side of the C ABI: one prediction step of the variable-N model, and the whole prediction loop, as ONE call for
// 1 .. 256 scenes (SURVEY 8f N2; dyn_step.h has the kernels).  Included by aether_hip.hip inside its extern "C" block,
// after host_dynamicvars.inc.  The step and rollout drivers are templates over a model (dyn_step_run, dyn_rollout_run):
// DynAetherModel here, DynDnriModel in host_dyn_dnri.inc.  aether_dyn_step / aether_dyn_rollout (one scene) are the
// n_scenes = 1 case of the batched entry points and forward to them (end of this file).

namespace {
// One scene of a step: the configuration, and 2 <= n <= n_max present objects with the edge count of the encoder's kNN graph.
int dyn_step_check(const AetherDynStepConfig* c, int n_max, int64_t n, int64_t E) {
    if (!c) return fail(AETHER_EINVAL, "dyn_step: null config");
    if (n_max < 2 || n_max > DYN_MAX_OBJECTS) return fail(AETHER_EINVAL, "dyn_step: 2..8192 object rows");
    if (n < 2 || n > n_max) return fail(AETHER_EINVAL, "dyn_step: a step needs 2..n_objects_max present objects");
    if (c->knn_k < 1 || c->knn_k > KNN_MAX_K) return fail(AETHER_EINVAL, "dyn_step: knn_k must be in 1..16");
    if (c->rnn_hidden < 16 || c->rnn_hidden % 16 != 0) return fail(AETHER_EINVAL, "dyn_step: rnn_hidden must be a multiple of 16");
    if (c->decoder_hidden < 128 || c->decoder_hidden % 128 != 0 || c->encoder_hidden < 128 || c->encoder_hidden % 128 != 0)
        return fail(AETHER_EINVAL, "dyn_step: encoder / decoder hidden must be multiples of 128");
    if (c->num_edge_types < 1 || c->num_edge_types > 4) return fail(AETHER_EINVAL, "dyn_step: 1..4 edge types");
    if (!(c->gumbel_tau > 0.0f)) return fail(AETHER_EINVAL, "dyn_step: gumbel_tau must be positive");
    // the encoder's own kNN graph has n * min(k, n - 1) edges; the caller's graph must list as many (the module raises
    // "graph_info and the encoder's kNN graph list a different number of edges" for the same reason)
    const int64_t k = std::min<int64_t>(std::min(c->knn_k, n_max - 1), n - 1);
    if (E != n * k)
        return fail(AETHER_EINVAL, "dyn_step: n_edges must be n_present * min(knn_k, n_present - 1), the size of the encoder's "
                                   "own kNN graph");
    return AETHER_OK;
}

struct DynBatchSizes { int64_t n_total, e_total, o_total; };
// The buffers of a step that every model on the scene engine uses.  A model's layout derives from this one and takes its own
// buffers behind these.  Every take starts 256-aligned and is rounded to 256 bytes, so `total` is the sum of the rounded
// sizes whatever the order of the takes.
struct DynSceneLayout {
    size_t idx, cidx, cur_in, cur_h, rowptr_dec, div_node, status, ksend, krecv, ksums, ktot, korder, krowptr, send, recv, order,
        slot, h0, c0, h1, c1, logits, ew, new_h, ws_knn, total = 0;
    size_t b_knn;
    int knn_k;
    size_t take(size_t bytes) { size_t o = total; total = align_up(total + bytes, 256); return o; }
    DynSceneLayout(const AetherDynStepConfig& c, int B, int n_max, const DynBatchSizes& Z) {
        const size_t nn = (size_t)Z.n_total, ee = (size_t)Z.e_total, oo = (size_t)Z.o_total, R = (size_t)c.rnn_hidden,
                     K = (size_t)c.num_edge_types, rows = (size_t)B * n_max;
        knn_k = std::min(c.knn_k, n_max - 1);
        idx = take(nn * 8); cidx = take(rows * 4); cur_in = take(nn * 16); cur_h = take(nn * c.decoder_hidden * 4);
        rowptr_dec = take((nn + 1) * 8); div_node = take(nn * 4); status = take((size_t)(1 + DYN_MAX_SCENES) * 4);
        const size_t kcap = std::max(ee, rows * (size_t)(knn_k > 0 ? knn_k : 1));      // whatever the masks hold
        ksend = take(kcap * 8); krecv = take(kcap * 8); ksums = take((size_t)2 * B * 8); ktot = take(64);
        korder = take(ee * 8); krowptr = take((nn + 1) * 8);
        send = take(ee * 8); recv = take(ee * 8); order = take((oo + 1) * 8); slot = take(ee * 8);
        h0 = take(ee * R * 4); c0 = take(ee * R * 4); h1 = take(ee * R * 4); c1 = take(ee * R * 4);
        logits = take(ee * K * 4); ew = take(ee * K * 4); new_h = take(nn * c.decoder_hidden * 4);
        b_knn = aether_knn_workspace_bytes(B, n_max, knn_k > 0 ? knn_k : 1);
        ws_knn = take(b_knn);
    }
};
struct DynBatchLayout : DynSceneLayout {
    size_t field_c, ext_full, ssend, srecv, out_c, ws_field, ws_prior, ws_dec;
    size_t b_field, b_prior, b_dec;
    DynBatchLayout(const AetherDynStepConfig& c, int B, int n_max, const DynBatchSizes& Z) : DynSceneLayout(c, B, n_max, Z) {
        const size_t nn = (size_t)Z.n_total, ee = (size_t)Z.e_total;
        field_c = take(nn * 8); ext_full = take((size_t)B * n_max * 24); ssend = take(ee * 8); srecv = take(ee * 8);
        out_c = take(nn * 16);
        b_field = aether_dyn_field_workspace_bytes(Z.n_total, c.field_hidden);
        b_prior = aether_dyn_prior_workspace_bytes(c.encoder_hidden, c.rnn_hidden, c.prior_hidden, Z.n_total, Z.e_total);
        b_dec = aether_dyn_decoder_workspace_bytes(c.decoder_hidden, Z.n_total, Z.e_total);
        ws_field = take(b_field); ws_prior = take(b_prior); ws_dec = take(b_dec);
    }
};

// The sequence encoder's buffers: the scene bookkeeping of a step, the field at the present rows and the model's prior
// workspace (sizes from the model), the posterior head's hidden rows and the decoder-count words k_dynb_present clears.
struct DynSeqLayout : DynSceneLayout {
    size_t field_c, ws_field, ws_prior, P1, P2, counts;
    size_t b_field, b_prior;
    DynSeqLayout(const AetherDynStepConfig& c, int F, int n_max, const DynBatchSizes& Z, size_t field_bytes, size_t prior_bytes,
                 int post_hidden)
        : DynSceneLayout(c, F, n_max, Z), b_field(field_bytes), b_prior(prior_bytes) {
        const size_t nn = (size_t)Z.n_total, ee = (size_t)Z.e_total, ph = (size_t)(post_hidden > 0 ? post_hidden : 1);
        field_c = take(nn * 8); ws_field = take(b_field); ws_prior = take(b_prior);
        P1 = take(ee * ph * 4); P2 = take(ee * ph * 4); counts = take(64 * 4);
    }
};

// (host_dyn_loss.inc) What a model's stages of the sequence encoder see
struct DynSeqCtx {
    const AetherDynStepConfig& c; const DynSeqLayout& L; char* ws; void* stream; int n; int64_t E;
    const NriSeqTail& tail; float* prior_logits;
    float* fp(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    int64_t* ip(size_t off) const { return reinterpret_cast<int64_t*>(ws + off); }
};

// Every scene is empty (n = 0) or passes dyn_step_check; fills the by-value scene table and the totals.
int dyn_batch_check(const AetherDynStepConfig* c, int B, int n_max, const int64_t* n_present, const int64_t* n_edges,
                    const int* in_degree, DynScenes* S, DynBatchSizes* Z) {
    if (!c || !n_present || !n_edges || !in_degree) return fail(AETHER_EINVAL, "dyn_step_batched: null size array");
    if (B < 1 || B > DYN_MAX_SCENES) return fail(AETHER_EINVAL, "dyn_step_batched: 1..256 scenes per call");
    if ((int64_t)B * n_max > (int64_t)1 << 24) return fail(AETHER_EINVAL, "dyn_step_batched: too many object rows");
    Z->n_total = Z->e_total = Z->o_total = 0;
    S->n_scenes = B; S->n_max = n_max; S->knn_k = std::min(c->knn_k, n_max - 1);
    bool checked = false;
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_present[b];
        S->n[b] = 0; S->deg[b] = 0;
        if (n == 0) {
            if (n_edges[b] != 0) return fail(AETHER_EINVAL, "dyn_step_batched: an empty scene lists edges");
            continue;
        }
        if (n == 1)
            return fail(AETHER_EINVAL, "dyn_step_batched: a scene with one present object (the reference fails there as well, "
                                       "aether_dynamicvars.py:843-851)");
        if (int rc = dyn_step_check(c, n_max, n, n_edges[b])) return rc;
        checked = true;
        if (in_degree[b] < 1 || in_degree[b] > 255 || (int64_t)in_degree[b] * n > n_edges[b])
            return fail(AETHER_EINVAL, "dyn_step_batched: edge2node of a scene is [n_present][in_degree] edge ids, in_degree <= 255");
        S->n[b] = (short)n; S->deg[b] = (unsigned char)in_degree[b];
        Z->n_total += n; Z->e_total += n_edges[b]; Z->o_total += n * in_degree[b];
    }
    if (!checked) {       // all scenes empty: the configuration itself has not been looked at yet
        if (n_max < 2 || n_max > DYN_MAX_OBJECTS) return fail(AETHER_EINVAL, "dyn_step_batched: 2..8192 object rows");
    }
    if (Z->e_total > INT32_MAX / 64) return fail(AETHER_EINVAL, "dyn_step_batched: too many edges");
    return AETHER_OK;
}

int dyn_fail(int code, const char* entry, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, what);
    return code;
}
}  // namespace

extern "C++" {
namespace {
dim3 dyn_blocks(int64_t cnt) { return dim3((unsigned)((cnt + 255) / 256)); }
// What a model's own launches of a step see: the checked sizes, the carved workspace and the caller's arrays.
template <class Layout>
struct DynStepCtx {
    const AetherDynStepConfig& c; const DynScenes& S; const DynBatchSizes& Z; const Layout& L;
    char* ws; void* stream;
    int n; int64_t E, rows;                      // present objects and edges of all scenes; n_scenes * n_objects_max
    const float* state; const int64_t *node_inds, *graph_send, *graph_recv, *edge2node;
    float *prior_h, *prior_c, *decoder_hidden, *prediction;
    hipStream_t st() const { return (hipStream_t)stream; }
    float* fp(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    int64_t* ip(size_t off) const { return reinterpret_cast<int64_t*>(ws + off); }
    int* cidx() const { return reinterpret_cast<int*>(ws + L.cidx); }
    int* status() const { return reinterpret_cast<int*>(ws + L.status); }
};
template <class Layout>
size_t dyn_step_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max, const int64_t* n_present,
                      const int64_t* n_edges, const int* in_degree) {
    DynScenes S; DynBatchSizes Z;
    if (dyn_batch_check(config, n_scenes, n_objects_max, n_present, n_edges, in_degree, &S, &Z)) return 0;
    if (Z.n_total == 0) return 512;
    return Layout(*config, n_scenes, n_objects_max, Z).total + 256;
}

// One prediction step of 1 .. 256 scenes.  The driver owns the refusals, the all-empty case, the workspace, the scene
// bookkeeping (present objects, the encoder's kNN graphs by receiver) and the sample; a Model supplies
//   Layout (a DynSceneLayout), step_name / rollout_name (the entries' names in messages), params_ok(),
//   config_check(entry, c), counts_offset(X) (where its decoder's `counts` words lie in the workspace),
//   field(X) (launches between the present rows and the kNN graphs), index(X), prior(X), decode(X, edge types).
template <class Model>
int dyn_step_run(const Model& M, const AetherDynStepConfig* config, int B, int n_max, const int64_t* n_present,
                 const int64_t* n_edges, const int* in_degree, const float* state, const float* mask, const int64_t* node_inds,
                 const int64_t* graph_send, const int64_t* graph_recv, const int64_t* edge2node, float* prior_h, float* prior_c,
                 float* decoder_hidden, const float* uniform, float* prediction, float* edge_types, void* workspace,
                 size_t workspace_bytes, void* stream) {
    const char* name = Model::step_name;
    if (!M.params_ok() || !state || !mask || !prior_h || !prior_c || !decoder_hidden || !prediction || !workspace)
        return dyn_fail(AETHER_EINVAL, name, "null pointer");
    DynScenes S; DynBatchSizes Z;
    if (int rc = dyn_batch_check(config, B, n_max, n_present, n_edges, in_degree, &S, &Z)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const AetherDynStepConfig& c = *config;
    const int64_t rows = (int64_t)B * n_max;
    if (Z.n_total == 0) {                        // nobody anywhere: zeros, states untouched
        HIP_OK(hipMemsetAsync(prediction, 0, (size_t)rows * 16, st));
        return AETHER_OK;
    }
    if (!graph_send || !graph_recv || !edge2node || !uniform) return dyn_fail(AETHER_EINVAL, name, "null graph / uniform pointer");
    if (int rc = M.config_check(name, c)) return rc;
    const typename Model::Layout L(c, B, n_max, Z);
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    if (workspace_bytes < L.total + 256) return dyn_fail(AETHER_ESPACE, name, "workspace too small");
    if (take_async_error()) return AETHER_EHIP;
    const DynStepCtx<typename Model::Layout> X{c, S, Z, L, ws, stream, (int)Z.n_total, Z.e_total, rows, state, node_inds,
                                               graph_send, graph_recv, edge2node, prior_h, prior_c, decoder_hidden, prediction};
    const int R = c.rnn_hidden;
    // ---- the present objects of every scene (mask -> rows), their state and decoder hidden rows
    {
        const size_t lds = ((size_t)3 * (DYN_MAX_SCENES + 1) + 257 + 2 * (size_t)n_max) * 4;
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_dynb_present), lds)) return AETHER_EHIP;
        k_dynb_present<<<dim3((unsigned)B), dim3(256), lds, st>>>(S, state, mask, decoder_hidden, c.decoder_hidden, X.ip(L.idx),
                                                                 X.cidx(), X.fp(L.cur_in), X.fp(L.cur_h), X.ip(L.rowptr_dec),
                                                                 X.fp(L.div_node), X.status(), async_error_word(), X.ip(L.ksums),
                                                                 reinterpret_cast<int*>(ws + M.counts_offset(X)));
    }
    if (int rc = M.field(X)) return rc;
    // ---- the encoder's own kNN graphs, scene by scene, then grouped by receiver per scene
    int64_t* ksums = X.ip(L.ksums);
    if (int rc = knn_edges_impl(state, 4, mask, B, n_max, L.knn_k, X.ip(L.ksend), X.ip(L.krecv), ksums, ksums + B, X.ip(L.ktot),
                                ws + L.ws_knn, L.b_knn, stream, true)) return rc;
    {
        const size_t lds = ((size_t)3 * (DYN_MAX_SCENES + 1) + 257 + 256 + (size_t)n_max) * 4;
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_dynb_csr), lds)) return AETHER_EHIP;
        k_dynb_csr<<<dim3((unsigned)B), dim3(256), lds, st>>>(S, X.ip(L.ksend), X.ip(L.krecv), X.status(), X.ip(L.korder),
                                                             X.ip(L.krowptr));
    }
    // ---- the callers' graphs in the numbering of the batch and the LSTM state rows of their edges; the prior step
    M.index(X);
    if (int rc = M.prior(X)) return rc;
    // ... state back into its slots and the hard Gumbel sample of the edge types, one launch; a scene whose mask disagreed with
    // its n poisons the rows (status[0] != 0)
    float* ew = edge_types ? edge_types : X.fp(L.ew);
    k_dyn_scatter_sample<<<dyn_blocks(X.E * (R / 4)), dim3(256), 0, st>>>(X.ip(L.slot), X.fp(L.h1), X.fp(L.c1), X.E, R, prior_h,
                                                                         prior_c, X.fp(L.logits), uniform, c.gumbel_tau,
                                                                         c.num_edge_types, ew, X.status(), 0);
    // ---- decoder step on the callers' graphs, rows back to their objects
    if (int rc = M.decode(X, ew)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// ------------------------------------------------------------------ the prediction loop (predict_future)
// Per step the burn-in mix and the model's step, queued without a host round trip.  Every per-step array is TIME-MAJOR -- inputs
// [n_steps + 1][B][n_max][4], masks / burn_in_masks [n_steps][B][n_max], predictions [n_steps][B][n_max][4] -- and the host
// size arrays [n_steps][B].
template <class Layout>
size_t dyn_rollout_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max, int n_steps, const int64_t* n_present,
                         const int64_t* n_edges, const int* in_degree) {
    if (!config || !n_present || !n_edges || !in_degree || n_steps <= 0 || n_scenes < 1) return 0;
    size_t need = 0;
    for (int t = 0; t < n_steps; ++t) {
        const size_t b = dyn_step_bytes<Layout>(config, n_scenes, n_objects_max, n_present + (size_t)t * n_scenes,
                                                n_edges + (size_t)t * n_scenes, in_degree + (size_t)t * n_scenes);
        if (b == 0) return 0;
        need = std::max(need, b);
    }
    return need + align_up((size_t)n_scenes * n_objects_max * 16, 256) + 256;
}

template <class Model>
int dyn_rollout_run(const Model& M, const AetherDynStepConfig* config, int B, int n_objects_max, int n_steps, const float* inputs,
                    const float* masks, const float* burn_in_masks, const int64_t* n_present, const int64_t* n_edges,
                    const int* in_degree, const int64_t* const* node_inds, const int64_t* const* graph_send,
                    const int64_t* const* graph_recv, const int64_t* const* edge2node, const float* const* uniform, float* prior_h,
                    float* prior_c, float* decoder_hidden, float* predictions, void* workspace, size_t workspace_bytes,
                    void* stream) {
    const char* name = Model::rollout_name;
    if (!config || !inputs || !masks || !burn_in_masks || !n_present || !n_edges || !in_degree || !graph_send || !graph_recv ||
        !edge2node || !uniform || !predictions || !workspace || !M.params_ok() || !prior_h || !prior_c || !decoder_hidden)
        return dyn_fail(AETHER_EINVAL, name, "null pointer");
    if (n_steps <= 0) return dyn_fail(AETHER_EINVAL, name, "n_steps must be positive");
    // every step of every scene is validated on the host before anything is queued
    for (int t = 0; t < n_steps; ++t) {
        DynScenes S; DynBatchSizes Z;
        if (int rc = dyn_batch_check(config, B, n_objects_max, n_present + (size_t)t * B, n_edges + (size_t)t * B,
                                     in_degree + (size_t)t * B, &S, &Z)) return rc;
        if (Z.n_total > 0 && (!graph_send[t] || !graph_recv[t] || !edge2node[t] || !uniform[t]))
            return dyn_fail(AETHER_EINVAL, name, "a step's graph / uniform pointer is null");
    }
    if (int rc = M.config_check(name, *config)) return rc;
    const size_t need = dyn_rollout_bytes<typename Model::Layout>(config, B, n_objects_max, n_steps, n_present, n_edges, in_degree);
    if (need == 0) return dyn_fail(AETHER_EINVAL, name, "bad sizes");
    if (workspace_bytes < need) return dyn_fail(AETHER_ESPACE, name, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(align_up((size_t)workspace, 256));
    float* state = reinterpret_cast<float*>(ws);
    const size_t rows = (size_t)B * n_objects_max;
    char* step_ws = ws + align_up(rows * 16, 256);
    const size_t step_bytes = workspace_bytes - (size_t)(step_ws - (char*)workspace);
    const size_t row = rows * 4;
    for (int t = 0; t < n_steps; ++t) {
        const float* last = t == 0 ? inputs : predictions + (size_t)(t - 1) * row;
        k_dyn_mix<<<dyn_blocks((int64_t)row), dim3(256), 0, st>>>(inputs + (size_t)t * row, last, burn_in_masks + (size_t)t * rows,
                                                                 (int)rows, state);
        if (int rc = dyn_step_run(M, config, B, n_objects_max, n_present + (size_t)t * B, n_edges + (size_t)t * B,
                                  in_degree + (size_t)t * B, state, masks + (size_t)t * rows, node_inds ? node_inds[t] : nullptr,
                                  graph_send[t], graph_recv[t], edge2node[t], prior_h, prior_c, decoder_hidden, uniform[t],
                                  predictions + (size_t)t * row, nullptr, step_ws, step_bytes, stream)) return rc;
    }
    return AETHER_OK;
}

// AetherDynamicVars on the driver: present, field, kNN, csr, index, prior, sample, decoder, finish.
struct DynAetherModel {
    using Layout = DynBatchLayout;
    using Ctx = DynStepCtx<Layout>;
    static constexpr const char* step_name = "dyn_step_batched";
    static constexpr const char* rollout_name = "dyn_rollout_batched";
    const AetherDynFieldQueryParams* field_params;
    const AetherDynPriorParams* prior_params;
    const AetherDynDecoderParams* decoder_params;
    bool params_ok() const { return field_params && prior_params && decoder_params; }
    int config_check(const char*, const AetherDynStepConfig&) const { return AETHER_OK; }   // (the stages check what they read)
    size_t counts_offset(const Ctx& X) const { return X.L.ws_dec + DynDecLayout(X.c.decoder_hidden, X.n, X.E).counts; }
    // field at the present objects (:64-79)
    int field(const Ctx& X) const {
        return aether_dyn_field(field_params, X.c.field_hidden, X.n, X.fp(X.L.cur_in), X.ws + X.L.ws_field, X.L.b_field,
                                X.fp(X.L.field_c), X.stream);
    }
    // the callers' graphs in the numbering of the batch, LSTM state rows of their edges (:680-694), ext_full (:823)
    void index(const Ctx& X) const {
        const Layout& L = X.L;
        const int R = X.c.rnn_hidden;
        const int64_t work = std::max<int64_t>(std::max<int64_t>(X.E * (R / 4), X.rows * 6), X.Z.o_total);
        k_dynb_index<<<dyn_blocks(work), dim3(256), 0, X.st()>>>(X.S, X.graph_send, X.graph_recv, X.node_inds, X.ip(L.idx),
                                                                X.edge2node, R, X.prior_h, X.prior_c, X.ip(L.send), X.ip(L.recv),
                                                                X.ip(L.ssend), X.ip(L.srecv), X.ip(L.slot), X.fp(L.h0), X.fp(L.c0),
                                                                X.ip(L.order), X.state, X.fp(L.field_c), X.cidx(), X.fp(L.ext_full));
    }
    int prior(const Ctx& X) const {
        const Layout& L = X.L;
        const AetherDynStepConfig& c = X.c;
        return aether_dyn_prior_step(prior_params, c.encoder_hidden, c.rnn_hidden, c.prior_layers, c.prior_hidden, c.num_edge_types,
                                     c.encoder_polar, X.n, X.E, X.fp(L.cur_in), X.fp(L.field_c), X.fp(L.h0), X.fp(L.c0),
                                     X.ip(L.ksend), X.ip(L.krecv), X.ip(L.korder), X.ip(L.krowptr), X.ws + L.ws_prior, L.b_prior,
                                     X.fp(L.logits), X.fp(L.h1), X.fp(L.c1), X.stream);
    }
    // decoder step on the callers' graphs (:775-870), rows back to their objects.  prior_nodes: the prior step of the same
    // call has the canonical states and frames of these rows in its workspace (false: the decoder computes its own)
    int decode(const Ctx& X, const float* ew, bool prior_nodes = true) const {
        const Layout& L = X.L;
        const AetherDynStepConfig& c = X.c;
        const int hd = c.decoder_hidden;
        const DynPriorLayout PL(c.encoder_hidden, c.rnn_hidden, c.prior_hidden, X.n, X.E);
        DynSharedNodes shared{reinterpret_cast<const float*>(X.ws + L.ws_prior + PL.ext),
                              reinterpret_cast<const float*>(X.ws + L.ws_prior + PL.rel),
                              reinterpret_cast<const float*>(X.ws + L.ws_prior + PL.Rinv), true};
        if (!prior_nodes) shared.ext = shared.rel = shared.Rinv = nullptr;
        if (int rc = dyn_decoder_impl(decoder_params, hd, c.num_edge_types, c.skip_first, c.decoder_polar, X.n, X.E, X.fp(L.cur_in),
                                      X.fp(L.cur_h), ew, X.fp(L.field_c), X.fp(L.ext_full), X.ip(L.ssend), X.ip(L.srecv),
                                      X.ip(L.send), X.ip(L.recv), X.ip(L.order), X.ip(L.rowptr_dec), 1.0f, X.fp(L.div_node),
                                      X.ws + L.ws_dec, L.b_dec, X.fp(L.out_c), X.fp(L.new_h), X.st(), &shared)) return rc;
        const int64_t work = std::max<int64_t>(X.rows * 4, (int64_t)X.n * (hd / 4));
        k_dynb_finish<<<dyn_blocks(work), dim3(256), 0, X.st()>>>(X.fp(L.out_c), X.fp(L.new_h), X.cidx(), X.ip(L.idx), X.status(),
                                                                 X.rows, X.n, hd, X.prediction, X.decoder_hidden);
        return AETHER_OK;
    }
    // ---- the evaluation half of calculate_loss (host_dyn_loss.inc: dyn_seq_run, dyn_loss_run)
    static constexpr const char* seq_name = "dyn_sequence_logits";
    static constexpr const char* loss_name = "dyn_loss_rollout";
    bool seq_params_ok() const { return field_params && prior_params; }
    bool loss_params_ok() const { return field_params && decoder_params; }
    static size_t seq_field_bytes(const AetherDynStepConfig& c, const DynBatchSizes& Z) {
        return aether_dyn_field_workspace_bytes(Z.n_total, c.field_hidden);
    }
    static size_t seq_prior_bytes(const AetherDynStepConfig& c, const DynBatchSizes& Z) {
        return aether_dyn_prior_workspace_bytes(c.encoder_hidden, c.rnn_hidden, c.prior_hidden, Z.n_total, Z.e_total);
    }
    int seq_field(const DynSeqCtx& Q) const {
        return aether_dyn_field(field_params, Q.c.field_hidden, Q.n, Q.fp(Q.L.cur_in), Q.ws + Q.L.ws_field, Q.L.b_field,
                                Q.fp(Q.L.field_c), Q.stream);
    }
    int seq_prior(const DynSeqCtx& Q) const {
        const AetherDynStepConfig& c = Q.c;
        return dyn_prior_impl(prior_params, c.encoder_hidden, c.rnn_hidden, c.prior_layers, c.prior_hidden, c.num_edge_types,
                              c.encoder_polar, Q.n, Q.E, Q.fp(Q.L.cur_in), Q.fp(Q.L.field_c), nullptr, nullptr, Q.ip(Q.L.ksend),
                              Q.ip(Q.L.krecv), Q.ip(Q.L.korder), Q.ip(Q.L.krowptr), Q.ws + Q.L.ws_prior, Q.L.b_prior,
                              Q.prior_logits, Q.fp(Q.L.h1), nullptr, Q.stream, &Q.tail);
    }
    // the data set's graph of a step of the loss loop as the decoder takes it, ext_full (:823)
    void loss_graph(const Ctx& X) const {
        const Layout& L = X.L;
        const int64_t work = std::max<int64_t>(std::max<int64_t>(X.E, X.Z.o_total), X.rows * 6);
        k_dyn_loss_graph<<<dyn_blocks(work), dim3(256), 0, X.st()>>>(X.graph_send, X.graph_recv, X.edge2node, X.n, X.E, X.Z.o_total,
                                                                    X.S.n_max, X.ip(L.send), X.ip(L.recv), X.ip(L.order),
                                                                    X.ip(L.ssend), X.ip(L.srecv), X.state, X.fp(L.field_c), X.cidx(),
                                                                    X.fp(L.ext_full), X.status());
    }
};
}  // namespace
}  // extern "C++"

size_t aether_dyn_step_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max,
                                               const int64_t* n_present, const int64_t* n_edges, const int* in_degree) {
    return dyn_step_bytes<DynBatchLayout>(config, n_scenes, n_objects_max, n_present, n_edges, in_degree);
}

int aether_dyn_step_batched(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                            const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_scenes,
                            int n_objects_max, const int64_t* n_present, const int64_t* n_edges, const int* in_degree,
                            const float* state, const float* mask, const int64_t* node_inds, const int64_t* graph_send,
                            const int64_t* graph_recv, const int64_t* edge2node, float* prior_h, float* prior_c,
                            float* decoder_hidden, const float* uniform, float* prediction, float* edge_types,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return dyn_step_run(DynAetherModel{field_params, prior_params, decoder_params}, config, n_scenes, n_objects_max, n_present,
                        n_edges, in_degree, state, mask, node_inds, graph_send, graph_recv, edge2node, prior_h, prior_c,
                        decoder_hidden, uniform, prediction, edge_types, workspace, workspace_bytes, stream);
}

size_t aether_dyn_rollout_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max, int n_steps,
                                                  const int64_t* n_present, const int64_t* n_edges, const int* in_degree) {
    return dyn_rollout_bytes<DynBatchLayout>(config, n_scenes, n_objects_max, n_steps, n_present, n_edges, in_degree);
}

int aether_dyn_rollout_batched(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                               const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_scenes,
                               int n_objects_max, int n_steps, const float* inputs, const float* masks,
                               const float* burn_in_masks, const int64_t* n_present, const int64_t* n_edges,
                               const int* in_degree, const int64_t* const* node_inds, const int64_t* const* graph_send,
                               const int64_t* const* graph_recv, const int64_t* const* edge2node, const float* const* uniform,
                               float* prior_h, float* prior_c, float* decoder_hidden, float* predictions, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return dyn_rollout_run(DynAetherModel{field_params, prior_params, decoder_params}, config, n_scenes, n_objects_max, n_steps,
                           inputs, masks, burn_in_masks, n_present, n_edges, in_degree, node_inds, graph_send, graph_recv,
                           edge2node, uniform, prior_h, prior_c, decoder_hidden, predictions, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------ one scene: n_scenes = 1 of the above
// The single-scene size functions take no in_degree: they size for the largest one a step accepts (n_edges / n_present).
size_t aether_dyn_step_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int64_t n_present,
                                       int64_t n_edges) {
    if (n_present < 2) {                         // (the batched entry takes an empty scene; a single step does not)
        fail(AETHER_EINVAL, "dyn_step: a step needs 2..n_objects_max present objects");
        return 0;
    }
    const int deg = (int)(n_edges / n_present);
    return aether_dyn_step_batched_workspace_bytes(config, 1, n_objects_max, &n_present, &n_edges, &deg);
}

int aether_dyn_step(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                    const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_objects_max,
                    int64_t n_present, int64_t n_edges, const float* state, const float* mask, const int64_t* node_inds,
                    const int64_t* graph_send, const int64_t* graph_recv, const int64_t* edge2node, int in_degree,
                    float* prior_h, float* prior_c, float* decoder_hidden, const float* uniform, float* prediction,
                    float* edge_types, void* workspace, size_t workspace_bytes, void* stream) {
    if (!field_params || !prior_params || !decoder_params || !state || !mask || !graph_send || !graph_recv || !edge2node ||
        !prior_h || !prior_c || !decoder_hidden || !uniform || !prediction || !workspace)
        return fail(AETHER_EINVAL, "dyn_step: null pointer");
    if (n_present < 2) return fail(AETHER_EINVAL, "dyn_step: a step needs 2..n_objects_max present objects");
    return aether_dyn_step_batched(field_params, prior_params, decoder_params, config, 1, n_objects_max, &n_present, &n_edges,
                                   &in_degree, state, mask, node_inds, graph_send, graph_recv, edge2node, prior_h, prior_c,
                                   decoder_hidden, uniform, prediction, edge_types, workspace, workspace_bytes, stream);
}

size_t aether_dyn_rollout_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int n_steps,
                                          const int64_t* n_present, const int64_t* n_edges) {
    if (!n_present || !n_edges || n_steps <= 0) return 0;
    std::vector<int> deg((size_t)n_steps, 0);
    for (int t = 0; t < n_steps; ++t)
        if (n_present[t] > 0) deg[t] = (int)(n_edges[t] / n_present[t]);
    return aether_dyn_rollout_batched_workspace_bytes(config, 1, n_objects_max, n_steps, n_present, n_edges, deg.data());
}

// The [n_steps] arrays of one scene are the [n_steps][1] arrays of the batched loop: the same memory.
int aether_dyn_rollout(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                       const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_objects_max,
                       int n_steps, const float* inputs, const float* masks, const float* burn_in_masks,
                       const int64_t* n_present, const int64_t* n_edges, const int64_t* const* node_inds,
                       const int64_t* const* graph_send, const int64_t* const* graph_recv, const int64_t* const* edge2node,
                       const int* in_degree, const float* const* uniform, float* prior_h, float* prior_c,
                       float* decoder_hidden, float* predictions, void* workspace, size_t workspace_bytes, void* stream) {
    if (!config || !inputs || !masks || !burn_in_masks || !n_present || !n_edges || !graph_send || !graph_recv || !edge2node ||
        !in_degree || !uniform || !predictions || !workspace || !field_params || !prior_params || !decoder_params || !prior_h ||
        !prior_c || !decoder_hidden)
        return fail(AETHER_EINVAL, "dyn_rollout: null pointer");
    return aether_dyn_rollout_batched(field_params, prior_params, decoder_params, config, 1, n_objects_max, n_steps, inputs, masks,
                                      burn_in_masks, n_present, n_edges, in_degree, node_inds, graph_send, graph_recv, edge2node,
                                      uniform, prior_h, prior_c, decoder_hidden, predictions, workspace, workspace_bytes, stream);
}
