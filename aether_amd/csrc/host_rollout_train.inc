// host_rollout_train.inc -- C entry points of training through the device rollout (include/aether_hip.h, "k-step loss");
// included inside extern "C".  The kernels between the steps: rollout_bwd.h.
//
// Workspace: `steps` slices of the single step's training layout (WsLayout, what aether_backward and
// aether_backward_inputs read; slice t also holds step t's input velocity, in its first velocity buffer).  Only what a
// forward keeps for its backward is a slice's own: slice t + 1 starts where slice t's backward temporaries start
// (WsLayout::saved_end).  The backward runs from the last step to the first, so step t's temporaries land on the slices
// of steps it has already finished with; the last slice is whole.  Behind the slices: everything derived from the
// weights alone (prepared once per call) and the scratch of the chain -- one step's parameter gradients (flat), gx, gv
// of this and the later step, gea, X.
//
// The dynamic-field model (aether_rollout_dynamic_field_train_forward / aether_rollout_dynamic_field_backward) runs the
// same two loops with the latent field around every step (DynRollout).  Forward: k_dynfield on (x_t, v_t), then the kept
// step with that field.  Backward: the step's backward with a grad_field destination, kb_dynfield on it (the field net's
// parameter gradients and gz = dL/d[x | v] through the field), the step's input gradients with gz folded in, the chain
// launch.  No field is kept per step: the step's backward reads it from the kept node table, never through the external
// pointer, and kb_dynfield recomputes the field net from x_t and v_t.  The 27 field-net gradients are summed over the
// steps in the per-graph rows of `partial` (step K-1 clears and writes, kb_dynfield<D, true> of every earlier step adds;
// each entry is owned by one thread) and over the graphs ONCE per call.  The four buffers sit behind the scratch above.

extern "C++" {
namespace {

// Floats of the 47 tensors of an AetherParams, in struct order.  The shapes are stated in three places that must be kept
// in step: the comments of struct AetherParams (include/aether_hip.h), transposed_weights / the kernels that read the
// tensors, and this table (the scratch a step's parameter gradients go to; the gradient tests hold every tensor).
void rollout_param_numels(int D, int* n) {
    const int F1 = 7 * D + D * (D - 1) / 2 + 2, FIN = 2 * D + 16;
    int k = 0;
    auto put = [&](int v) { n[k++] = v; };
    put(32 * FIN); put(32); put(32 * 32); put(32); put(D * 32); put(D); put(3 * 16);
    put(H * F1); put(H); put(H * H); put(H); put(H * 3 * D); put(H); put(2 * H * H); put(2 * H); put(H * 2 * H); put(H);
    const int ln[8] = {H * 3 * H, H, H * H, H, 2 * H * H, 2 * H, H * 2 * H, H};
    for (int t = 0; t < 8; ++t)
        for (int l = 0; l < 3; ++l) put(ln[t]);
    put(H * H); put(H); put(H * H); put(H); put(D * H); put(D);
}
static_assert(sizeof(AetherParams) == RC_MAX_TENSORS * sizeof(float*), "AetherParams: 47 pointers");
constexpr int RC_FIELD_TENSORS = 7;       // the built-in field net's tensors lead the struct (field_w0 .. field_emb)

struct RolloutTrainLayout {
    size_t slice, wimg, wt, pgrad, gx, gv[2], gea, xg, total;
    int numel[RC_MAX_TENSORS], off[RC_MAX_TENSORS], pfloats;
    RolloutTrainLayout(int64_t Nn, int64_t E, int D, int steps) {
        const WsLayout W(Nn, E, D, true);
        slice = align_up(W.saved_end, 256);
        size_t o = slice * (size_t)(steps - 1) + align_up(W.total, 256);
        auto take = [&](size_t floats) { size_t r = o; o = align_up(o + floats * 4, 256); return r; };
        rollout_param_numels(D, numel);
        pfloats = 0;
        for (int k = 0; k < RC_MAX_TENSORS; ++k) { off[k] = pfloats; pfloats += (numel[k] + 3) / 4 * 4; }
        wimg = take(FUSED_WIMG_SET); wt = take((size_t)160 * 1024);      // (WsLayout::wimg, ::wt)
        pgrad = take((size_t)pfloats);
        const size_t nd = (size_t)Nn * D;
        gx = take(nd); gv[0] = take(nd); gv[1] = take(nd);
        gea = take((size_t)(E > 0 ? E : 1) * 2);
        xg = take(nd);
        total = o;
    }
};

// The latent field around the steps of a training rollout; null for the models without one.
struct DynRollout {
    const AetherDynFieldParams* P;
    const AetherDynFieldParams* G;          // destinations of the field-net gradients (the backward)
    int npg;                                // nodes per graph
    float *field, *gfield, *gz, *partial;   // DynRolloutTrainLayout
};

struct DynRolloutTrainLayout : RolloutTrainLayout {
    size_t field, gfield, gz, partial;
    DynRolloutTrainLayout(int64_t Nn, int64_t E, int D, int npg, int steps) : RolloutTrainLayout(Nn, E, D, steps) {
        size_t o = total;
        auto take = [&](size_t floats) { size_t r = o; o = align_up(o + floats * 4, 256); return r; };
        const size_t nd = (size_t)Nn * D;
        field = take(nd); gfield = take(nd); gz = take(2 * nd);
        partial = take((size_t)(Nn / npg) * (size_t)(D == 2 ? DynOff<2>::total : DynOff<3>::total));
        total = o;
    }
    DynRollout bind(char* ws, const AetherDynFieldParams* P, const AetherDynFieldParams* G, int npg) const {
        auto fp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
        return DynRollout{P, G, npg, fp(field), fp(gfield), fp(gz), fp(partial)};
    }
};

bool dyn_rollout_sizes_ok(int64_t n_nodes, int nodes_per_graph) {
    return nodes_per_graph > 0 && nodes_per_graph <= DYNFIELD_MAX_NODES && n_nodes > 0 && n_nodes % nodes_per_graph == 0 &&
           n_nodes / nodes_per_graph < ((int64_t)1 << 31);
}

// nodes_per_graph 0: the entries without a latent field
int rollout_train_check(const char* what, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                        const AetherGraphInfo* info, size_t workspace_bytes, int steps, float dt, int nodes_per_graph = 0) {
    auto bad = [&](int code, const char* msg) { snprintf(g_err, sizeof(g_err), "%s: %s", what, msg); return code; };
    if (hidden > AETHER_HIDDEN) return bad(AETHER_EINVAL, "rollout training: 64-wide engine only");
    if (hidden != AETHER_HIDDEN) return bad(AETHER_EINVAL, "hidden must be 64 (narrower models: zero-pad the parameters)");
    if (num_dims != 2 && num_dims != 3) return bad(AETHER_EINVAL, "num_dims must be 2 or 3");
    if (n_nodes <= 0 || n_edges < 0) return bad(AETHER_EINVAL, "bad sizes");
    if (info->n_nodes != n_nodes || info->n_edges != n_edges) return bad(AETHER_EINVAL, "graph info does not match n_nodes / n_edges");
    if (steps < 1) return bad(AETHER_EINVAL, "steps must be at least 1");
    if (!(dt != 0.0f)) return bad(AETHER_EINVAL, "dt must be non-zero");
    if (nodes_per_graph == 0) {
        if (workspace_bytes < RolloutTrainLayout(n_nodes, n_edges, num_dims, steps).total)
            return bad(AETHER_ESPACE, "workspace too small (aether_rollout_train_workspace_bytes)");
        return AETHER_OK;
    }
    if (!dyn_rollout_sizes_ok(n_nodes, nodes_per_graph))
        return bad(AETHER_EINVAL, "1..2048 nodes per graph, n_nodes a multiple of nodes_per_graph");
    if (workspace_bytes < DynRolloutTrainLayout(n_nodes, n_edges, num_dims, nodes_per_graph, steps).total)
        return bad(AETHER_ESPACE, "workspace too small (aether_rollout_dynamic_field_train_workspace_bytes)");
    return AETHER_OK;
}

template <int D>
int rollout_train_forward_impl(const AetherParams& P, int64_t Nn, int64_t E, const AetherGraphInfo& info, const float* x0,
                               const float* vel0, const float* charges, const char* graph, char* ws, float* trajectory,
                               int steps, float dt, bool fused, hipStream_t st, const DynRollout* dyn = nullptr) {
    const RolloutTrainLayout L(Nn, E, D, steps);
    const WsLayout W(Nn, E, D, true);
    // split images (the fused forward and the fused backward's recompute) and transposed copies (every backward): once
    const PreparedWeights pw{reinterpret_cast<float*>(ws + L.wimg), reinterpret_cast<float*>(ws + L.wt)};
    if (prepare_weights_at<D>(P, pw.wimg, pw.wt, true, true, st)) return AETHER_EHIP;
    const size_t stride = (size_t)Nn * D;
    for (int t = 0; t < steps; ++t) {
        char* sl = ws + L.slice * (size_t)t;
        const float* x = t == 0 ? x0 : trajectory + (size_t)(t - 1) * stride;
        const float* v = t == 0 ? vel0 : reinterpret_cast<const float*>(sl + W.velbuf[0]);
        // v_{t+1} goes where step t + 1 (and its backward) reads it; after the last step nothing reads it
        float* vnext = t + 1 < steps ? reinterpret_cast<float*>(sl + L.slice + W.velbuf[0]) : nullptr;
        if (dyn)                // LatentFieldNetwork on the current state, then the step with that field
            k_dynfield<D><<<dim3((unsigned)(Nn / dyn->npg)), dim3(256), 0, st>>>(*dyn->P, x, v, charges, dyn->field, dyn->npg);
        StepExtras ex{charges, vnext, dt, dyn ? dyn->field : nullptr, true};
        ex.dropword = reinterpret_cast<int*>(sl + W.dropword);        // no masks: the word tells the backward so
        const int rc = fused ? fused_impl<D>(P, Nn, E, info, x, v, charges, nullptr, graph, sl, trajectory + (size_t)t * stride,
                                             true, true, ex, st, true, &pw)
                             : streamed_impl<D>(P, Nn, E, x, v, charges, nullptr, graph, sl, trajectory + (size_t)t * stride,
                                                true, ex, st, &pw);
        if (rc != AETHER_OK) return rc;
    }
    return AETHER_OK;
}

template <int D>
int rollout_backward_impl(const AetherParams& P, const AetherParams& Gr, int64_t Nn, int64_t E, const AetherGraphInfo& info,
                          const float* x0, const float* vel0, const float* charges, const char* graph, char* ws,
                          const float* trajectory, const float* grad_trajectory, float* grad_x0, float* grad_vel0, int steps,
                          float dt, hipStream_t st, const DynRollout* dyn = nullptr) {
    const RolloutTrainLayout L(Nn, E, D, steps);
    const WsLayout W(Nn, E, D, true);
    const GraphLayout G(E, Nn, false);
    auto gp = [&](size_t off) { return reinterpret_cast<const int32_t*>(graph + off); };
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const PreparedWeights pw{fp(L.wimg), fp(L.wt)};                  // written by the forward
    // destinations of steps K-2 .. 0: the scratch, added to `grads` by the chain launch of that step
    // (with an external field a step's backward leaves the built-in field net's seven slots -- the first of the struct --
    // unwritten: they stay out of the sum)
    AetherParams Gs;
    RolloutParamAdd A;
    const int k0 = dyn ? RC_FIELD_TENSORS : 0, n_add = RC_MAX_TENSORS - k0;
    {
        float** gs = reinterpret_cast<float**>(&Gs);
        float* const* gr = reinterpret_cast<float* const*>(&Gr);
        int blocks = 0;
        for (int k = 0; k < RC_MAX_TENSORS; ++k) {
            gs[k] = fp(L.pgrad) + L.off[k];
            if (k < k0) continue;
            const int j = k - k0;
            A.dst[j] = gr[k]; A.numel[j] = L.numel[k]; A.off[j] = L.off[k];
            A.block0[j] = blocks;
            blocks += (L.numel[k] + RC_ADD_BLOCK - 1) / RC_ADD_BLOCK;
        }
        A.block0[n_add] = blocks;
        A.src = fp(L.pgrad);
    }
    const bool fused_bwd = fused_backward_applies<D>(info, Nn, E);
    const size_t stride = (size_t)Nn * D;
    const int node_blocks = (int)((Nn + 7) / 8);
    const float inv_dt = 1.0f / dt;
    for (int t = steps - 1; t >= 0; --t) {
        char* sl = ws + L.slice * (size_t)t;
        auto sp = [&](size_t off) { return reinterpret_cast<float*>(sl + off); };
        const float* x = t == 0 ? x0 : trajectory + (size_t)(t - 1) * stride;
        const float* v = t == 0 ? vel0 : sp(W.velbuf[0]);
        const float* out = trajectory + (size_t)t * stride;
        // X_{t+1}: the last step's is the caller's g_K alone (nothing later reads x_K or v_K)
        const float* g_out = t == steps - 1 ? grad_trajectory + (size_t)t * stride : fp(L.xg);
        const bool last = t == steps - 1;
        const AetherParams& dstp = last ? Gr : Gs;
        float* const gfield = dyn ? dyn->gfield : nullptr;
        int rc = fused_bwd ? backward_fused_impl<D>(P, dstp, Nn, E, info, x, v, charges, graph, sl, g_out, st, gfield, &pw)
                           : backward_impl<D>(P, dstp, Nn, E, x, v, charges, graph, sl, g_out, st, gfield, &pw);
        if (rc != AETHER_OK) return rc;
        if (dyn) {              // dL/dfield -> the field net's gradients (into the rows of `partial`) and dL/d[x | v] through it
            const dim3 grid((unsigned)(Nn / dyn->npg));
            if (last) kb_dynfield<D, false><<<grid, dim3(256), 0, st>>>(*dyn->P, x, v, charges, gfield, dyn->partial, dyn->npg, dyn->gz);
            else kb_dynfield<D, true><<<grid, dim3(256), 0, st>>>(*dyn->P, x, v, charges, gfield, dyn->partial, dyn->npg, dyn->gz);
        }
        float* gv = fp(L.gv[t & 1]);
        rc = backward_inputs_impl<D>(P, Nn, E, x, v, charges, graph, sl, out, g_out, fp(L.gx), gv, fp(L.gea),
                                     dyn ? dyn->gz : nullptr, st);
        if (rc != AETHER_OK) return rc;
        A.n = last ? 0 : n_add;
        const int add_blocks = last ? 0 : A.block0[n_add];
        const float* gv_next = last ? nullptr : fp(L.gv[(t + 1) & 1]);
        k_rollout_chain<D><<<dim3((unsigned)(node_blocks + add_blocks)), dim3(256), 0, st>>>(
            x, t > 0 ? grad_trajectory + (size_t)(t - 1) * stride : nullptr, fp(L.gx), gv, gv_next, fp(L.gea), gp(G.rowptr),
            gp(G.send_s), gp(G.recv_s), gp(G.perm), gp(G.srowptr), gp(G.sperm), inv_dt, t > 0 ? fp(L.xg) : grad_x0,
            t > 0 ? nullptr : grad_vel0, Nn, node_blocks, A);
    }
    if (dyn)                    // the rows hold the sum over the steps: one sum over the graphs
        k_dynfield_reduce<D><<<dim3((DynOff<D>::total + 31) / 32), dim3(256), 0, st>>>(dyn->partial, Nn / dyn->npg, *dyn->G);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

}  // namespace
}  // extern "C++"

size_t aether_rollout_train_workspace_bytes(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden, int steps) {
    if (n_nodes <= 0 || n_edges < 0 || (num_dims != 2 && num_dims != 3) || hidden != AETHER_HIDDEN || steps < 1) return 0;
    return RolloutTrainLayout(n_nodes, n_edges, num_dims, steps).total;
}

int aether_rollout_train_forward(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                                 const float* x0, const float* vel0, const float* charges, const void* graph,
                                 const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, float* trajectory,
                                 int steps, float dt, int flags, void* stream) {
    if (!params || !x0 || !vel0 || !charges || !graph || !info || !workspace || !trajectory)
        return fail(AETHER_EINVAL, "rollout_train_forward: null pointer");
    if (int rc = rollout_train_check("rollout_train_forward", num_dims, hidden, n_nodes, n_edges, info, workspace_bytes, steps, dt))
        return rc;
    const bool fused = info->n_groups > 0 && n_edges > 0 && !(flags & AETHER_FLAG_FORCE_STREAMED);
    if ((flags & AETHER_FLAG_FORCE_FUSED) && !fused)
        return fail(AETHER_EINVAL, "rollout_train_forward: fused path requested but the graph has no groups");
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    if (num_dims == 2)
        return rollout_train_forward_impl<2>(*params, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                             (char*)workspace, trajectory, steps, dt, fused, st);
    return rollout_train_forward_impl<3>(*params, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                         (char*)workspace, trajectory, steps, dt, fused, st);
}

int aether_rollout_backward(const AetherParams* params, const AetherParams* grads, int num_dims, int hidden, int64_t n_nodes,
                            int64_t n_edges, const float* x0, const float* vel0, const float* charges, const void* graph,
                            const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* trajectory,
                            const float* grad_trajectory, float* grad_x0, float* grad_vel0, int steps, float dt, void* stream) {
    if (!params || !grads || !x0 || !vel0 || !charges || !graph || !info || !workspace || !trajectory || !grad_trajectory)
        return fail(AETHER_EINVAL, "rollout_backward: null pointer");
    {
        const float* const* gp = reinterpret_cast<const float* const*>(grads);
        for (int k = 0; k < RC_MAX_TENSORS; ++k)
            if (!gp[k]) return fail(AETHER_EINVAL, "rollout_backward: null gradient pointer");
    }
    if (int rc = rollout_train_check("rollout_backward", num_dims, hidden, n_nodes, n_edges, info, workspace_bytes, steps, dt))
        return rc;
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    if (num_dims == 2)
        return rollout_backward_impl<2>(*params, *grads, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                        (char*)workspace, trajectory, grad_trajectory, grad_x0, grad_vel0, steps, dt, st);
    return rollout_backward_impl<3>(*params, *grads, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                    (char*)workspace, trajectory, grad_trajectory, grad_x0, grad_vel0, steps, dt, st);
}

size_t aether_rollout_dynamic_field_train_workspace_bytes(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden,
                                                          int nodes_per_graph, int steps) {
    if (n_nodes <= 0 || n_edges < 0 || (num_dims != 2 && num_dims != 3) || hidden != AETHER_HIDDEN || steps < 1) return 0;
    if (!dyn_rollout_sizes_ok(n_nodes, nodes_per_graph)) return 0;
    return DynRolloutTrainLayout(n_nodes, n_edges, num_dims, nodes_per_graph, steps).total;
}

int aether_rollout_dynamic_field_train_forward(const AetherParams* params, const AetherDynFieldParams* dyn_params, int num_dims,
                                               int hidden, int64_t n_nodes, int64_t n_edges, int nodes_per_graph,
                                               const float* x0, const float* vel0, const float* charges, const void* graph,
                                               const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                                               float* trajectory, int steps, float dt, int flags, void* stream) {
    const char* what = "rollout_dynamic_field_train_forward";
    if (!params || !dyn_params || !x0 || !vel0 || !charges || !graph || !info || !workspace || !trajectory)
        return fail(AETHER_EINVAL, "rollout_dynamic_field_train_forward: null pointer");
    if (nodes_per_graph <= 0) return fail(AETHER_EINVAL, "rollout_dynamic_field_train_forward: 1..2048 nodes per graph");
    if (int rc = rollout_train_check(what, num_dims, hidden, n_nodes, n_edges, info, workspace_bytes, steps, dt, nodes_per_graph))
        return rc;
    const bool fused = info->n_groups > 0 && n_edges > 0 && !(flags & AETHER_FLAG_FORCE_STREAMED);
    if ((flags & AETHER_FLAG_FORCE_FUSED) && !fused)
        return fail(AETHER_EINVAL, "rollout_dynamic_field_train_forward: fused path requested but the graph has no groups");
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    const DynRollout dyn = DynRolloutTrainLayout(n_nodes, n_edges, num_dims, nodes_per_graph, steps)
                               .bind((char*)workspace, dyn_params, nullptr, nodes_per_graph);
    if (num_dims == 2)
        return rollout_train_forward_impl<2>(*params, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                             (char*)workspace, trajectory, steps, dt, fused, st, &dyn);
    return rollout_train_forward_impl<3>(*params, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                         (char*)workspace, trajectory, steps, dt, fused, st, &dyn);
}

int aether_rollout_dynamic_field_backward(const AetherParams* params, const AetherDynFieldParams* dyn_params,
                                          const AetherParams* grads, const AetherDynFieldParams* dyn_grads, int num_dims,
                                          int hidden, int64_t n_nodes, int64_t n_edges, int nodes_per_graph, const float* x0,
                                          const float* vel0, const float* charges, const void* graph,
                                          const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                                          const float* trajectory, const float* grad_trajectory, float* grad_x0,
                                          float* grad_vel0, int steps, float dt, void* stream) {
    const char* what = "rollout_dynamic_field_backward";
    if (!params || !dyn_params || !grads || !dyn_grads || !x0 || !vel0 || !charges || !graph || !info || !workspace ||
        !trajectory || !grad_trajectory)
        return fail(AETHER_EINVAL, "rollout_dynamic_field_backward: null pointer");
    {
        const float* const* gp = reinterpret_cast<const float* const*>(grads);
        for (int k = 0; k < RC_MAX_TENSORS; ++k)
            if (!gp[k]) return fail(AETHER_EINVAL, "rollout_dynamic_field_backward: null gradient pointer");
        const float* const* dp = reinterpret_cast<const float* const*>(dyn_grads);
        for (size_t k = 0; k < sizeof(AetherDynFieldParams) / sizeof(const float*); ++k)
            if (!dp[k]) return fail(AETHER_EINVAL, "rollout_dynamic_field_backward: null field-net gradient pointer");
    }
    if (nodes_per_graph <= 0) return fail(AETHER_EINVAL, "rollout_dynamic_field_backward: 1..2048 nodes per graph");
    if (int rc = rollout_train_check(what, num_dims, hidden, n_nodes, n_edges, info, workspace_bytes, steps, dt, nodes_per_graph))
        return rc;
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    const DynRollout dyn = DynRolloutTrainLayout(n_nodes, n_edges, num_dims, nodes_per_graph, steps)
                               .bind((char*)workspace, dyn_params, dyn_grads, nodes_per_graph);
    if (num_dims == 2)
        return rollout_backward_impl<2>(*params, *grads, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                        (char*)workspace, trajectory, grad_trajectory, grad_x0, grad_vel0, steps, dt, st, &dyn);
    return rollout_backward_impl<3>(*params, *grads, n_nodes, n_edges, *info, x0, vel0, charges, (const char*)graph,
                                    (char*)workspace, trajectory, grad_trajectory, grad_x0, grad_vel0, steps, dt, st, &dyn);
}
