// host_wide.inc -- C entry points that take the hidden width (include/aether_hip.h, "any hidden_size"); included inside
// extern "C".  hidden == 64: the calls above (fused / streamed 64-wide kernels); hidden = 64 m > 64: wide.h.

static int wide_check_hidden(int hidden, const char* what) {
    if (hidden == AETHER_HIDDEN || wide_hidden_ok(hidden)) return AETHER_OK;
    snprintf(g_err, sizeof(g_err), "%s: hidden must be a multiple of 64 in [64, 4096] (other widths: zero-pad the parameters)", what);
    return AETHER_EINVAL;
}

size_t aether_workspace_bytes_h(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden, int keep_for_backward) {
    if (hidden == AETHER_HIDDEN) return aether_workspace_bytes(n_nodes, n_edges, num_dims, keep_for_backward);
    if (n_nodes <= 0 || n_edges < 0 || (num_dims != 2 && num_dims != 3) || !wide_hidden_ok(hidden)) return 0;
    return WideLayout(n_nodes, n_edges, num_dims, hidden, keep_for_backward != 0).total;
}

size_t aether_dropout_mask_offset_h(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden) {
    if (hidden == AETHER_HIDDEN) return aether_dropout_mask_offset(n_nodes, n_edges, num_dims);
    if (n_nodes <= 0 || n_edges < 0 || (num_dims != 2 && num_dims != 3) || !wide_hidden_ok(hidden)) return 0;
    return WideLayout(n_nodes, n_edges, num_dims, hidden, true).drop;
}

int aether_forward_h(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                     const float* x, const float* vel, const float* charges, const float* field,
                     const float* edge_attr_orig, const void* graph, const AetherGraphInfo* info,
                     void* workspace, size_t workspace_bytes, float* out, int flags, void* stream) {
    if (wide_check_hidden(hidden, "forward_h")) return AETHER_EINVAL;
    if (hidden == AETHER_HIDDEN)
        return forward_common(params, num_dims, n_nodes, n_edges, x, vel, charges, edge_attr_orig, graph, info, workspace,
                              workspace_bytes, out, flags, stream, field);
    if (!params || !x || !vel || !charges || !graph || !info || !workspace || !out)
        return fail(AETHER_EINVAL, "forward_h: null pointer");
    if (take_async_error()) return AETHER_EHIP;
    if (info->n_nodes != n_nodes || info->n_edges != n_edges)
        return fail(AETHER_EINVAL, "forward_h: graph info does not match n_nodes / n_edges");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "forward_h: num_dims must be 2 or 3");
    if (n_nodes <= 0 || n_edges < 0) return fail(AETHER_EINVAL, "forward_h: bad sizes");
    if (n_edges > 0 && !edge_attr_orig) return fail(AETHER_EINVAL, "forward_h: null edge_attr");
    if (flags & AETHER_FLAG_FORCE_FUSED) return fail(AETHER_EINVAL, "forward_h: the fused kernel is 64 wide");
    const bool keep = (flags & AETHER_FLAG_KEEP_INTERMEDIATES) != 0;
    if ((flags & AETHER_FLAG_DROPOUT) && !keep)
        return fail(AETHER_EINVAL, "forward_h: AETHER_FLAG_DROPOUT needs AETHER_FLAG_KEEP_INTERMEDIATES (the masks live in the training workspace)");
    const WideLayout W(n_nodes, n_edges, num_dims, hidden, keep);
    if (workspace_bytes < W.total) return fail(AETHER_ESPACE, "forward_h: workspace too small");
    StepExtras ex{nullptr, nullptr, 1.0f, field};
    if (keep) {
        float* masks = reinterpret_cast<float*>((char*)workspace + W.drop);
        if (flags & AETHER_FLAG_DROPOUT) { ex.drop1 = masks; ex.drop2 = masks + (size_t)n_nodes * hidden; }
        ex.dropword = reinterpret_cast<int*>((char*)workspace + W.dropword);
    }
    hipStream_t st = (hipStream_t)stream;
    if (num_dims == 2)
        return wide_forward_impl<2>(*params, hidden, n_nodes, n_edges, x, vel, charges, edge_attr_orig, (const char*)graph,
                                    (char*)workspace, out, keep, ex, st);
    return wide_forward_impl<3>(*params, hidden, n_nodes, n_edges, x, vel, charges, edge_attr_orig, (const char*)graph,
                                (char*)workspace, out, keep, ex, st);
}

int aether_backward_h(const AetherParams* params, const AetherParams* grads, int num_dims, int hidden, int64_t n_nodes,
                      int64_t n_edges, const float* x, const float* vel, const float* charges, const void* graph,
                      const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* grad_out,
                      float* grad_field, void* stream) {
    if (wide_check_hidden(hidden, "backward_h")) return AETHER_EINVAL;
    if (hidden == AETHER_HIDDEN) {
        if (grad_field)
            return aether_backward_field(params, grads, num_dims, n_nodes, n_edges, x, vel, charges, graph, info, workspace,
                                         workspace_bytes, grad_out, grad_field, stream);
        return aether_backward(params, grads, num_dims, n_nodes, n_edges, x, vel, charges, graph, info, workspace,
                               workspace_bytes, grad_out, stream);
    }
    if (!params || !grads || !x || !vel || !charges || !graph || !info || !workspace || !grad_out)
        return fail(AETHER_EINVAL, "backward_h: null pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "backward_h: num_dims must be 2 or 3");
    if (n_nodes <= 0 || n_edges < 0 || info->n_nodes != n_nodes || info->n_edges != n_edges)
        return fail(AETHER_EINVAL, "backward_h: bad sizes");
    if (workspace_bytes < WideLayout(n_nodes, n_edges, num_dims, hidden, true).total)
        return fail(AETHER_ESPACE, "backward_h: workspace too small (forward must run with KEEP_INTERMEDIATES)");
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    if (num_dims == 2)
        return wide_backward_impl<2>(*params, *grads, hidden, n_nodes, n_edges, x, vel, charges, (const char*)graph,
                                     (char*)workspace, grad_out, st, grad_field);
    return wide_backward_impl<3>(*params, *grads, hidden, n_nodes, n_edges, x, vel, charges, (const char*)graph,
                                 (char*)workspace, grad_out, st, grad_field);
}

int aether_backward_inputs_h(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                             const float* x, const float* vel, const float* charges, const void* graph,
                             const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* out,
                             const float* grad_out, float* grad_x, float* grad_vel, float* grad_edge_attr,
                             const float* field_input_grad, void* stream) {
    if (wide_check_hidden(hidden, "backward_inputs_h")) return AETHER_EINVAL;
    if (hidden == AETHER_HIDDEN)
        return aether_backward_inputs(params, num_dims, n_nodes, n_edges, x, vel, charges, graph, info, workspace,
                                      workspace_bytes, out, grad_out, grad_x, grad_vel, grad_edge_attr, field_input_grad, stream);
    if (!params || !x || !vel || !charges || !graph || !info || !workspace || !out || !grad_out || !grad_x || !grad_vel)
        return fail(AETHER_EINVAL, "backward_inputs_h: null pointer");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "backward_inputs_h: num_dims must be 2 or 3");
    if (n_nodes <= 0 || n_edges < 0 || info->n_nodes != n_nodes || info->n_edges != n_edges)
        return fail(AETHER_EINVAL, "backward_inputs_h: bad sizes");
    GraphLayout G(n_edges, n_nodes, false);
    WideLayout W(n_nodes, n_edges, num_dims, hidden, true);
    if (workspace_bytes < W.total)
        return fail(AETHER_ESPACE, "backward_inputs_h: workspace too small (the workspace of the forward / backward pair)");
    if (take_async_error()) return AETHER_EHIP;
    hipStream_t st = (hipStream_t)stream;
    const char* g = (const char*)graph;
    char* ws = (char*)workspace;
    auto gp = [&](size_t off) { return reinterpret_cast<const int32_t*>(g + off); };
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const dim3 grid((unsigned)((n_nodes + 7) / 8));
    if (num_dims == 2)
        kb_inputs<2><<<grid, dim3(256), 0, st>>>(*params, x, vel, charges, wp(W.nodeinfo), wp(W.o2), grad_out, wp(W.DA), wp(W.DN),
                                               wp(W.DF), gp(G.rowptr), gp(G.send_s), gp(G.recv_s), gp(G.srowptr),
                                               gp(G.sperm), grad_x, grad_vel, n_nodes, field_input_grad, hidden);
    else
        kb_inputs<3><<<grid, dim3(256), 0, st>>>(*params, x, vel, charges, wp(W.nodeinfo), wp(W.o2), grad_out, wp(W.DA), wp(W.DN),
                                               wp(W.DF), gp(G.rowptr), gp(G.send_s), gp(G.recv_s), gp(G.srowptr),
                                               gp(G.sperm), grad_x, grad_vel, n_nodes, field_input_grad, hidden);
    if (grad_edge_attr && n_edges > 0) {
        const int D = num_dims, col0 = 7 * D + D * (D - 1) / 2;
        kb_edge_attr_grad<<<dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, st>>>(wp(W.DA), gp(G.perm), col0, grad_edge_attr,
                                                                                       n_edges);
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

static int wide_rollout(const AetherParams* params, const AetherDynFieldParams* dyn, int nodes_per_graph, float* field_buf,
                        int num_dims, int hidden, int64_t n_nodes, int64_t n_edges, const float* x0, const float* vel0,
                        const float* charges, const void* graph, const AetherGraphInfo* info, void* workspace,
                        size_t workspace_bytes, float* trajectory, int steps, float dt, int flags, void* stream) {
    if (!params || !x0 || !vel0 || !charges || !graph || !info || !workspace || !trajectory)
        return fail(AETHER_EINVAL, "rollout_h: null pointer");
    if (take_async_error()) return AETHER_EHIP;
    if (info->n_nodes != n_nodes || info->n_edges != n_edges)
        return fail(AETHER_EINVAL, "rollout_h: graph info does not match n_nodes / n_edges");
    if (num_dims != 2 && num_dims != 3) return fail(AETHER_EINVAL, "rollout_h: num_dims must be 2 or 3");
    if (n_nodes <= 0 || n_edges < 0 || steps < 0) return fail(AETHER_EINVAL, "rollout_h: bad sizes");
    if (!(dt != 0.0f)) return fail(AETHER_EINVAL, "rollout_h: dt must be non-zero");
    if (flags & (AETHER_FLAG_KEEP_INTERMEDIATES | AETHER_FLAG_FORCE_FUSED))
        return fail(AETHER_EINVAL, "rollout_h: inference only, and the fused kernel is 64 wide");
    if (dyn && (!field_buf || nodes_per_graph <= 0 || n_nodes % nodes_per_graph != 0))
        return fail(AETHER_EINVAL, "rollout_h: n_nodes must be a multiple of nodes_per_graph (and a field buffer given)");
    WideLayout W(n_nodes, n_edges, num_dims, hidden, false);
    if (workspace_bytes < W.total) return fail(AETHER_ESPACE, "rollout_h: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const size_t stride = (size_t)n_nodes * num_dims;
    for (int t = 0; t < steps; ++t) {
        const float* x = t == 0 ? x0 : trajectory + (size_t)(t - 1) * stride;
        const float* v = t == 0 ? vel0 : reinterpret_cast<const float*>(ws + W.velbuf[(t - 1) & 1]);
        float* out = trajectory + (size_t)t * stride;
        if (dyn) {              // the dynamic-field model: LatentFieldNetwork on the current state, then the step
            const int rc = aether_dynamic_field(dyn, num_dims, n_nodes / nodes_per_graph, nodes_per_graph, x, v, charges,
                                                field_buf, stream);
            if (rc != AETHER_OK) return rc;
        }
        StepExtras ex{charges, reinterpret_cast<float*>(ws + W.velbuf[t & 1]), dt, dyn ? field_buf : nullptr};
        const int rc = num_dims == 2 ? wide_forward_impl<2>(*params, hidden, n_nodes, n_edges, x, v, charges, nullptr,
                                                            (const char*)graph, ws, out, false, ex, st)
                                     : wide_forward_impl<3>(*params, hidden, n_nodes, n_edges, x, v, charges, nullptr,
                                                            (const char*)graph, ws, out, false, ex, st);
        if (rc != AETHER_OK) return rc;
    }
    return AETHER_OK;
}

int aether_rollout_h(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges, const float* x0,
                     const float* vel0, const float* charges, const void* graph, const AetherGraphInfo* info,
                     void* workspace, size_t workspace_bytes, float* trajectory, int steps, float dt, int flags,
                     void* stream) {
    if (wide_check_hidden(hidden, "rollout_h")) return AETHER_EINVAL;
    if (hidden == AETHER_HIDDEN)
        return aether_rollout(params, num_dims, n_nodes, n_edges, x0, vel0, charges, graph, info, workspace, workspace_bytes,
                              trajectory, steps, dt, flags, stream);
    return wide_rollout(params, nullptr, 0, nullptr, num_dims, hidden, n_nodes, n_edges, x0, vel0, charges, graph, info,
                        workspace, workspace_bytes, trajectory, steps, dt, flags, stream);
}

int aether_rollout_dynamic_field_h(const AetherParams* params, const AetherDynFieldParams* dyn_params, int num_dims,
                                   int hidden, int64_t n_nodes, int64_t n_edges, int nodes_per_graph, const float* x0,
                                   const float* vel0, const float* charges, const void* graph, const AetherGraphInfo* info,
                                   void* workspace, size_t workspace_bytes, float* field_scratch, float* trajectory,
                                   int steps, float dt, int flags, void* stream) {
    if (wide_check_hidden(hidden, "rollout_dynamic_field_h")) return AETHER_EINVAL;
    if (hidden == AETHER_HIDDEN)
        return aether_rollout_dynamic_field(params, dyn_params, num_dims, n_nodes, n_edges, nodes_per_graph, x0, vel0, charges,
                                            graph, info, workspace, workspace_bytes, field_scratch, trajectory, steps, dt,
                                            flags, stream);
    if (!dyn_params) return fail(AETHER_EINVAL, "rollout_dynamic_field_h: null pointer");
    return wide_rollout(params, dyn_params, nodes_per_graph, field_scratch, num_dims, hidden, n_nodes, n_edges, x0, vel0,
                        charges, graph, info, workspace, workspace_bytes, trajectory, steps, dt, flags, stream);
}

int64_t aether_debug_fetch_h(const char* name, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                             const void* workspace, float* dst, void* stream) {
    if (hidden == AETHER_HIDDEN) return aether_debug_fetch(name, num_dims, n_nodes, n_edges, workspace, dst, stream);
    if (!name || !workspace || !dst) return fail(AETHER_EINVAL, "debug_fetch_h: null pointer");
    if ((num_dims != 2 && num_dims != 3) || !wide_hidden_ok(hidden)) return fail(AETHER_EINVAL, "debug_fetch_h: num_dims / hidden");
    const int D = num_dims, NIS = D == 2 ? 16 : 24;
    WideLayout W(n_nodes, n_edges, D, hidden, true);       // per-layer tensors exist in the training layout only
    const char* ws = (const char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    auto copy2d = [&](const float* src, int64_t rows, int src_ld, int col0, int cols) -> int64_t {
        hipError_t e = hipMemcpy2DAsync(dst, (size_t)cols * 4, src + col0, (size_t)src_ld * 4,
                                        (size_t)cols * 4, (size_t)rows, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) { fail(AETHER_EHIP, hipGetErrorString(e)); return AETHER_EHIP; }
        return rows * cols;
    };
    const float* ni = (const float*)(ws + W.nodeinfo);
    if (!strcmp(name, "field")) return copy2d(ni, n_nodes, NIS, 2 * D, D);
    if (!strcmp(name, "R")) return copy2d(ni, n_nodes, NIS, 3 * D, D * D);
    if (!strcmp(name, "canon")) return copy2d(ni, n_nodes, NIS, 3 * D + D * D, 2 * D);
    if (name[0] == 'x' && name[1] >= '0' && name[1] <= '4' && !name[2])
        return copy2d((const float*)(ws + W.x[name[1] - '0']), n_nodes, hidden, 0, hidden);
    if (name[0] == 'e' && name[1] >= '1' && name[1] <= '4' && !name[2])
        return copy2d((const float*)(ws + W.em[name[1] - '1']), n_edges, hidden, 0, hidden);
    if (!strcmp(name, "efeat")) return copy2d((const float*)(ws + W.feat), n_edges, FPAD, 0, FPAD);
    return fail(AETHER_EINVAL, "debug_fetch_h: unknown name");
}
