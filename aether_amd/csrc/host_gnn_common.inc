// Host plumbing shared by the layer-by-layer GNN models (host_egnn.inc, host_clof.inc): workspace arena, gradient-buffer
// offsets, graph-view pointers, argument checks, template dispatch and the weight-gradient reduction.  Included by
// aether_hip.hip before them, inside its extern "C" block; not a stand-alone source file.  Device side: csrc/gnn_common.h.

extern "C++" {
namespace {

// fail() with the entry's name in front: "<what>: <why>"
int gnn_fail(int code, const char* what, const char* why) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    return fail(code, msg);
}

// Workspace layout: regions of floats one after the other, each at a 256-byte boundary.
struct FloatArena {
    size_t off = 0;
    size_t take(size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; }
};

// Pointers into a workspace: wp(off), and slot s of the layouts' [slots][Nn][H] (hs, gh) and [slots][Nn][3] (xs, gx) regions
struct WsFloats {
    char* ws;
    int64_t Nn;
    size_t H, hs, xs, ghs, gxs;
    float* operator()(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    float* h(int s) const { return (*this)(hs) + (size_t)s * Nn * H; }        // layer inputs (keep: every layer's)
    float* x(int s) const { return (*this)(xs) + (size_t)s * Nn * 3; }
    float* gh(int s) const { return (*this)(ghs) + (size_t)s * Nn * H; }      // backward: two alternating gradient slots
    float* gx(int s) const { return (*this)(gxs) + (size_t)s * Nn * 3; }
};

// float offset of parameter p in the flat gradient buffer: every tensor padded to 4 floats (16 bytes), in
// named_parameters() order -- the layout of the drop-ins' _grad_buffers.  p = the parameter count: the buffer's size.
template <class Numel>
int64_t gnn_grad_offset(int p, Numel numel) {
    int64_t off = 0;
    for (int q = 0; q < p; ++q) off += (numel(q) + 3) / 4 * 4;
    return off;
}

// The row-sorted graph view (aether_graph_build with the index rows swapped): CSR by row = edges[0] (rowptr, perm, row_s,
// col_s) and the same sorted positions grouped by col (sperm, srowptr)
struct GraphView {
    const int32_t *perm, *row_s, *col_s, *rowptr, *sperm, *srowptr;
    GraphView(const void* graph, int64_t Nn, int64_t E) {
        const GraphLayout G(E, Nn, false);
        auto gp = [&](size_t off) { return reinterpret_cast<const int32_t*>((const char*)graph + off); };
        perm = gp(G.perm); row_s = gp(G.recv_s); col_s = gp(G.send_s); rowptr = gp(G.rowptr);
        sperm = gp(G.sperm); srowptr = gp(G.srowptr);
    }
};

// What every entry checks once the model's own sizes are known to be valid.  n_per: nodes per graph (1: no such notion).
int gnn_check(const float* const* params, int n_params, int want_params, const char* params_why, int n_per, int64_t Nn,
              int64_t E, const void* graph, const AetherGraphInfo* info, const char* what) {
    auto bad = [&](const char* why) { return gnn_fail(AETHER_EINVAL, what, why); };
    if (!params || n_params != want_params) return bad(params_why);
    for (int p = 0; p < n_params; ++p)
        if (!params[p]) return bad("null parameter pointer");
    if (Nn <= 0 || E < 0 || Nn >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) return bad("bad sizes");
    if (n_per < 1 || Nn % n_per != 0) return bad("n_nodes must be a multiple of the nodes per graph");
    if (!graph || !info || info->n_nodes != Nn || info->n_edges != E)
        return bad("graph view missing or built for another (n_nodes, n_edges)");
    return AETHER_OK;
}

// The rest of a forward / backward entry's checks.  grad_need < 0: a forward (no gradient buffer).
int gnn_entry_check(const char* what, bool any_null, int unknown_flags, size_t ws_bytes, size_t ws_need,
                    int64_t grad_floats = 0, int64_t grad_need = -1) {
    auto bad = [&](int code, const char* why) { return gnn_fail(code, what, why); };
    if (any_null) return bad(AETHER_EINVAL, "null pointer");
    if (unknown_flags) return bad(AETHER_EINVAL, "unknown flag");
    if (grad_need < 0) return ws_bytes < ws_need ? bad(AETHER_ESPACE, "workspace too small") : AETHER_OK;
    if (grad_floats < grad_need) return bad(AETHER_ESPACE, "gradient buffer too small");
    if (ws_bytes < ws_need) return bad(AETHER_ESPACE, "workspace too small (keep-for-backward size)");
    return AETHER_OK;
}

// "h" / "x" of aether_*_workspace_offset: byte offset of layer `layer`'s input in the keep-for-backward workspace
int64_t gnn_slot_offset(const char* what, const char* names, const char* name, int layer, int n_layers, size_t hs, size_t xs,
                        int64_t n_nodes, int hidden) {
    if (layer < 0 || layer > n_layers) return gnn_fail(AETHER_EINVAL, what, "layer outside [0, n_layers]");
    if (!strcmp(name, "h")) return (int64_t)(hs + (size_t)layer * n_nodes * hidden * 4);
    if (!strcmp(name, "x")) return (int64_t)(xs + (size_t)layer * n_nodes * 3 * 4);
    char why[64];
    snprintf(why, sizeof(why), "unknown name (%s)", names);
    return gnn_fail(AETHER_EINVAL, what, why);
}

// f(std::bool_constant<b>...) for run-time bools, first bool first: picks a kernel's template arguments, e.g.
//   dispatch_bools([&](auto NORM, auto TANH) { k<decltype(NORM)::value, decltype(TANH)::value><<<...>>>(...); }, norm, tanh)
template <class F>
void dispatch_bools(F f) { f(); }
template <class F, class... Bs>
void dispatch_bools(F f, bool b, Bs... rest) {
    if (b) dispatch_bools([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else dispatch_bools([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

// The jobs of one weight-gradient launch (gnn_common.h): out[J][K] (row stride ldo) = G[rows][J]^T act(A[rows][K])
struct WgTable {
    gnn::WgJobs T;
    WgTable() { T.n = 0; }
    void add(const float* G, int ldg, const float* A, int lda, int act, float* out, int ldo, int J, int K, int64_t rows) {
        gnn::WgJob& j = T.j[T.n++];
        j.G = G; j.A = A; j.out = out; j.ldg = ldg; j.lda = lda; j.ldo = ldo; j.J = J; j.K = K; j.act = act; j.rows = rows;
        j.tile0 = j.poff = 0;
    }
};

// Both stages: the model's `part` kernel (one workgroup of `block` threads per edge x edge output tile and row chunk) into
// part[n_ch][<= part_out], then k_gnn_wgrad_sum
int gnn_wgrad(gnn::WgJobs& T, int edge, int block, void (*part_kernel)(gnn::WgJobs, float*), float* part, int64_t part_out,
              int64_t n_ch, const char* too_many, hipStream_t st) {
    int tiles = 0, outs = 0;
    for (int q = 0; q < T.n; ++q) {
        gnn::WgJob& J = T.j[q];
        J.tile0 = tiles;
        J.poff = outs;
        tiles += ((J.J + edge - 1) / edge) * ((J.K + edge - 1) / edge);
        outs += J.J * J.K;
    }
    if (outs > part_out) return fail(AETHER_EINVAL, too_many);
    T.n_tiles = tiles;
    T.n_out = outs;
    T.n_ch = (int)n_ch;
    part_kernel<<<dim3((unsigned)tiles, (unsigned)T.n_ch), dim3(block), 0, st>>>(T, part);
    gnn::k_gnn_wgrad_sum<<<dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st>>>(T, part);
    return AETHER_OK;
}

// State of a device rollout, behind the model's inference workspace (`base` bytes): vel[Nn][3], h[Nn] and edge_attr[E][2]
// of the step about to run.  Positions need no buffer of their own: step t reads x0 (t = 0) or row t - 1 of the
// trajectory and writes row t.
struct RolloutState : FloatArena {
    size_t vel, h, ea, total;
    RolloutState(size_t base, int64_t Nn, int64_t E) {
        off = align_up(base, 256);
        vel = take((size_t)Nn * 3);
        h = take((size_t)Nn);
        ea = take((size_t)(E > 0 ? E : 1) * 2);
        total = off;
    }
};

// What a rollout entry checks beyond gnn_check: widths and flags a rollout cannot serve, pointers, workspace
int gnn_rollout_check(const char* what, int in_nf, int keep_flag, bool any_null, int unknown_flags, size_t ws_bytes,
                      size_t ws_need) {
    if (in_nf != 1) return gnn_fail(AETHER_EINVAL, what, "in_node_nf must be 1 (h = |vel| is rebuilt every step)");
    if (keep_flag) return gnn_fail(AETHER_EINVAL, what, "the keep-for-backward flag has no meaning in a rollout");
    return gnn_entry_check(what, any_null, unknown_flags, ws_bytes, ws_need);
}

// The loop of aether_egnn_rollout / aether_clof_rollout: x_{t+1} = model(x_t, v_t), v_{t+1} = (x_{t+1} - x_t) / dt, the
// step's h and edge_attr from k_gnn_rollout_state.  step(h, x, vel, edge_attr, out) launches the model's layers (weight
// images already prepared by the caller).  Launches only: no allocation, no synchronisation, nothing read back.
template <class Step>
int gnn_rollout(char* ws, const RolloutState& R, int64_t Nn, int64_t E, const float* x0, const float* vel0,
                const float* charges, const int64_t* send, const int64_t* recv, float* traj, int steps, float dt,
                hipStream_t st, Step step) {
    float *vel = reinterpret_cast<float*>(ws + R.vel), *h = reinterpret_cast<float*>(ws + R.h),
          *ea = reinterpret_cast<float*>(ws + R.ea);
    const dim3 grid((unsigned)(((E > Nn ? E : Nn) + 255) / 256)), block(256);
    const size_t row = (size_t)Nn * 3;
    for (int t = 0; t < steps; ++t) {
        const float* x = t == 0 ? x0 : traj + (size_t)(t - 1) * row;
        if (t == 0)
            gnn::k_gnn_rollout_state<true><<<grid, block, 0, st>>>(Nn, E, x, nullptr, vel0, dt, charges, recv, send, vel, h, ea);
        else
            gnn::k_gnn_rollout_state<false><<<grid, block, 0, st>>>(Nn, E, x, t == 1 ? x0 : traj + (size_t)(t - 2) * row,
                                                                     nullptr, dt, charges, recv, send, vel, h, ea);
        if (int rc = step(h, x, vel, ea, traj + (size_t)t * row)) return rc;
    }
    return AETHER_OK;
}

}  // namespace
}  // extern "C++"
