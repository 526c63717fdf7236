// Host side of the C ABI: EGNN-Aether (EGNN_vel_Aether, nn/state2state/egnn_aether.py), forward and parameter backward.
// Included by aether_hip.hip inside its extern "C" block; not a stand-alone source file.  Kernels: csrc/egnn.h; shared
// plumbing: csrc/host_gnn_common.inc.

extern "C++" {
namespace {

// Parameter tensors in the reference's named_parameters() order (= state_dict order)
constexpr int EGNN_FLAGS = AETHER_EGNN_NORM_DIFF | AETHER_EGNN_TANH | AETHER_EGNN_KEEP;
constexpr int EGNN_PER_LAYER = 15;        // edge_mlp.0 w b, .2 w b, node_mlp.0 w b, .2 w b, coord_mlp.0 w b, .2 w,
                                          // coord_mlp_vel.0 w b, .2 w b
constexpr int EGNN_FIELD = 7;             // field_net.net.0 w b, .2 w b, .4 w b, class_embedding

int egnn_n_params(int L) { return 2 + EGNN_PER_LAYER * L + EGNN_FIELD; }
bool egnn_sizes_ok(int H, int L, int in_nf) { return (H == 64 || H == 128) && L >= 1 && L <= 64 && in_nf >= 1; }

// numel of parameter p (named_parameters order)
int64_t egnn_numel(int p, int H, int L, int in_nf) {
    const int64_t KIN = 2 * H + 9;
    if (p == 0) return (int64_t)H * in_nf;
    if (p == 1) return H;
    if (p < 2 + EGNN_PER_LAYER * L) {
        const int64_t sz[EGNN_PER_LAYER] = {H * KIN, H, (int64_t)H * H, H, 2LL * H * H, H, (int64_t)H * H, H,
                                            (int64_t)H * H, H, H, (int64_t)H * (H + 3), H, H, 1};
        return sz[(p - 2) % EGNN_PER_LAYER];
    }
    const int64_t fs[EGNN_FIELD] = {egnn::FH * egnn::FIN, egnn::FH, egnn::FH * egnn::FH, egnn::FH, 3 * egnn::FH, 3, 3 * 16};
    return fs[p - 2 - EGNN_PER_LAYER * L];
}

int64_t egnn_grad_offset(int p, int H, int L, int in_nf) {
    return gnn_grad_offset(p, [&](int q) { return egnn_numel(q, H, L, in_nf); });
}

struct EgnnLayout : FloatArena {
    size_t wt, F, hs, xs, agg, total_fwd;
    size_t gh, gx, gf, ghn, gagg, zn, gn1, zp, gp1, gpsi, gxm, gfn, ghe, gxe, gfe;
    size_t in, z1, m, z3, ga1, ga2, gc1, gphi, ghc, gd, gfc;
    size_t fin, fz1, fz2, fga1, fga2, onehot, gemb, part, total;
    int64_t wt_layer, n_slots, n_out, n_ch;
    EgnnLayout(int H, int L, int in_nf, int64_t Nn, int64_t E, bool keep) {
        const size_t n = (size_t)Nn, e = (size_t)(E > 0 ? E : 1), h = (size_t)H, KIN = 2 * h + 9;
        wt_layer = (int64_t)(h * (8 * h + 12));
        n_slots = keep ? L + 1 : 2;
        wt = take((size_t)L * wt_layer);
        F = take(n * 3);
        hs = take((size_t)n_slots * n * h);
        xs = take((size_t)n_slots * n * 3);
        agg = take(keep ? (size_t)L * n * h : 1);
        total_fwd = off;
        // weight-gradient partials: the larger of one layer's jobs and the field / embedding jobs
        const int64_t lay = (int64_t)(h * KIN + h + h * h + h + 2 * h * h + h + h * h + h + h * h + h + h + h * (h + 3) + h + h + 1);
        const int64_t fld = egnn::FH * egnn::FIN + egnn::FH + egnn::FH * egnn::FH + egnn::FH + 3 * egnn::FH + 3 + 3 * 16 +
                            (int64_t)H * in_nf + H;
        n_out = lay > fld ? lay : fld;
        const int64_t rows = E > Nn ? E : Nn;
        n_ch = (rows + 127) / 128;                              // >= 128 rows per chunk
        if (n_ch > egnn::WG_CH_MAX) n_ch = egnn::WG_CH_MAX;
        if (n_ch < 1) n_ch = 1;
        if (!keep) {
            gh = gx = gf = ghn = gagg = zn = gn1 = zp = gp1 = gpsi = gxm = gfn = ghe = gxe = gfe = 0;
            in = z1 = m = z3 = ga1 = ga2 = gc1 = gphi = ghc = gd = gfc = 0;
            fin = fz1 = fz2 = fga1 = fga2 = onehot = gemb = part = 0;
            total = off;
            return;
        }
        gh = take(2 * n * h); gx = take(2 * n * 3); gf = take(n * 3);
        ghn = take(n * h); gagg = take(n * h); zn = take(n * h); gn1 = take(n * h); zp = take(n * h); gp1 = take(n * h);
        gpsi = take(n); gxm = take(n * 3); gfn = take(n * 3); ghe = take(n * h); gxe = take(n * 3); gfe = take(n * 3);
        in = take(e * KIN); z1 = take(e * h); m = take(e * h); z3 = take(e * h);
        ga1 = take(e * h); ga2 = take(e * h); gc1 = take(e * h); gphi = take(e); ghc = take(e * h); gd = take(e * 3);
        gfc = take(e * 3);
        fin = take(n * egnn::FIN); fz1 = take(n * egnn::FH); fz2 = take(n * egnn::FH); fga1 = take(n * egnn::FH);
        fga2 = take(n * egnn::FH); onehot = take(n * 3); gemb = take(n * 16);
        part = take((size_t)n_ch * (size_t)n_out);
        total = off;
    }
};

struct EgnnCall : GraphView {
    int H, L, in_nf;
    bool norm, tanh_;
    int64_t Nn, E;
};

int egnn_check(const float* const* params, int n_params, int H, int L, int in_nf, int64_t Nn, int64_t E,
               const void* graph, const AetherGraphInfo* info, const char* what) {
    if (H != 64 && H != 128) return gnn_fail(AETHER_EINVAL, what, "hidden must be 64 or 128");
    if (L < 1 || L > 64) return gnn_fail(AETHER_EINVAL, what, "n_layers must lie in [1, 64]");
    if (in_nf < 1 || in_nf > 4096) return gnn_fail(AETHER_EINVAL, what, "in_node_nf must lie in [1, 4096]");
    return gnn_check(params, n_params, egnn_n_params(L), "parameter list does not match n_layers", 1, Nn, E, graph, info,
                     what);
}

EgnnCall egnn_call(int H, int L, int in_nf, int flags, int64_t Nn, int64_t E, const void* graph) {
    return EgnnCall{GraphView(graph, Nn, E), H, L, in_nf, (flags & AETHER_EGNN_NORM_DIFF) != 0,
                    (flags & AETHER_EGNN_TANH) != 0, Nn, E};
}

egnn::LayerW egnn_layer_w(const float* const* params, int l, const EgnnLayout& Lo, char* ws, int H) {
    const float* const* P = params + 2 + EGNN_PER_LAYER * l;
    float* wt = reinterpret_cast<float*>(ws + Lo.wt) + (size_t)l * Lo.wt_layer;
    const size_t KIN = 2 * H + 9, h = H;
    egnn::LayerW W;
    W.e_w0t = wt; W.e_w2t = wt + KIN * h; W.c_w0t = W.e_w2t + h * h; W.n_w0t = W.c_w0t + h * h;
    W.n_w2t = W.n_w0t + 2 * h * h; W.v_w0t = W.n_w2t + h * h;
    W.e_w0 = P[0]; W.e_b0 = P[1]; W.e_w2 = P[2]; W.e_b2 = P[3]; W.n_w0 = P[4]; W.n_b0 = P[5]; W.n_w2 = P[6];
    W.n_b2 = P[7]; W.c_w0 = P[8]; W.c_b0 = P[9]; W.c_w2 = P[10]; W.v_w0 = P[11]; W.v_b0 = P[12]; W.v_w2 = P[13];
    W.v_b2 = P[14];
    return W;
}

egnn::FieldW egnn_field_w(const float* const* params, int L) {
    const float* const* P = params + 2 + EGNN_PER_LAYER * L;
    egnn::FieldW f;
    f.w0 = P[0]; f.b0 = P[1]; f.w2 = P[2]; f.b2 = P[3]; f.w4 = P[4]; f.b4 = P[5]; f.emb = P[6];
    return f;
}

// transposed weight images, one launch per layer
template <int H>
void egnn_weight_images(const float* const* params, int L, const EgnnLayout& Lo, char* ws, hipStream_t st) {
    for (int l = 0; l < L; ++l) {
        const egnn::LayerW W = egnn_layer_w(params, l, Lo, ws, H);
        egnn::WtJob J;
        const float* const* P = params + 2 + EGNN_PER_LAYER * l;
        const int srcs[6] = {0, 2, 8, 4, 6, 11};
        const float* dsts[6] = {W.e_w0t, W.e_w2t, W.c_w0t, W.n_w0t, W.n_w2t, W.v_w0t};
        const int cols[6] = {2 * H + 9, H, H, 2 * H, H, H + 3};
        for (int q = 0; q < 6; ++q) { J.src[q] = P[srcs[q]]; J.dst[q] = const_cast<float*>(dsts[q]); J.cols[q] = cols[q]; }
        egnn::k_egnn_wt<H><<<dim3((unsigned)(((2 * H + 9) * H + 255) / 256), 6), dim3(256), 0, st>>>(J);
    }
}

// images: prepare the weight images first (a rollout prepares them once, in front of its first step)
template <int H>
int egnn_forward_impl(const EgnnCall& c, const float* const* params, const EgnnLayout& Lo, bool keep, const float* hin,
                      const float* x, const float* vel, const float* ea, const float* charges, char* ws, float* out,
                      hipStream_t st, bool images = true) {
    const int L = c.L;
    const int64_t Nn = c.Nn;
    const size_t h = H;
    const WsFloats wp{ws, Nn, H, Lo.hs, Lo.xs, Lo.gh, Lo.gx};
    float* F = wp(Lo.F);
    if (images) egnn_weight_images<H>(params, L, Lo, ws, st);
    egnn::k_egnn_prep<H><<<dim3((unsigned)Nn), dim3(H), 0, st>>>(egnn_field_w(params, L), params[0], params[1], c.in_nf, hin,
                                                                 x, vel, charges, F, wp.h(0));
    HIP_OK(hipMemcpyAsync(wp.x(0), x, (size_t)Nn * 3 * 4, hipMemcpyDeviceToDevice, st));
    for (int l = 0; l < L; ++l) {
        const int si = keep ? l : l % 2, so = keep ? l + 1 : (l + 1) % 2;
        const egnn::LayerW W = egnn_layer_w(params, l, Lo, ws, H);
        float* agg = keep ? wp(Lo.agg) + (size_t)l * Nn * h : nullptr;
        float* x2 = l == L - 1 ? out : nullptr;
        dispatch_bools([&](auto NORM, auto TANH) {
            egnn::k_egnn_layer<H, decltype(NORM)::value, decltype(TANH)::value><<<dim3((unsigned)Nn), dim3(H), 0, st>>>(
                W, wp.h(si), wp.x(si), vel, F, ea, c.perm, c.col_s, c.rowptr, wp.h(so), wp.x(so), x2, agg);
        }, c.norm, c.tanh_);
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int egnn_wgrad(gnn::WgJobs& T, const EgnnLayout& Lo, char* ws, hipStream_t st) {
    return gnn_wgrad(T, 64, 256, egnn::k_egnn_wgrad_part, reinterpret_cast<float*>(ws + Lo.part), Lo.n_out, Lo.n_ch,
                     "egnn: weight-gradient partials exceed their region", st);
}

template <int H>
int egnn_backward_impl(const EgnnCall& c, const float* const* params, const EgnnLayout& Lo, const float* hin,
                       const float* x, const float* vel, const float* ea, const float* charges, char* ws,
                       const float* grad_out, float* grad, hipStream_t st) {
    const int L = c.L, KIN = 2 * H + 9;
    const int64_t Nn = c.Nn, E = c.E;
    const size_t h = H;
    const WsFloats wp{ws, Nn, H, Lo.hs, Lo.xs, Lo.gh, Lo.gx};
    auto gdst = [&](int p) { return grad + egnn_grad_offset(p, H, L, c.in_nf); };
    float* F = wp(Lo.F);
    egnn::BwdBufs B;
    B.gf = wp(Lo.gf);
    B.ghn = wp(Lo.ghn); B.gagg = wp(Lo.gagg); B.zn = wp(Lo.zn); B.gn1 = wp(Lo.gn1); B.zp = wp(Lo.zp); B.gp1 = wp(Lo.gp1);
    B.gpsi = wp(Lo.gpsi); B.gxm = wp(Lo.gxm); B.gfn = wp(Lo.gfn); B.ghe = wp(Lo.ghe); B.gxe = wp(Lo.gxe); B.gfe = wp(Lo.gfe);
    B.in = wp(Lo.in); B.z1 = wp(Lo.z1); B.m = wp(Lo.m); B.z3 = wp(Lo.z3); B.ga1 = wp(Lo.ga1); B.ga2 = wp(Lo.ga2);
    B.gc1 = wp(Lo.gc1); B.gphi = wp(Lo.gphi); B.ghc = wp(Lo.ghc); B.gd = wp(Lo.gd); B.gfc = wp(Lo.gfc);
    HIP_OK(hipMemsetAsync(B.gf, 0, (size_t)Nn * 3 * 4, st));
    HIP_OK(hipMemsetAsync(wp.gh(0), 0, (size_t)Nn * h * 4, st));                 // the output x does not depend on h_L
    const dim3 nb((unsigned)Nn), tb(H);
    const float* gx_out = grad_out;
    for (int l = L - 1; l >= 0; --l) {
        const int cur = (L - 1 - l) % 2, nxt = 1 - cur;
        const float* gh_out = wp.gh(cur);
        B.gh_in = wp.gh(nxt);
        B.gx_in = wp.gx(nxt);
        const egnn::LayerW W = egnn_layer_w(params, l, Lo, ws, H);
        const float* hl = wp.h(l);
        const float* xl = wp.x(l);
        const float* aggl = wp(Lo.agg) + (size_t)l * Nn * h;
        egnn::kb_egnn_node<H><<<nb, tb, 0, st>>>(W, B, hl, aggl, vel, F, c.rowptr, gh_out, gx_out);
        dispatch_bools([&](auto NORM, auto TANH) {
            egnn::kb_egnn_edge<H, decltype(NORM)::value, decltype(TANH)::value><<<nb, tb, 0, st>>>(
                W, B, hl, xl, F, ea, c.perm, c.col_s, c.rowptr);
        }, c.norm, c.tanh_);
        egnn::kb_egnn_gather<H><<<nb, tb, 0, st>>>(B, gx_out, c.sperm, c.srowptr);
        // weight gradients of the layer (parameters 2 + 15 l ...)
        const int p0 = 2 + EGNN_PER_LAYER * l;
        WgTable J;
        J.add(B.ga1, H, B.in, KIN, 0, gdst(p0 + 0), KIN, H, KIN, E);            // edge_mlp.0
        J.add(B.ga1, H, nullptr, 0, 0, gdst(p0 + 1), 1, H, 1, E);
        J.add(B.ga2, H, B.z1, H, 0, gdst(p0 + 2), H, H, H, E);                  // edge_mlp.2
        J.add(B.ga2, H, nullptr, 0, 0, gdst(p0 + 3), 1, H, 1, E);
        J.add(B.gn1, H, hl, H, 0, gdst(p0 + 4), 2 * H, H, H, Nn);               // node_mlp.0: [h | agg]
        J.add(B.gn1, H, aggl, H, 0, gdst(p0 + 4) + H, 2 * H, H, H, Nn);
        J.add(B.gn1, H, nullptr, 0, 0, gdst(p0 + 5), 1, H, 1, Nn);
        J.add(gh_out, H, B.zn, H, 0, gdst(p0 + 6), H, H, H, Nn);                // node_mlp.2
        J.add(gh_out, H, nullptr, 0, 0, gdst(p0 + 7), 1, H, 1, Nn);
        J.add(B.gc1, H, B.m, H, 0, gdst(p0 + 8), H, H, H, E);                   // coord_mlp.0
        J.add(B.gc1, H, nullptr, 0, 0, gdst(p0 + 9), 1, H, 1, E);
        J.add(B.gphi, 1, B.z3, H, 0, gdst(p0 + 10), H, 1, H, E);                // coord_mlp.2 (no bias)
        J.add(B.gp1, H, hl, H, 0, gdst(p0 + 11), H + 3, H, H, Nn);              // coord_mlp_vel.0: [h | f]
        J.add(B.gp1, H, F, 3, 0, gdst(p0 + 11) + H, H + 3, H, 3, Nn);
        J.add(B.gp1, H, nullptr, 0, 0, gdst(p0 + 12), 1, H, 1, Nn);
        J.add(B.gpsi, 1, B.zp, H, 0, gdst(p0 + 13), H, 1, H, Nn);               // coord_mlp_vel.2
        J.add(B.gpsi, 1, nullptr, 0, 0, gdst(p0 + 14), 1, 1, 1, Nn);
        if (int rc = egnn_wgrad(J.T, Lo, ws, st)) return rc;
        gx_out = B.gx_in;
    }
    // field net (d/dF summed over the layers) and embedding (d/dh_0)
    const float* gh0 = wp.gh(L % 2);
    egnn::FieldBufs Fb;
    Fb.fin = wp(Lo.fin); Fb.z1 = wp(Lo.fz1); Fb.z2 = wp(Lo.fz2); Fb.ga1 = wp(Lo.fga1); Fb.ga2 = wp(Lo.fga2);
    Fb.onehot = wp(Lo.onehot); Fb.gemb = wp(Lo.gemb);
    egnn::kb_egnn_field<<<nb, dim3(64), 0, st>>>(egnn_field_w(params, L), Fb, x, vel, charges, B.gf);
    const int f0 = 2 + EGNN_PER_LAYER * L, FH = egnn::FH, FIN = egnn::FIN;
    WgTable J;
    J.add(gh0, H, hin, c.in_nf, 0, gdst(0), c.in_nf, H, c.in_nf, Nn);          // embedding
    J.add(gh0, H, nullptr, 0, 0, gdst(1), 1, H, 1, Nn);
    J.add(Fb.ga1, FH, Fb.fin, FIN, 0, gdst(f0 + 0), FIN, FH, FIN, Nn);          // field_net.net.0
    J.add(Fb.ga1, FH, nullptr, 0, 0, gdst(f0 + 1), 1, FH, 1, Nn);
    J.add(Fb.ga2, FH, Fb.z1, FH, 0, gdst(f0 + 2), FH, FH, FH, Nn);              // field_net.net.2
    J.add(Fb.ga2, FH, nullptr, 0, 0, gdst(f0 + 3), 1, FH, 1, Nn);
    J.add(B.gf, 3, Fb.z2, FH, 0, gdst(f0 + 4), FH, 3, FH, Nn);                  // field_net.net.4
    J.add(B.gf, 3, nullptr, 0, 0, gdst(f0 + 5), 1, 3, 1, Nn);
    J.add(Fb.onehot, 3, Fb.gemb, 16, 0, gdst(f0 + 6), 16, 3, 16, Nn);          // class_embedding
    if (int rc = egnn_wgrad(J.T, Lo, ws, st)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

}  // namespace
}  // extern "C++"

size_t aether_egnn_workspace_bytes(int hidden, int n_layers, int in_node_nf, int64_t n_nodes, int64_t n_edges,
                                   int keep_for_backward) {
    if (!egnn_sizes_ok(hidden, n_layers, in_node_nf) || n_nodes <= 0 || n_edges < 0) return 0;
    return EgnnLayout(hidden, n_layers, in_node_nf, n_nodes, n_edges, keep_for_backward != 0).total;
}

int64_t aether_egnn_grad_floats(int hidden, int n_layers, int in_node_nf) {
    if (!egnn_sizes_ok(hidden, n_layers, in_node_nf)) return AETHER_EINVAL;
    return egnn_grad_offset(egnn_n_params(n_layers), hidden, n_layers, in_node_nf);
}

int64_t aether_egnn_workspace_offset(const char* name, int layer, int hidden, int n_layers, int in_node_nf, int64_t n_nodes,
                                     int64_t n_edges) {
    if (!name || !egnn_sizes_ok(hidden, n_layers, in_node_nf) || n_nodes <= 0 || n_edges < 0)
        return fail(AETHER_EINVAL, "egnn_workspace_offset: bad arguments");
    const EgnnLayout Lo(hidden, n_layers, in_node_nf, n_nodes, n_edges, true);
    if (!strcmp(name, "field")) return (int64_t)Lo.F;
    return gnn_slot_offset("egnn_workspace_offset", "field, h, x", name, layer, n_layers, Lo.hs, Lo.xs, n_nodes, hidden);
}

int aether_egnn_forward(const float* const* params, int n_params, int hidden, int n_layers, int in_node_nf, int flags,
                        int64_t n_nodes, int64_t n_edges, const float* h, const float* x, const float* vel,
                        const float* edge_attr, const float* charges, const void* graph, const AetherGraphInfo* info,
                        void* workspace, size_t workspace_bytes, float* out, void* stream) {
    if (int rc = egnn_check(params, n_params, hidden, n_layers, in_node_nf, n_nodes, n_edges, graph, info, "egnn_forward"))
        return rc;
    const bool keep = (flags & AETHER_EGNN_KEEP) != 0;
    const EgnnLayout Lo(hidden, n_layers, in_node_nf, n_nodes, n_edges, keep);
    if (int rc = gnn_entry_check("egnn_forward",
                                 !h || !x || !vel || !charges || !workspace || !out || (n_edges > 0 && !edge_attr),
                                 flags & ~EGNN_FLAGS, workspace_bytes,
                                 Lo.total))
        return rc;
    const EgnnCall c = egnn_call(hidden, n_layers, in_node_nf, flags, n_nodes, n_edges, graph);
    hipStream_t st = (hipStream_t)stream;
    if (hidden == 64) return egnn_forward_impl<64>(c, params, Lo, keep, h, x, vel, edge_attr, charges, (char*)workspace, out, st);
    return egnn_forward_impl<128>(c, params, Lo, keep, h, x, vel, edge_attr, charges, (char*)workspace, out, st);
}

int aether_egnn_backward(const float* const* params, int n_params, int hidden, int n_layers, int in_node_nf, int flags,
                         int64_t n_nodes, int64_t n_edges, const float* h, const float* x, const float* vel,
                         const float* edge_attr, const float* charges, const void* graph, const AetherGraphInfo* info,
                         void* workspace, size_t workspace_bytes, const float* grad_out, float* grad, int64_t grad_floats,
                         void* stream) {
    if (int rc = egnn_check(params, n_params, hidden, n_layers, in_node_nf, n_nodes, n_edges, graph, info, "egnn_backward"))
        return rc;
    const EgnnLayout Lo(hidden, n_layers, in_node_nf, n_nodes, n_edges, true);
    if (int rc = gnn_entry_check("egnn_backward", !h || !x || !vel || !charges || !workspace || !grad_out || !grad ||
                                                      (n_edges > 0 && !edge_attr),
                                 flags & ~EGNN_FLAGS, workspace_bytes,
                                 Lo.total, grad_floats,
                                 egnn_grad_offset(egnn_n_params(n_layers), hidden, n_layers, in_node_nf)))
        return rc;
    const EgnnCall c = egnn_call(hidden, n_layers, in_node_nf, flags, n_nodes, n_edges, graph);
    hipStream_t st = (hipStream_t)stream;
    if (hidden == 64)
        return egnn_backward_impl<64>(c, params, Lo, h, x, vel, edge_attr, charges, (char*)workspace, grad_out, grad, st);
    return egnn_backward_impl<128>(c, params, Lo, h, x, vel, edge_attr, charges, (char*)workspace, grad_out, grad, st);
}

size_t aether_egnn_rollout_workspace_bytes(int hidden, int n_layers, int in_node_nf, int64_t n_nodes, int64_t n_edges) {
    if (!egnn_sizes_ok(hidden, n_layers, in_node_nf) || n_nodes <= 0 || n_edges < 0) return 0;
    return RolloutState(EgnnLayout(hidden, n_layers, in_node_nf, n_nodes, n_edges, false).total, n_nodes, n_edges).total;
}

extern "C++" {
namespace {

template <int H>
int egnn_rollout_impl(const EgnnCall& c, const float* const* params, const EgnnLayout& Lo, const RolloutState& R,
                      const float* x0, const float* vel0, const float* charges, const int64_t* send,
                      const int64_t* recv, char* ws, float* traj, int steps, float dt, hipStream_t st) {
    egnn_weight_images<H>(params, c.L, Lo, ws, st);
    return gnn_rollout(ws, R, c.Nn, c.E, x0, vel0, charges, send, recv, traj, steps, dt, st,
                       [&](const float* h, const float* x, const float* vel, const float* ea, float* out) {
                           return egnn_forward_impl<H>(c, params, Lo, false, h, x, vel, ea, charges, ws, out, st, false);
                       });
}

}  // namespace
}  // extern "C++"

int aether_egnn_rollout(const float* const* params, int n_params, int hidden, int n_layers, int in_node_nf, int flags,
                        int64_t n_nodes, int64_t n_edges, const float* x0, const float* vel0, const float* charges,
                        const int64_t* send, const int64_t* recv, const void* graph, const AetherGraphInfo* info,
                        void* workspace, size_t workspace_bytes, float* trajectory, int steps, float dt, void* stream) {
    if (int rc = egnn_check(params, n_params, hidden, n_layers, in_node_nf, n_nodes, n_edges, graph, info, "egnn_rollout"))
        return rc;
    const EgnnLayout Lo(hidden, n_layers, in_node_nf, n_nodes, n_edges, false);
    const RolloutState R(Lo.total, n_nodes, n_edges);
    if (int rc = gnn_rollout_check("egnn_rollout", in_node_nf, flags & AETHER_EGNN_KEEP,
                                   !x0 || !vel0 || !charges || !workspace || (steps > 0 && !trajectory) ||
                                       (n_edges > 0 && (!send || !recv)),
                                   flags & ~EGNN_FLAGS, workspace_bytes, R.total))
        return rc;
    if (steps <= 0) return 0;
    const EgnnCall c = egnn_call(hidden, n_layers, in_node_nf, flags, n_nodes, n_edges, graph);
    hipStream_t st = (hipStream_t)stream;
    if (hidden == 64)
        return egnn_rollout_impl<64>(c, params, Lo, R, x0, vel0, charges, send, recv, (char*)workspace, trajectory, steps, dt, st);
    return egnn_rollout_impl<128>(c, params, Lo, R, x0, vel0, charges, send, recv, (char*)workspace, trajectory, steps, dt, st);
}
