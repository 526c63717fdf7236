// Host side of the C ABI: ClofNet (ClofNet / ClofNet_vel / ClofNet_vel_gbf, nn/state2state/clof/clof.py), forward and
// parameter backward.  Included by aether_hip.hip inside its extern "C" block; not a stand-alone source file.
// Kernels: csrc/clof.h; shared plumbing: csrc/host_gnn_common.inc.

extern "C++" {
namespace {

constexpr int CLOF_FLAGS = AETHER_CLOF_NORM_DIFF | AETHER_CLOF_TANH | AETHER_CLOF_KEEP | AETHER_CLOF_RECURRENT;
constexpr int CLOF_PER_LAYER = 19;   // edge_mlp.{0,2,4} w b, node_mlp.{0,2} w b, coord_mlp.0 w b, coord_mlp.2 w,
                                     // coord_mlp_vel.{0,2} w b, layer_norm w b
// head tensors before gcl_0: embedding_node w b, then ClofNet: embedding_edge.0 w b, fuse_edge.{0,2} w b;
// ClofNet_vel: fuse_edge.{0,2} w b; ClofNet_vel_gbf: gbf.{means,stds,mul,bias}.weight, fuse_edge.{0,2} w b
int clof_head(int variant) { return variant == 0 ? 8 : (variant == 1 ? 6 : 10); }
int clof_fuse_in(int variant) { return variant == 0 ? 10 : (variant == 1 ? 16 : 14); }
int clof_fuse0(int variant) { return variant == 0 ? 4 : (variant == 1 ? 2 : 6); }     // index of fuse_edge.0.weight
int clof_n_params(int variant, int L) { return clof_head(variant) + CLOF_PER_LAYER * L; }
int64_t clof_kin(int H) { return 2LL * H + 1 + H / 2; }

int64_t clof_numel(int p, int variant, int H, int L, int in_nf) {
    const int64_t h = H, h2 = H / 2, F = clof_fuse_in(variant);
    const int nh = clof_head(variant);
    if (p < nh) {
        if (p == 0) return h * in_nf;
        if (p == 1) return h;
        if (variant == 0 && p < 4) return p == 2 ? 16 : 8;                       // embedding_edge.0: Linear(2, 8)
        if (variant == 2 && p < 6) return p < 4 ? h2 : clof::NTYPES;             // means, stds [1][K]; mul, bias [8][1]
        const int f = p - clof_fuse0(variant);
        const int64_t fs[4] = {h2 * F, h2, h2 * h2, h2};
        return fs[f];
    }
    (void)L;
    const int64_t sz[CLOF_PER_LAYER] = {h * clof_kin(H), h, h * h, h, h * h, h, 2 * h * h, h, h * h, h, h * h, h, 3 * h,
                                        h * h, h, h, 1, h, h};
    return sz[(p - nh) % CLOF_PER_LAYER];
}

int64_t clof_grad_offset(int p, int variant, int H, int L, int in_nf) {
    return gnn_grad_offset(p, [&](int q) { return clof_numel(q, variant, H, L, in_nf); });
}

struct ClofLayout : FloatArena {
    size_t wimg, cen, hs, xs, P, ef, m, trans;
    size_t fin, af1, af2, a1, a2, a3, ac1, rad, av, an1, agg, xhat, rstd;
    size_t gx, gh, gtr, gav, gpsi, gu, gn1, glnw, gagg, ghp, ga1, ga2, ga3, gac1, gc, gef, gxr, gxc, srow, scol;
    size_t gaf1, gaf2, gmean, gstd, gmul, gbias, part, total;
    int64_t img_layer, n_slots, n_out, n_ch;
    ClofLayout(int variant, int H, int L, int in_nf, int64_t Nn, int64_t E, bool keep) {
        const size_t n = (size_t)Nn, e = (size_t)(E > 0 ? E : 1), h = (size_t)H, h2 = h / 2, l = (size_t)L;
        img_layer = (int64_t)(13 * h * h + h);
        n_slots = keep ? L + 1 : 2;
        wimg = take(l * (size_t)img_layer);
        cen = take(n * 3);
        hs = take((size_t)n_slots * n * h);
        xs = take((size_t)n_slots * n * 3);
        P = take(n * 2 * h);
        ef = take(e * h2);
        m = take(e * h);
        trans = take(e * 3);
        int64_t lay = 0, head = 0;
        const int nh = clof_head(variant);
        for (int p = 0; p < nh; ++p) head += clof_numel(p, variant, H, L, in_nf);
        for (int p = nh; p < nh + CLOF_PER_LAYER; ++p) lay += clof_numel(p, variant, H, L, in_nf);
        n_out = lay > head ? lay : head;
        const int64_t rows = E > Nn ? E : Nn;
        n_ch = (rows + 255) / 256;
        if (n_ch > clof::WG_CH_MAX) n_ch = clof::WG_CH_MAX;
        if (n_ch < 1) n_ch = 1;
        if (!keep) {
            fin = af1 = af2 = a1 = a2 = a3 = ac1 = rad = av = an1 = agg = xhat = rstd = 0;
            gx = gh = gtr = gav = gpsi = gu = gn1 = glnw = gagg = ghp = ga1 = ga2 = ga3 = gac1 = gc = gef = gxr = gxc = 0;
            srow = scol = gaf1 = gaf2 = gmean = gstd = gmul = gbias = part = 0;
            total = off;
            return;
        }
        fin = take(e * clof::FMAX); af1 = take(e * h2); af2 = take(e * h2);
        a1 = take(l * e * h); a2 = take(l * e * h); a3 = take(l * e * h); ac1 = take(l * e * h); rad = take(l * e);
        av = take(l * n * h); an1 = take(l * n * h); agg = take(l * n * h); xhat = take(l * n * h); rstd = take(l * n);
        gx = take(2 * n * 3); gh = take(2 * n * h); gtr = take(n * 3); gav = take(n * h); gpsi = take(n);
        gu = take(n * h); gn1 = take(n * h); glnw = take(n * h); gagg = take(n * h); ghp = take(n * h);
        ga1 = take(e * h); ga2 = take(e * h); ga3 = take(e * h); gac1 = take(e * h); gc = take(e * 3); gef = take(e * h2);
        gxr = take(e * 3); gxc = take(e * 3); srow = take(n * h); scol = take(n * h);
        gaf1 = take(e * h2); gaf2 = take(e * h2); gmean = take(e * h2); gstd = take(e * h2);
        gmul = take(e * clof::NTYPES); gbias = take(e * clof::NTYPES);
        part = take((size_t)n_ch * (size_t)n_out);
        total = off;
    }
};

struct ClofCall : GraphView {
    int variant, H, L, in_nf, n_per, recurrent;
    bool norm, tanh_;
    float cw;
    int64_t Nn, E;
};

bool clof_sizes_ok(int variant, int H, int L, int in_nf) {
    return variant >= 0 && variant <= 2 && (H == 64 || H == 128) && L >= 1 && L <= 64 && in_nf >= 1 && in_nf <= 4096;
}

int clof_check(const float* const* params, int n_params, int variant, int H, int L, int in_nf, int n_per, int64_t Nn,
               int64_t E, const void* graph, const AetherGraphInfo* info, const char* what) {
    if (!clof_sizes_ok(variant, H, L, in_nf))
        return gnn_fail(AETHER_EINVAL, what,
                        "variant must be 0..2, hidden 64 or 128, n_layers in [1, 64], in_node_nf in [1, 4096]");
    return gnn_check(params, n_params, clof_n_params(variant, L), "parameter list does not match variant / n_layers", n_per,
                     Nn, E, graph, info, what);
}

ClofCall clof_call(int variant, int H, int L, int in_nf, int flags, float cw, int n_per, int64_t Nn, int64_t E,
                   const void* graph) {
    return ClofCall{GraphView(graph, Nn, E), variant, H, L, in_nf, n_per, (flags & AETHER_CLOF_RECURRENT) != 0 ? 1 : 0,
                    (flags & AETHER_CLOF_NORM_DIFF) != 0, (flags & AETHER_CLOF_TANH) != 0, cw, Nn, E};
}

// layer l's packed images (offsets inside its image block) and tensors
clof::LayerW clof_layer_w(const float* const* params, int variant, int l, const ClofLayout& Lo, char* ws, int H) {
    const float* const* P = params + clof_head(variant) + CLOF_PER_LAYER * l;
    const float* im = reinterpret_cast<const float*>(ws + Lo.wimg) + (size_t)l * Lo.img_layer;
    const size_t h = H, hh = h * h;
    clof::LayerW W;
    W.w0ef = im; W.w0eft = im + hh / 2; W.w2 = im + hh; W.w2t = im + 2 * hh; W.w4 = im + 3 * hh; W.w4t = im + 4 * hh;
    W.wc0 = im + 5 * hh; W.wc0t = im + 6 * hh; W.w0rt = im + 7 * hh; W.w0ct = im + 8 * hh; W.wv0t = im + 9 * hh;
    W.wn0t = im + 10 * hh; W.wn2t = im + 12 * hh; W.wrad = im + 13 * hh;
    W.e_w0 = P[0]; W.e_b0 = P[1]; W.e_b2 = P[3]; W.e_b4 = P[5]; W.n_w0 = P[6]; W.n_b0 = P[7]; W.n_w2 = P[8];
    W.n_b2 = P[9]; W.c_b0 = P[11]; W.c_w2 = P[12]; W.v_w0 = P[13]; W.v_b0 = P[14]; W.v_w2 = P[15]; W.v_b2 = P[16];
    W.ln_w = P[17]; W.ln_b = P[18];
    return W;
}

void clof_pack_layer(const float* const* params, int variant, int l, const ClofLayout& Lo, char* ws, int H, hipStream_t st) {
    const float* const* P = params + clof_head(variant) + CLOF_PER_LAYER * l;
    const clof::LayerW W = clof_layer_w(params, variant, l, Lo, ws, H);
    const int KIN = (int)clof_kin(H), H2 = H / 2;
    clof::PackJobs T;
    T.n = 0;
    auto job = [&](const float* src, const float* dst, int lds, int c0, int A, int B, int trans) {
        clof::PackJob& j = T.j[T.n++];
        j.src = src; j.dst = const_cast<float*>(dst); j.lds = lds; j.c0 = c0; j.A = A; j.B = B; j.trans = trans;
    };
    job(P[0], W.w0ef, KIN, 2 * H + 1, H, H2, 0);      // edge_mlp.0, edge_feat columns: [H][H/2] and [H/2][H]
    job(P[0], W.w0eft, KIN, 2 * H + 1, H2, H, 1);
    job(P[2], W.w2, H, 0, H, H, 0);
    job(P[2], W.w2t, H, 0, H, H, 1);
    job(P[4], W.w4, H, 0, H, H, 0);
    job(P[4], W.w4t, H, 0, H, H, 1);
    job(P[10], W.wc0, H, 0, H, H, 0);
    job(P[10], W.wc0t, H, 0, H, H, 1);
    job(P[0], W.w0rt, KIN, 0, H, H, 1);               // h_row / h_col blocks, [in][out] for the node products
    job(P[0], W.w0ct, KIN, H, H, H, 1);
    job(P[13], W.wv0t, H, 0, H, H, 1);
    job(P[6], W.wn0t, 2 * H, 0, 2 * H, H, 1);
    job(P[8], W.wn2t, H, 0, H, H, 1);
    job(P[0], W.wrad, KIN, 2 * H, H, 1, 0);           // radial column
    clof::k_clof_pack<<<dim3((unsigned)((2 * H * H + 255) / 256), (unsigned)T.n), dim3(256), 0, st>>>(T);
}

clof::ProW clof_pro_w(const float* const* params, int variant) {
    clof::ProW w;
    const int f0 = clof_fuse0(variant);
    w.f_w0 = params[f0]; w.f_b0 = params[f0 + 1]; w.f_w2 = params[f0 + 2]; w.f_b2 = params[f0 + 3];
    w.g_means = w.g_stds = w.g_mul = w.g_bias = nullptr;
    if (variant == 2) { w.g_means = params[2]; w.g_stds = params[3]; w.g_mul = params[4]; w.g_bias = params[5]; }
    return w;
}

template <int H>
int clof_forward_impl(const ClofCall& c, const float* const* params, const ClofLayout& Lo, bool keep, const float* hin,
                      const float* x, const float* vel, const float* ea, char* ws, float* out, hipStream_t st,
                      bool images = true) {
    const int L = c.L, v = c.variant;
    const int64_t Nn = c.Nn, E = c.E;
    const size_t h = H;
    const WsFloats wp{ws, Nn, H, Lo.hs, Lo.xs, Lo.gh, Lo.gx};
    if (images)                       // a rollout packs them once, in front of its first step
        for (int l = 0; l < L; ++l) clof_pack_layer(params, v, l, Lo, ws, H, st);
    const unsigned nb = (unsigned)((Nn + clof::NB - 1) / clof::NB);
    clof::k_clof_prep<H><<<dim3(nb), dim3(H), 0, st>>>(clof_layer_w(params, v, 0, Lo, ws, H), params[0], params[1], c.in_nf,
                                                        c.n_per, Nn, hin, x, wp.x(0), wp(Lo.cen), wp.h(0), wp(Lo.P));
    if (E > 0) {
        const clof::ProW pw = clof_pro_w(params, v);
        const dim3 eg((unsigned)((E + 63) / 64));
        float *fin = keep ? wp(Lo.fin) : nullptr, *af1 = keep ? wp(Lo.af1) : nullptr, *af2 = keep ? wp(Lo.af2) : nullptr;
        auto pro = [&](auto VAR, auto NORM, auto KEEP) {
            clof::k_clof_prologue<H, decltype(VAR)::value, decltype(NORM)::value, decltype(KEEP)::value>
                <<<eg, dim3(64), 0, st>>>(pw, E, c.perm, c.row_s, c.col_s, wp.x(0), vel, ea, wp(Lo.ef), fin, af1, af2);
        };
        // ClofNet_vel / _gbf scalarize with norm_diff = True whatever the argument (clof.py:113,190); ClofNet uses it
        using std::integral_constant;
        if (v == 0) dispatch_bools([&](auto NORM, auto KEEP) { pro(integral_constant<int, 0>{}, NORM, KEEP); }, c.norm, keep);
        else if (v == 1) dispatch_bools([&](auto KEEP) { pro(integral_constant<int, 1>{}, std::true_type{}, KEEP); }, keep);
        else dispatch_bools([&](auto KEEP) { pro(integral_constant<int, 2>{}, std::true_type{}, KEEP); }, keep);
    }
    const dim3 eb((unsigned)((E + clof::ET - 1) / clof::ET)), et(64 * clof::EW);
    for (int l = 0; l < L; ++l) {
        const int si = keep ? l : l % 2, so = keep ? l + 1 : (l + 1) % 2;
        const clof::LayerW W = clof_layer_w(params, v, l, Lo, ws, H);
        const clof::LayerW Wn = clof_layer_w(params, v, l + 1 < L ? l + 1 : l, Lo, ws, H);
        if (E > 0) {
            clof::EdgeBufs B;
            B.x = wp.x(si); B.P = wp(Lo.P); B.ef = wp(Lo.ef); B.m = wp(Lo.m); B.trans = wp(Lo.trans);
            const size_t eo = (size_t)l * E * h;
            B.a1 = keep ? wp(Lo.a1) + eo : nullptr; B.a2 = keep ? wp(Lo.a2) + eo : nullptr;
            B.a3 = keep ? wp(Lo.a3) + eo : nullptr; B.ac1 = keep ? wp(Lo.ac1) + eo : nullptr;
            B.rad = keep ? wp(Lo.rad) + (size_t)l * E : nullptr;
            dispatch_bools([&](auto NORM, auto TANH, auto KEEP) {
                clof::k_clof_edge<H, decltype(NORM)::value, decltype(TANH)::value, decltype(KEEP)::value>
                    <<<eb, et, 0, st>>>(W, B, E, c.row_s, c.col_s);
            }, c.norm, c.tanh_, keep);
        }
        clof::NodeBufs N;
        N.h = wp.h(si); N.x = wp.x(si); N.vel = vel; N.m = wp(Lo.m); N.trans = wp(Lo.trans); N.cen = wp(Lo.cen);
        N.h2 = wp.h(so); N.x2 = wp.x(so); N.out = out; N.P = wp(Lo.P);
        const size_t no = (size_t)l * Nn * h;
        N.av = keep ? wp(Lo.av) + no : nullptr; N.an1 = keep ? wp(Lo.an1) + no : nullptr;
        N.agg = keep ? wp(Lo.agg) + no : nullptr; N.xhat = keep ? wp(Lo.xhat) + no : nullptr;
        N.rstd = keep ? wp(Lo.rstd) + (size_t)l * Nn : nullptr;
        const bool last = l == L - 1;
        dispatch_bools([&](auto LAST, auto KEEP) {
            clof::k_clof_node<H, decltype(LAST)::value, decltype(KEEP)::value><<<dim3(nb), dim3(H), 0, st>>>(
                W, Wn, N, c.cw, c.recurrent, Nn, c.rowptr);
        }, last, keep);
    }
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

int clof_wgrad(gnn::WgJobs& T, const ClofLayout& Lo, char* ws, hipStream_t st) {
    return gnn_wgrad(T, 32, 64, clof::k_clof_wgrad_part, reinterpret_cast<float*>(ws + Lo.part), Lo.n_out, Lo.n_ch,
                     "clof: weight-gradient partials exceed their region", st);
}

template <int H>
int clof_backward_impl(const ClofCall& c, const float* const* params, const ClofLayout& Lo, const float* hin,
                       const float* vel, const float* ea, char* ws, const float* grad_out, float* grad, hipStream_t st) {
    const int L = c.L, v = c.variant, KIN = (int)clof_kin(H), H2 = H / 2;
    const int64_t Nn = c.Nn, E = c.E;
    const size_t h = H;
    const WsFloats wp{ws, Nn, H, Lo.hs, Lo.xs, Lo.gh, Lo.gx};
    auto gdst = [&](int p) { return grad + clof_grad_offset(p, v, H, L, c.in_nf); };
    const unsigned nb = (unsigned)((Nn + clof::NB - 1) / clof::NB);
    const dim3 eb((unsigned)((E + clof::ET - 1) / clof::ET)), et(64 * clof::EW);
    const float* gx_out = grad_out;
    const float* gh_out = nullptr;
    for (int l = L - 1; l >= 0; --l) {
        const int s = (L - 1 - l) % 2;
        const bool last = l == L - 1, first = l == 0;
        const clof::LayerW W = clof_layer_w(params, v, l, Lo, ws, H);
        const size_t eo = (size_t)l * E * h, no = (size_t)l * Nn * h;
        const float* hl = wp.h(l);
        clof::BNodeBufs BN;
        BN.gx = gx_out; BN.gh = gh_out; BN.h = hl; BN.vel = vel; BN.av = wp(Lo.av) + no; BN.an1 = wp(Lo.an1) + no;
        BN.xhat = wp(Lo.xhat) + no; BN.rstd = wp(Lo.rstd) + (size_t)l * Nn;
        BN.gtr = wp(Lo.gtr); BN.gav = wp(Lo.gav); BN.gpsi = wp(Lo.gpsi); BN.gu = wp(Lo.gu); BN.gn1 = wp(Lo.gn1);
        BN.glnw = wp(Lo.glnw); BN.gagg = wp(Lo.gagg); BN.ghp = wp(Lo.ghp);
        dispatch_bools([&](auto LAST) {
            clof::kb_clof_node<H, decltype(LAST)::value><<<dim3(nb), dim3(H), 0, st>>>(W, BN, c.cw, c.recurrent, Nn, c.rowptr);
        }, last);
        if (E > 0) {
            clof::BEdgeBufs BE;
            BE.x = wp.x(l); BE.a1 = wp(Lo.a1) + eo; BE.a2 = wp(Lo.a2) + eo; BE.a3 = wp(Lo.a3) + eo; BE.ac1 = wp(Lo.ac1) + eo;
            BE.gtr = wp(Lo.gtr); BE.gagg = wp(Lo.gagg);
            BE.ga1 = wp(Lo.ga1); BE.ga2 = wp(Lo.ga2); BE.ga3 = wp(Lo.ga3); BE.gac1 = wp(Lo.gac1); BE.gc = wp(Lo.gc);
            BE.gef = wp(Lo.gef); BE.gxr = wp(Lo.gxr); BE.gxc = wp(Lo.gxc);
            const int top = last ? 1 : 0, fst = first ? 1 : 0;
            dispatch_bools([&](auto NORM, auto TANH) {
                clof::kb_clof_edge<H, decltype(NORM)::value, decltype(TANH)::value><<<eb, et, 0, st>>>(
                    W, BE, E, c.row_s, c.col_s, top, fst);
            }, c.norm, c.tanh_);
        }
        clof::BGatherBufs BG;
        BG.ga1 = wp(Lo.ga1); BG.ghp = wp(Lo.ghp); BG.gx = gx_out; BG.gxr = wp(Lo.gxr); BG.gxc = wp(Lo.gxc);
        BG.srow = wp(Lo.srow); BG.scol = wp(Lo.scol); BG.gh = wp.gh(s); BG.gxo = wp.gx(s);
        clof::kb_clof_gather<H><<<dim3(nb), dim3(H), 0, st>>>(W, BG, KIN, Nn, c.rowptr, c.sperm, c.srowptr,
                                                              first ? 1 : 0);
        // weight gradients of layer l (parameters p0 ...); the last layer's node_mlp and layer_norm are dead
        const int p0 = clof_head(v) + CLOF_PER_LAYER * l, SILU = 1;
        WgTable J;
        J.add(wp(Lo.srow), H, hl, H, 0, gdst(p0), KIN, H, H, Nn);                           // edge_mlp.0: h_row, h_col
        J.add(wp(Lo.scol), H, hl, H, 0, gdst(p0) + H, KIN, H, H, Nn);
        J.add(wp(Lo.ga1), H, wp(Lo.rad) + (size_t)l * E, 1, 0, gdst(p0) + 2 * H, KIN, H, 1, E);   // radial
        J.add(wp(Lo.ga1), H, wp(Lo.ef), H2, 0, gdst(p0) + 2 * H + 1, KIN, H, H2, E);       // edge_feat
        J.add(wp(Lo.ga1), H, nullptr, 0, 0, gdst(p0 + 1), 1, H, 1, E);
        J.add(wp(Lo.ga2), H, wp(Lo.a1) + eo, H, SILU, gdst(p0 + 2), H, H, H, E);          // edge_mlp.2
        J.add(wp(Lo.ga2), H, nullptr, 0, 0, gdst(p0 + 3), 1, H, 1, E);
        J.add(wp(Lo.ga3), H, wp(Lo.a2) + eo, H, SILU, gdst(p0 + 4), H, H, H, E);          // edge_mlp.4
        J.add(wp(Lo.ga3), H, nullptr, 0, 0, gdst(p0 + 5), 1, H, 1, E);
        if (!last) {
            J.add(wp(Lo.gn1), H, hl, H, 0, gdst(p0 + 6), 2 * H, H, H, Nn);                 // node_mlp.0: [h | agg]
            J.add(wp(Lo.gn1), H, wp(Lo.agg) + no, H, 0, gdst(p0 + 6) + H, 2 * H, H, H, Nn);
            J.add(wp(Lo.gn1), H, nullptr, 0, 0, gdst(p0 + 7), 1, H, 1, Nn);
            J.add(wp(Lo.gu), H, wp(Lo.an1) + no, H, SILU, gdst(p0 + 8), H, H, H, Nn);      // node_mlp.2
            J.add(wp(Lo.gu), H, nullptr, 0, 0, gdst(p0 + 9), 1, H, 1, Nn);
        }
        J.add(wp(Lo.gac1), H, wp(Lo.a3) + eo, H, SILU, gdst(p0 + 10), H, H, H, E);        // coord_mlp.0
        J.add(wp(Lo.gac1), H, nullptr, 0, 0, gdst(p0 + 11), 1, H, 1, E);
        J.add(wp(Lo.gc), 3, wp(Lo.ac1) + eo, H, SILU, gdst(p0 + 12), H, 3, H, E);         // coord_mlp.2
        J.add(wp(Lo.gav), H, hl, H, 0, gdst(p0 + 13), H, H, H, Nn);                        // coord_mlp_vel.0
        J.add(wp(Lo.gav), H, nullptr, 0, 0, gdst(p0 + 14), 1, H, 1, Nn);
        J.add(wp(Lo.gpsi), 1, wp(Lo.av) + no, H, SILU, gdst(p0 + 15), H, 1, H, Nn);        // coord_mlp_vel.2
        J.add(wp(Lo.gpsi), 1, nullptr, 0, 0, gdst(p0 + 16), 1, 1, 1, Nn);
        if (!last) {
            J.add(wp(Lo.glnw), H, nullptr, 0, 0, gdst(p0 + 17), 1, H, 1, Nn);             // layer_norm
            J.add(gh_out, H, nullptr, 0, 0, gdst(p0 + 18), 1, H, 1, Nn);
        }
        if (int rc = clof_wgrad(J.T, Lo, ws, st)) return rc;
        gx_out = wp.gx(s);
        gh_out = wp.gh(s);
    }
    // the prologue: edge_feat's gradient (summed over the layers) through fuse_edge and the Gaussian layer
    const int F = clof_fuse_in(v), f0 = clof_fuse0(v), SILU = 1;
    if (E > 0) {
        clof::BProBufs BP;
        BP.gef = wp(Lo.gef); BP.fin = wp(Lo.fin); BP.af1 = wp(Lo.af1); BP.af2 = wp(Lo.af2); BP.ea = ea;
        BP.gaf1 = wp(Lo.gaf1); BP.gaf2 = wp(Lo.gaf2); BP.gmean = wp(Lo.gmean); BP.gstd = wp(Lo.gstd);
        BP.gmul = wp(Lo.gmul); BP.gbias = wp(Lo.gbias);
        const clof::ProW pw = clof_pro_w(params, v);
        const dim3 eg((unsigned)((E + 63) / 64));
        if (v == 2) clof::kb_clof_prologue<H, 2><<<eg, dim3(64), 0, st>>>(pw, BP, F, E, c.perm);
        else clof::kb_clof_prologue<H, 0><<<eg, dim3(64), 0, st>>>(pw, BP, F, E, c.perm);
    }
    WgTable J;
    J.add(gh_out, H, hin, c.in_nf, 0, gdst(0), c.in_nf, H, c.in_nf, Nn);                   // embedding_node
    J.add(gh_out, H, nullptr, 0, 0, gdst(1), 1, H, 1, Nn);
    const int64_t re = E > 0 ? E : 0;
    J.add(wp(Lo.gaf1), H2, wp(Lo.fin), clof::FMAX, 0, gdst(f0), F, H2, F, re);             // fuse_edge.0
    J.add(wp(Lo.gaf1), H2, nullptr, 0, 0, gdst(f0 + 1), 1, H2, 1, re);
    J.add(wp(Lo.gaf2), H2, wp(Lo.af1), H2, SILU, gdst(f0 + 2), H2, H2, H2, re);           // fuse_edge.2
    J.add(wp(Lo.gaf2), H2, nullptr, 0, 0, gdst(f0 + 3), 1, H2, 1, re);
    if (v == 2) {                                                                         // gbf.{means,stds,mul,bias}
        J.add(wp(Lo.gmean), H2, nullptr, 0, 0, gdst(2), 1, H2, 1, re);
        J.add(wp(Lo.gstd), H2, nullptr, 0, 0, gdst(3), 1, H2, 1, re);
        J.add(wp(Lo.gmul), clof::NTYPES, nullptr, 0, 0, gdst(4), 1, clof::NTYPES, 1, re);
        J.add(wp(Lo.gbias), clof::NTYPES, nullptr, 0, 0, gdst(5), 1, clof::NTYPES, 1, re);
    }
    if (int rc = clof_wgrad(J.T, Lo, ws, st)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

}  // namespace
}  // extern "C++"

size_t aether_clof_workspace_bytes(int variant, int hidden, int n_layers, int in_node_nf, int64_t n_nodes, int64_t n_edges,
                                   int keep_for_backward) {
    if (!clof_sizes_ok(variant, hidden, n_layers, in_node_nf) || n_nodes <= 0 || n_edges < 0) return 0;
    return ClofLayout(variant, hidden, n_layers, in_node_nf, n_nodes, n_edges, keep_for_backward != 0).total;
}

int64_t aether_clof_grad_floats(int variant, int hidden, int n_layers, int in_node_nf) {
    if (!clof_sizes_ok(variant, hidden, n_layers, in_node_nf)) return AETHER_EINVAL;
    return clof_grad_offset(clof_n_params(variant, n_layers), variant, hidden, n_layers, in_node_nf);
}

int64_t aether_clof_workspace_offset(const char* name, int layer, int variant, int hidden, int n_layers, int in_node_nf,
                                     int64_t n_nodes, int64_t n_edges) {
    if (!name || !clof_sizes_ok(variant, hidden, n_layers, in_node_nf) || n_nodes <= 0 || n_edges < 0)
        return fail(AETHER_EINVAL, "clof_workspace_offset: bad arguments");
    const ClofLayout Lo(variant, hidden, n_layers, in_node_nf, n_nodes, n_edges, true);
    if (!strcmp(name, "edge_feat")) return (int64_t)Lo.ef;
    return gnn_slot_offset("clof_workspace_offset", "edge_feat, h, x", name, layer, n_layers, Lo.hs, Lo.xs, n_nodes, hidden);
}

int aether_clof_forward(const float* const* params, int n_params, int variant, int hidden, int n_layers, int in_node_nf,
                        int flags, float coords_weight, int n_per_graph, int64_t n_nodes, int64_t n_edges, const float* h,
                        const float* x, const float* vel, const float* edge_attr, const void* graph,
                        const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, float* out, void* stream) {
    if (int rc = clof_check(params, n_params, variant, hidden, n_layers, in_node_nf, n_per_graph, n_nodes, n_edges, graph,
                            info, "clof_forward"))
        return rc;
    const bool keep = (flags & AETHER_CLOF_KEEP) != 0;
    const ClofLayout Lo(variant, hidden, n_layers, in_node_nf, n_nodes, n_edges, keep);
    if (int rc = gnn_entry_check("clof_forward", !h || !x || !vel || !workspace || !out || (n_edges > 0 && !edge_attr),
                                 flags & ~CLOF_FLAGS, workspace_bytes, Lo.total))
        return rc;
    const ClofCall c = clof_call(variant, hidden, n_layers, in_node_nf, flags, coords_weight, n_per_graph, n_nodes, n_edges,
                                 graph);
    hipStream_t st = (hipStream_t)stream;
    if (hidden == 64) return clof_forward_impl<64>(c, params, Lo, keep, h, x, vel, edge_attr, (char*)workspace, out, st);
    return clof_forward_impl<128>(c, params, Lo, keep, h, x, vel, edge_attr, (char*)workspace, out, st);
}

int aether_clof_backward(const float* const* params, int n_params, int variant, int hidden, int n_layers, int in_node_nf,
                         int flags, float coords_weight, int n_per_graph, int64_t n_nodes, int64_t n_edges, const float* h,
                         const float* x, const float* vel, const float* edge_attr, const void* graph,
                         const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* grad_out,
                         float* grad, int64_t grad_floats, void* stream) {
    if (int rc = clof_check(params, n_params, variant, hidden, n_layers, in_node_nf, n_per_graph, n_nodes, n_edges, graph,
                            info, "clof_backward"))
        return rc;
    const ClofLayout Lo(variant, hidden, n_layers, in_node_nf, n_nodes, n_edges, true);
    if (int rc = gnn_entry_check("clof_backward",
                                 !h || !x || !vel || !workspace || !grad_out || !grad || (n_edges > 0 && !edge_attr),
                                 flags & ~CLOF_FLAGS, workspace_bytes, Lo.total, grad_floats,
                                 clof_grad_offset(clof_n_params(variant, n_layers), variant, hidden, n_layers, in_node_nf)))
        return rc;
    const ClofCall c = clof_call(variant, hidden, n_layers, in_node_nf, flags, coords_weight, n_per_graph, n_nodes, n_edges,
                                 graph);
    hipStream_t st = (hipStream_t)stream;
    if (hidden == 64)
        return clof_backward_impl<64>(c, params, Lo, h, vel, edge_attr, (char*)workspace, grad_out, grad, st);
    return clof_backward_impl<128>(c, params, Lo, h, vel, edge_attr, (char*)workspace, grad_out, grad, st);
}

size_t aether_clof_rollout_workspace_bytes(int variant, int hidden, int n_layers, int in_node_nf, int64_t n_nodes,
                                           int64_t n_edges) {
    if (!clof_sizes_ok(variant, hidden, n_layers, in_node_nf) || n_nodes <= 0 || n_edges < 0) return 0;
    return RolloutState(ClofLayout(variant, hidden, n_layers, in_node_nf, n_nodes, n_edges, false).total, n_nodes, n_edges)
        .total;
}

extern "C++" {
namespace {

template <int H>
int clof_rollout_impl(const ClofCall& c, const float* const* params, const ClofLayout& Lo, const RolloutState& R,
                      const float* x0, const float* vel0, const float* charges, const int64_t* send,
                      const int64_t* recv, char* ws, float* traj, int steps, float dt, hipStream_t st) {
    for (int l = 0; l < c.L; ++l) clof_pack_layer(params, c.variant, l, Lo, ws, H, st);
    return gnn_rollout(ws, R, c.Nn, c.E, x0, vel0, charges, send, recv, traj, steps, dt, st,
                       [&](const float* h, const float* x, const float* vel, const float* ea, float* out) {
                           return clof_forward_impl<H>(c, params, Lo, false, h, x, vel, ea, ws, out, st, false);
                       });
}

}  // namespace
}  // extern "C++"

int aether_clof_rollout(const float* const* params, int n_params, int variant, int hidden, int n_layers, int in_node_nf,
                        int flags, float coords_weight, int n_per_graph, int64_t n_nodes, int64_t n_edges, const float* x0,
                        const float* vel0, const float* charges, const int64_t* send, const int64_t* recv,
                        const void* graph, const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                        float* trajectory, int steps, float dt, void* stream) {
    if (int rc = clof_check(params, n_params, variant, hidden, n_layers, in_node_nf, n_per_graph, n_nodes, n_edges, graph,
                            info, "clof_rollout"))
        return rc;
    const ClofLayout Lo(variant, hidden, n_layers, in_node_nf, n_nodes, n_edges, false);
    const RolloutState R(Lo.total, n_nodes, n_edges);
    if (int rc = gnn_rollout_check("clof_rollout", in_node_nf, flags & AETHER_CLOF_KEEP,
                                   !x0 || !vel0 || !charges || !workspace || (steps > 0 && !trajectory) ||
                                       (n_edges > 0 && (!send || !recv)),
                                   flags & ~CLOF_FLAGS, workspace_bytes, R.total))
        return rc;
    if (steps <= 0) return 0;
    const ClofCall c = clof_call(variant, hidden, n_layers, in_node_nf, flags, coords_weight, n_per_graph, n_nodes, n_edges,
                                 graph);
    hipStream_t st = (hipStream_t)stream;
    if (hidden == 64)
        return clof_rollout_impl<64>(c, params, Lo, R, x0, vel0, charges, send, recv, (char*)workspace, trajectory, steps, dt, st);
    return clof_rollout_impl<128>(c, params, Lo, R, x0, vel0, charges, send, recv, (char*)workspace, trajectory, steps, dt, st);
}
