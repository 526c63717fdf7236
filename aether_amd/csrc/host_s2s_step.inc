// Host side of the C ABI: the fused autoregressive step of the seq2seq Aether and its device-side rollout (SURVEY 8f N1).
// Included by aether_hip.hip inside its extern "C" block; not a stand-alone source file.

namespace {

int s2s_fail(int code, const char* what, const char* why) {
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    return fail(code, msg);
}

// locs: the plain localizer of the seq2seq LoCS (s2s_locs.h) -- 3D + O features per edge, rel_feat 2D wide, no origin edge
struct S2SDims {
    int D, O, NF, RF, RFp, EA, EAp, EP;
    explicit S2SDims(int D_, int locs = 0) : D(D_) {
        O = D * (D - 1) / 2; EP = D + O;
        if (locs) { NF = 3 * D + O; RF = 2 * D; } else { NF = 4 * D + O; RF = 3 * D + NF; }
        EA = NF + RF;
        RFp = (RF + 15) / 16 * 16; EAp = (EA + 31) / 32 * 32;      // EAp: whole 32-wide k blocks (split GEMM)
    }
};

// Prepared weights (device): everything the per-module entry points rebuild on every call.
struct S2SPlanLayout {
    size_t fimg, res1p, bn, p1p[4], wr, wi, wn, br, bi, bn_, lb, lbp, total;
    size_t i_mlp4e, i_mlp4_3, i_ih, i_hh, i_prior[4], i_msg2[4], i_pmsg1[4], i_pmsg2[4];       // fp16 x 2 images (0: none)
    size_t i_f0, i_f2, i_mlp3_0, i_mlp3_3, i_ps, i_pr, i_a[4], i_s[4], i_wr, i_wi, i_wn, i_hh2, i_out0, i_out3;   // node-level layers
    size_t i_film1 = 0, i_film2 = 0;     // FiLM field net (mlp_hidden > 0): linear_1 [mh][he], linear_2 [mh][mh]; no i_f0 / i_f2 then
    int ldg;
    // Markov decoder (markov_ku >= 0 used edge types; the recurrent decoder's tensors are then not in the plan): padded lin1 /
    // res1, lin2's bias permuted from c Ku + k to k h + c, and the images of lin1 and of lin2's per-type h x h blocks
    size_t m_l1p = 0, m_r1p = 0, m_b2 = 0, m_i_l1 = 0, m_i_l2[4] = {0, 0, 0, 0};
    static bool splittable(int M, int Kk) { return M % 128 == 0 && Kk % 32 == 0; }
    // filt_R > 0: the filter image has that many features instead of EA (the charge-aware model's folded filter, EA + 4)
    // locs: the widths of the plain localizer (S2SDims), no field net
    S2SPlanLayout(int D, int he, int hd, int K, int R, int prior_layers = 1, int ph = 0, int markov_ku = -1, int mlp_hidden = 0,
                  int filt_R = 0, int locs = 0) {
        const S2SDims d(D, locs);
        const bool rec = markov_ku < 0;
        const int Kr = rec ? K : 0;
        const int64_t hr = rec ? hd : 0;
        ldg = S2S_RFG + 2 * hd;
        size_t off = 0;
        auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
        fimg = take(filt_image_bytes(filt_R > 0 ? filt_R : d.EA, he));
        res1p = take((size_t)he * d.RFp * 4);
        bn = take((size_t)4 * he * 4);
        for (int k = 0; k < 4; ++k) p1p[k] = take(k < Kr ? (size_t)hd * d.EAp * 4 : 0);
        wr = take((size_t)hr * ldg * 4); wi = take((size_t)hr * ldg * 4); wn = take((size_t)hr * ldg * 4);
        br = take((size_t)hr * 4); bi = take((size_t)hr * 4); bn_ = take((size_t)hr * 4);
        lb = take((size_t)4 * R * 4);
        lbp = take((size_t)4 * R * 4);          // the same, gates interleaved by unit (the fused LSTM cell of the split GEMM)
        auto image = [&](int M, int Kk) { return splittable(M, Kk) ? take((size_t)M * Kk * 4) : (size_t)0; };
        i_mlp4e = image(he, he); i_mlp4_3 = image(he, he); i_ih = image(4 * R, he); i_hh = image(4 * R, R);
        for (int l = 0; l < 4; ++l) i_prior[l] = l + 1 < prior_layers ? image(ph, l == 0 ? R : ph) : 0;
        for (int k = 0; k < 4; ++k) {
            i_msg2[k] = k < Kr ? image(hd, hd) : 0; i_pmsg1[k] = k < Kr ? image(hd, d.EAp) : 0; i_pmsg2[k] = k < Kr ? image(hd, hd) : 0;
            i_a[k] = k < Kr ? image(hd, hd) : 0; i_s[k] = k < Kr ? image(hd, hd) : 0;
        }
        if (mlp_hidden > 0) { i_f0 = i_f2 = 0; i_film1 = image(mlp_hidden, he); i_film2 = image(mlp_hidden, mlp_hidden); }
        else if (locs) i_f0 = i_f2 = 0;
        else { i_f0 = image(he, he); i_f2 = image(he, he); }
        i_mlp3_0 = image(he, he); i_mlp3_3 = image(he, he); i_ps = image(he, he);
        i_pr = image(he, he);
        if (rec) { i_wr = image(hd, ldg); i_wi = image(hd, ldg); i_wn = image(hd, S2S_RFG + hd); i_hh2 = image(hd, hd); }
        else i_wr = i_wi = i_wn = i_hh2 = 0;
        i_out0 = image(hd, hd); i_out3 = image(hd, hd);
        if (!rec) {
            m_l1p = take((size_t)hd * d.EAp * 4); m_r1p = take((size_t)hd * d.RFp * 4); m_b2 = take((size_t)markov_ku * hd * 4);
            m_i_l1 = image(hd, d.EAp);
            for (int k = 0; k < markov_ku && k < 4; ++k) m_i_l2[k] = image(hd, hd);
        }
        total = off;
    }
};

struct S2SStepLayout {
    size_t gamma, fh1, fh2, field, ext, rel, relp, Rinv, ea, eap, epos, bimg, fpart, eaf, X0, X1, X3, PsPr, T1e, X4, G, Y1, Y2,
        logits, edges, lists, counts, A, S, Tm, T1p, M1, M2, wide, rp, ip, np_, hh, o1, o2, pred, xa, xb, da, db, ha, hb, ca, cb,
        total;
    int splits;
    // mlp_hidden > 0: the field query is the FiLM net, whose hidden rows (fh1, fh2) are mlp_hidden wide
    // locs: the widths of the plain localizer, and no field query: gamma, fh1, fh2, field and ext are empty
    S2SStepLayout(int D, int he, int hd, int R, int ph, int K, int64_t Nn, int64_t E, int mlp_hidden = 0, int locs = 0) {
        const S2SDims d(D, locs);
        size_t off = 0;
        auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * 4, 256); return o; };
        const size_t nn = (size_t)Nn, ee = (size_t)E, h = (size_t)he, g = (size_t)hd;
        const size_t fw = (size_t)(mlp_hidden > he ? mlp_hidden : he);
        const size_t fq = locs ? 0 : nn;                       // rows of the field query's buffers
        gamma = take(fq * h); fh1 = take(fq * fw); fh2 = take(fq * fw); field = take(fq * D);
        ext = take(fq * 3 * D); rel = take(nn * d.RF); relp = take(nn * d.RFp); Rinv = take(nn * D * D);
        ea = take(ee * d.EA); eap = take(ee * d.EAp); epos = take(ee * d.EP);
        bimg = take((filt_bimg_bytes(E, (int)h) + 3) / 4);
        splits = S2SPriorLayout::filter_splits(he, E);
        fpart = take(splits > 1 ? ee * h * splits : 0);
        eaf = take(ee * h);
        X0 = take(nn * h); X1 = take(nn * h); X3 = take(nn * h); PsPr = take(2 * nn * h);
        T1e = take(ee * h); X4 = take(ee * h); G = take(ee * 4 * (size_t)R);
        Y1 = take(ee * (size_t)(ph > 0 ? ph : 1)); Y2 = take(ee * (size_t)(ph > 0 ? ph : 1));
        logits = take(ee * K); edges = take(ee * K); lists = take(ee * K * 2); counts = take(64);
        A = take((size_t)K * nn * g); S = take((size_t)K * nn * g); Tm = take((size_t)K * ee * g); T1p = take((size_t)K * ee * g);
        M1 = take(ee * g); M2 = take(ee * g);
        wide = take(nn * (S2S_RFG + 2 * g));
        rp = take(nn * g); ip = take(nn * g); np_ = take(nn * g); hh = take(nn * g); o1 = take(nn * g); o2 = take(nn * g);
        pred = take(nn * 2 * D);
        // ping-pong state of aether_s2s_rollout
        xa = take(nn * 2 * D); xb = take(nn * 2 * D); da = take(nn * g); db = take(nn * g);
        ha = take(ee * (size_t)R); hb = take(ee * (size_t)R); ca = take(ee * (size_t)R); cb = take(ee * (size_t)R);
        total = off;
    }
};

// One launch for a table of independent dense layers.  All jobs share the tiling, chosen for the widest job as
// s2s_linear chooses it for a single layer.
// Will s2s_launch_jobs run this table on the split GEMM (k_s2s_gemm_split)?  (The LSTM job decides by it whether its cell
// update rides in the epilogue.)
bool s2s_jobs_take_split(const S2SJobs& T) {
    if (T.n <= 0 || !g_gemm_split) return false;
    int best = 0;
    for (int t = 1; t < T.n; ++t)
        if (T.j[t].N * T.j[t].M > T.j[best].N * T.j[best].M) best = t;
    int64_t tiles_big = 0;
    for (int t = 0; t < T.n; ++t) tiles_big += ((T.j[t].N + 63) / 64) * ((T.j[t].M + 127) / 128);
    if (!(T.j[best].M >= 128 && tiles_big >= LINEAR_SMALL_WGS)) return false;
    for (int t = 0; t < T.n; ++t) {
        const S2SJob& J = T.j[t];
        if (!(J.Wimg != nullptr && J.M % 128 == 0 && J.K % 32 == 0 && (J.W2 == nullptr || (J.W2img != nullptr && J.K2 % 32 == 0)) &&
              (J.g1 == nullptr || J.g2 != nullptr))) return false;
    }
    return true;
}

// One table's launch into the record of aether_s2s_launch_stats (kind: see include/aether_hip.h)
void s2s_stats_jobs(const S2SJobs& T, int kind, int64_t wg128, int wgs) {
    AetherS2SLaunchStats& G = g_s2s_stats;
    AetherS2SLaunchRecord r{};
    int best = 0;
    r.kind = kind; r.jobs = T.n; r.images = 1; r.wgs = wgs; r.wg128 = wg128; r.min_n = T.j[0].N;
    for (int t = 0; t < T.n; ++t) {
        const S2SJob& J = T.j[t];
        if (J.N * J.M > T.j[best].N * T.j[best].M) best = t;
        if (J.N < r.min_n) r.min_n = J.N;
        r.tiles64 += ((J.N + 63) / 64) * ((J.M + 127) / 128);
        if (!(J.Wimg != nullptr && J.M % 128 == 0 && J.K % 32 == 0 && (J.W2 == nullptr || (J.W2img != nullptr && J.K2 % 32 == 0)) &&
              (J.g1 == nullptr || J.g2 != nullptr))) r.images = 0;
        if (J.N > G.max_n[kind]) G.max_n[kind] = J.N;
        if (J.M > G.max_m[kind]) G.max_m[kind] = J.M;
        if (J.K > G.max_k[kind]) G.max_k[kind] = J.K;
        if (J.W2 != nullptr && J.K2 > G.max_k2[kind]) G.max_k2[kind] = J.K2;
    }
    r.N = T.j[best].N; r.M = T.j[best].M; r.K = T.j[best].K; r.K2 = T.j[best].W2 != nullptr ? T.j[best].K2 : 0;
    ++G.launches[kind]; G.jobs[kind] += T.n;
    if (G.logged < AETHER_S2S_LAUNCH_LOG) G.log[G.logged] = r;
    ++G.logged;
}

int s2s_launch_jobs(S2SJobs& T, hipStream_t st) {
    if (T.n <= 0) return AETHER_OK;
    for (int t = 0; t < T.n; ++t) {
        const S2SJob& J = T.j[t];
        if (J.film_gamma != nullptr && (J.film_beta == nullptr || J.film_rows <= 0 || J.act == 5))
            return fail(AETHER_EINVAL, "s2s_step: a FiLM job needs gamma, beta and rows per graph, and is never the LSTM cell job");
    }
    bool big = false, wide = false, ksplit = false;
    {
        int best = 0;
        for (int t = 1; t < T.n; ++t)
            if (T.j[t].N * T.j[t].M > T.j[best].N * T.j[best].M) best = t;
        const S2SJob& B = T.j[best];
        int64_t tiles_big = 0, tiles_small = 0;
        for (int t = 0; t < T.n; ++t) {
            tiles_big += ((T.j[t].N + 63) / 64) * ((T.j[t].M + 127) / 128);
            tiles_small += ((T.j[t].N + 63) / 64) * ((T.j[t].M + 31) / 32);
        }
        big = B.M >= 128 && tiles_big >= LINEAR_SMALL_WGS;
        wide = big && B.N >= 16384;
        ksplit = !big && g_linear_kwaves == 4 && B.K >= 128 && tiles_small < 1024;
    }
    if (big && g_gemm_split) {                               // >= 2 K rows, every weight with an image: the bf16 pipe
        bool all = true;
        for (int t = 0; t < T.n; ++t) {
            const S2SJob& J = T.j[t];
            all = all && J.Wimg != nullptr && J.M % 128 == 0 && J.K % 32 == 0 && (J.W2 == nullptr || (J.W2img != nullptr && J.K2 % 32 == 0)) &&
                  (J.g1 == nullptr || J.g2 != nullptr);
        }
        if (all) {
            // 128-row tiles once they fill the chip twice over, 64-row tiles below (2,560 rows x 512: 160 workgroups)
            int64_t wg128 = 0;
            for (int t = 0; t < T.n; ++t) wg128 += ((T.j[t].N + 127) / 128) * (T.j[t].M / 128);
            const int rows = wg128 >= 512 ? 128 : 64;
            int wgs = 0;
            for (int t = 0; t < T.n; ++t) {
                S2SJob& J = T.j[t];
                const int64_t gx = (J.N + rows - 1) / rows;
                J.wg0 = wgs; J.gx = (int)(gx > 0 ? gx : 1);
                wgs += (int)((gx + 7) / 8 * 8 * (J.M / 128));      // (padded: see the kernel's tile mapping)
            }
            if (wgs == 0) return AETHER_OK;
#define S2S_GS_LAUNCH(KERN, NBV, LDS)                                                                  \
    do {                                                                                               \
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(KERN<NBV>), LDS)) return AETHER_EHIP;     \
        KERN<NBV><<<dim3((unsigned)wgs), dim3(256), LDS, st>>>(T);                                     \
    } while (0)
            // Two structures (s2s_step.h): with at most one workgroup per CU nothing else hides a step's memory round trips,
            // so both operands come through the deep LDS-DMA ring; with more, three workgroups of the registers-for-X
            // structure share a CU and cover for each other (measured: 16.5 vs 22 us at 160 workgroups, 42 vs 57 us at 800).
            // aether_set_option("gemm_split", 2 | 3) forces the second / the first.
            if (g_gemm_split == 2 || (g_gemm_split != 3 && wgs > 256)) {
                const size_t lds = (size_t)GS1_NST * GS_STAGE * 16;
                s2s_stats_jobs(T, rows == 128 ? 4 : 3, wg128, wgs);
                if (rows == 128) S2S_GS_LAUNCH(k_s2s_gemm_split_r1, 2, lds); else S2S_GS_LAUNCH(k_s2s_gemm_split_r1, 1, lds);
            } else {
                s2s_stats_jobs(T, rows == 128 ? 2 : 1, wg128, wgs);
                if (rows == 128) S2S_GS_LAUNCH(k_s2s_gemm_split, 2, gs_lds_bytes(2)); else S2S_GS_LAUNCH(k_s2s_gemm_split, 1, gs_lds_bytes(1));
            }
#undef S2S_GS_LAUNCH
            return AETHER_OK;
        }
    }
    const int nt = wide ? 4 : 2;
    int wg = 0;
    for (int t = 0; t < T.n; ++t) {
        S2SJob& J = T.j[t];
        if (J.K % 16 != 0) return fail(AETHER_EINVAL, "s2s_step: K must be a multiple of 16");
        const int64_t gx = ksplit ? (J.N + 31) / 32 : (J.N + 32 * nt - 1) / (32 * nt);
        const int64_t gy = big ? (J.M + 127) / 128 : ksplit ? (J.M + 15) / 16 : (J.M + 31) / 32;
        J.wg0 = wg; J.gx = (int)(gx > 0 ? gx : 1);
        wg += (int)(gx * gy);
    }
    if (wg == 0) return AETHER_OK;
    s2s_stats_jobs(T, 0, 0, wg);
    bool two = false;
    for (int t = 0; t < T.n; ++t) two = two || T.j[t].W2 != nullptr;
#define S2S_JOBS(MT, NT, KW)                                                                            \
    do {                                                                                                \
        if (two) k_s2s_linear_jobs<MT, NT, 2, KW, true><<<dim3((unsigned)wg), dim3(256), 0, st>>>(T);   \
        else k_s2s_linear_jobs<MT, NT, 2, KW, false><<<dim3((unsigned)wg), dim3(256), 0, st>>>(T);      \
    } while (0)
    if (wide) S2S_JOBS(4, 4, 1);
    else if (big) S2S_JOBS(4, 2, 1);
    else if (ksplit) S2S_JOBS(1, 2, 4);
    else S2S_JOBS(1, 2, 1);
#undef S2S_JOBS
    return AETHER_OK;
}

S2SJob s2s_job(int act, const float* W, int ldw, const float* b, const float* X, int ldx, float* Y, int ldy, int M, int K,
               int64_t N) {
    S2SJob J{};
    J.W = W; J.ldw = ldw; J.bias = b; J.X = X; J.ldx = ldx; J.Y = Y; J.ldy = ldy; J.M = M; J.K = K; J.N = N; J.act = act;
    return J;
}

// The model's sizes and scalar options, as the step / rollout entries receive them
struct S2SSizes {
    int D, he, hd, R, prior_layers, ph, K, skip_first, polar, num_vars;
    float tau;
    int64_t Nn, E;
    int locs = 0;              // the seq2seq LoCS: plain localizer in front of the step, no field (host_s2s_locs.inc)
};

// Everything a step reads besides its state: made once per entry call (s2s_step_args).  Exactly one of dp (recurrent
// decoder) and mp (Markov decoder) is set; the plan's layout P is the one of that decoder.
struct S2SStepArgs : S2SSizes {
    const AetherS2SFieldParams* fp; const AetherS2SPriorParams* pp; const AetherS2SDecoderParams* dp;
    const AetherS2SMarkovParams* mp;
    const char* plan;
    const int64_t *send, *recv, *order, *rowptr;
    bool field_images;         // the plan was built with the field net's parameters (images of its two hidden layers)
    S2SPlanLayout P;
    S2SStepLayout L;
    // The FiLM field query of the dynamic-field model (film != nullptr; fp is null then): mod = gamma_1 | beta_1 | gamma_2 |
    // beta_2, each [batch][mlp_hidden] (aether_s2s_film_modulation); node n belongs to graph n / num_objects
    const AetherS2SFilmParams* film = nullptr;
    int mlp_hidden = 0;
    const float* mod = nullptr;
    int64_t batch = 0;
    int num_objects = 0;
    // The charge-aware model (host_s2s_charges.inc; null: the plain one).  fp / pp / dp then hold the chargeless slices of the
    // widened layers, whose biases the tables below carry: the jobs of those layers take no bias vector.
    const struct S2SChargeArgs* chg = nullptr;
    // ext_logits [E][K] (charge-aware entries): the sample is taken from these logits and the prior (filter .. prior_fc_out) is
    // skipped, h1 / c1 are not written: the decoder on given logits.  features_out [E][he]: the front stops behind mlp4 and
    // leaves its rows there (the per-time-step features of the full-sequence encoder).
    const float* ext_logits = nullptr;
    float* features_out = nullptr;
};

// nidx [Nn] in {0, 1, 2}, eidx [E] in 0 .. 3 (k_s2s_charge_index); bias tables of field_net.0, encoder.res1, the three gates
// (3 rows each) and present_msg_fc1[k] (4 rows); ea: the edge features with the four indicator columns [E][EA + 4]; b2: the
// folded filter bias (its image is the plan's, EA + 4 features)
struct S2SChargeArgs {
    const int32_t *nidx, *eidx;
    const float* nscale;           // [Nn]: 1, or NaN where nidx is 2 (row scale of the output MLP's last hidden layer)
    const float *t_f0, *t_res1, *t_gr, *t_gi, *t_gn, *t_p1[4], *b2;
    float* ea;
};

extern "C++" {                 // (templates: the including block has C linkage)
// f(std::integral_constant<int, D>) for the run-time num_dims (2 or 3): picks a kernel's template argument, e.g.
//   dispatch_dim(D, [&](auto DD) { k<decltype(DD)::value><<<...>>>(...); })      (as dispatch_bools, host_gnn_common.inc)
template <class F>
void dispatch_dim(int D, F&& f) {
    if (D == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

// The half of the step both decoders share -- field query -> local frames -> prior step -> hard Gumbel sample
// (aether.py:86-90, :384-410, :92-98) -- up to the per-type edge lists.  x_in [Nn][2D], h0 / c0 [E][R], uniform [E][K] ->
// h1, c1, and, when `edges` is not null, the sample [E][K] with its lists / counts in the workspace (edges == nullptr: no
// sample, the burn-in of the Markov rollout).  The decoder rides along in two launches: first_jobs(T) adds its jobs to the
// field query's first layer (flushing T itself when it fills up), res1_jobs(T) to the prior's res1 layer, whose launch
// holds only that job otherwise.  P: the plan's layout (recurrent or Markov, S2SPlanLayout).
template <class FirstJobs, class Res1Jobs>
int s2s_front_impl(const S2SStepArgs& a, const S2SStepLayout& L, const S2SPlanLayout& P, char* ws, const float* x_in,
                   const float* ext_field, const float* h0, const float* c0, const float* uniform, float* h1, float* c1,
                   float* edges, FirstJobs&& first_jobs, Res1Jobs&& res1_jobs, hipStream_t st) {
    const int D = a.D, he = a.he, R = a.R, K = a.K, k0 = a.skip_first ? 1 : 0;
    const int64_t Nn = a.Nn, E = a.E;
    const S2SDims d(D, a.locs);
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto pl = [&](size_t off) { return reinterpret_cast<const float*>(a.plan + off); };
    auto im = [&](size_t off) { return off ? reinterpret_cast<const void*>(a.plan + off) : nullptr; };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    const AetherS2SPriorParams* p = a.pp;
    const bool query = !ext_field && !a.locs;                  // the built-in field query runs (LoCS has no field)
    S2SJobs T;
    const int ldg = P.ldg;
    // ---- field query (aether.py:86-90); its first layer shares a launch with first_jobs
    T.n = 0;
    const int mh = a.mlp_hidden;
    const size_t mplane = (size_t)a.batch * mh;
    if (query && a.film) {
        // the FiLM net (dynamic_field_aether.py:117-134, nn/nn/filmed_network.py:27-35): linear_1 - FiLM - SiLU here, linear_2 -
        // FiLM - SiLU below, linear_3 in k_s2s_node_prep
        const int half = he / 2;
        const unsigned rb = (unsigned)((Nn * half + 255) / 256);
        dispatch_dim(D, [&](auto DD) {
            k_s2s_rff<decltype(DD)::value><<<dim3(rb), dim3(256), 0, st>>>(x_in, 2 * D, a.film->B, half, wp(L.gamma), Nn);
        });
        S2SJob J = s2s_job(1, a.film->lin1_w, he, a.film->lin1_b, wp(L.gamma), he, wp(L.fh1), mh, mh, he, Nn);
        J.film_gamma = a.mod; J.film_beta = a.mod + mplane; J.film_rows = a.num_objects; J.Wimg = im(P.i_film1);
        T.j[T.n++] = J;
    } else if (query) {
        const int half = he / 2;
        const unsigned rb = (unsigned)((Nn * half + 255) / 256);
        dispatch_dim(D, [&](auto DD) {
            k_s2s_rff<decltype(DD)::value><<<dim3(rb), dim3(256), 0, st>>>(x_in, 2 * D, a.fp->B, half, wp(L.gamma), Nn);
        });
        T.j[T.n++] = s2s_job(1, a.fp->w0, he, a.chg ? nullptr : a.fp->b0, wp(L.gamma), he, wp(L.fh1), he, he, he, Nn);
        T.j[T.n - 1].Wimg = a.field_images ? im(P.i_f0) : nullptr;
        if (a.chg) { T.j[T.n - 1].btab = a.chg->t_f0; T.j[T.n - 1].bidx = a.chg->nidx; T.j[T.n - 1].bstride = he; }
    }
    if (int rc = first_jobs(T)) return rc;
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    if (query && a.film) {
        S2SJob J = s2s_job(1, a.film->lin2_w, mh, a.film->lin2_b, wp(L.fh1), mh, wp(L.fh2), mh, mh, mh, Nn);
        J.film_gamma = a.mod + 2 * mplane; J.film_beta = a.mod + 3 * mplane; J.film_rows = a.num_objects; J.Wimg = im(P.i_film2);
        T.n = 0; T.j[T.n++] = J;
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    } else if (query) {
        T.n = 0; T.j[T.n++] = s2s_job(1, a.fp->w2, he, a.fp->b2, wp(L.fh1), he, wp(L.fh2), he, he, he, Nn);
        T.j[T.n - 1].Wimg = a.field_images ? im(P.i_f2) : nullptr;
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    }
    // ---- last field layer + local frames of [inputs | field], once for the prior and the decoder (:385-388, :620-622)
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int64_t* lists = reinterpret_cast<int64_t*>(ws + L.lists);
    if (a.locs) {                      // the plain localizer on the inputs themselves (locs.py:343, :572)
        dispatch_dim(D, [&](auto DD) {
            constexpr int Dc = decltype(DD)::value;
            k_s2s_locs_node_prep<Dc><<<blocks(Nn), dim3(256), 0, st>>>(x_in, wp(L.rel), wp(L.Rinv), wp(L.relp), d.RFp, wp(L.wide), ldg,
                                                                      counts, Nn);
            k_s2s_locs_edge_prep<Dc><<<blocks(E), dim3(256), 0, st>>>(x_in, a.send, a.recv, wp(L.rel), a.polar, wp(L.ea), wp(L.eap),
                                                                      wp(L.epos), E);
        });
    } else {
        const float* fh2 = ext_field ? nullptr : wp(L.fh2);
        const float* w4 = ext_field ? nullptr : a.film ? a.film->lin3_w : a.fp->w4;
        const float* b4 = ext_field ? nullptr : a.film ? a.film->lin3_b : a.fp->b4;
        const int fk = a.film ? mh : he;                        // width of the last hidden layer of the field query
        float* fout = ext_field ? nullptr : wp(L.field);
        const dim3 nb4((unsigned)((Nn + 3) / 4));
        dispatch_dim(D, [&](auto DD) {
            constexpr int Dc = decltype(DD)::value;
            k_s2s_node_prep<Dc><<<nb4, dim3(256), 0, st>>>(x_in, ext_field, fh2, w4, b4, fk, fout, wp(L.ext), wp(L.rel), wp(L.Rinv),
                                                           wp(L.relp), d.RFp, wp(L.wide), ldg, counts, Nn);
            if (a.chg)
                k_s2s_edge_prep_charges<Dc><<<blocks(E), dim3(256), 0, st>>>(wp(L.ext), a.send, a.recv, wp(L.rel), a.polar, a.chg->ea,
                                                                             wp(L.eap), wp(L.epos), E, a.chg->eidx);
            else
                k_s2s_edge_prep<Dc><<<blocks(E), dim3(256), 0, st>>>(wp(L.ext), a.send, a.recv, wp(L.rel), a.polar, wp(L.ea), wp(L.eap),
                                                                     wp(L.epos), E);
        });
    }
    if (a.ext_logits == nullptr) {     // (the prior: not for the decoder on given logits)
    // ---- anisotropic edge filter (:391)
    {
        const f16x8* image = reinterpret_cast<const f16x8*>(a.plan + P.fimg);
        f16x8* bimg = reinterpret_cast<f16x8*>(ws + L.bimg);
        dispatch_dim(D, [&](auto DD) {
            constexpr int EP = decltype(DD)::value * (decltype(DD)::value + 1) / 2;       // S2SDims::EP: 3 or 6
            k_s2s_filter_bimg<EP><<<filter_bimg_grid(E), dim3(256), 0, st>>>(wp(L.epos), p->filt_w0, p->filt_b0, 0, he, E, bimg);
        });
        const int64_t units = ((E + 255) / 256) * (he / 64) * L.splits;
        const dim3 grid((unsigned)(units < FILTER_WGS ? units : FILTER_WGS));
        float* dst = L.splits > 1 ? wp(L.fpart) : wp(L.eaf);
        s2s_stats_filter(L.splits);
#define FILT_LAUNCH(RR)                                                                                                  \
    do {                                                                                                                 \
        const size_t lds = filt_lds_bytes(RR);                                                                           \
        if (ensure_dynamic_lds(reinterpret_cast<const void*>(k_s2s_filter_split<RR>), lds)) return AETHER_EHIP;          \
        k_s2s_filter_split<RR><<<grid, dim3(512), lds, st>>>(image, filt_b2, filt_ea, bimg, dst, he, E, L.splits, 1, (int)grid.x);   \
    } while (0)
        const float* filt_b2 = a.chg ? a.chg->b2 : p->filt_b2;
        const float* filt_ea = a.chg ? a.chg->ea : wp(L.ea);
        if (a.chg) { if (D == 2) FILT_LAUNCH(28); else FILT_LAUNCH(43); }       // + the four one-hot charge features
        else if (a.locs) { if (D == 2) FILT_LAUNCH(11); else FILT_LAUNCH(18); } // the plain localizer's 5D + O
        else if (D == 2) FILT_LAUNCH(24); else FILT_LAUNCH(39);
#undef FILT_LAUNCH
        // x = edge2node(edge_attr) (:393-394): planes added and in-edges summed in one pass
        k_s2s_planes_segsum<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(dst, L.splits, (int64_t)E * he, a.order, a.rowptr,
                                                                      wp(L.eaf), wp(L.X0), he, (float)(a.num_vars - 1));
    }
    const float *bn3s = pl(P.bn), *bn3b = pl(P.bn) + he, *bn4s = pl(P.bn) + 2 * he, *bn4b = pl(P.bn) + 3 * he;
    // + res1(rel_feat) (:395), mlp3 (RefNRIMLP, eval)
    { S2SJob J = s2s_job(0, pl(P.res1p), d.RFp, a.chg ? nullptr : p->res1_b, wp(L.relp), d.RFp, wp(L.X0), he, he, d.RFp, Nn);
      J.accumulate = 1;
      if (a.chg) { J.btab = a.chg->t_res1; J.bidx = a.chg->nidx; J.bstride = he; }
      T.n = 0; T.j[T.n++] = J;
      if (int rc = res1_jobs(T)) return rc;
      if (int rc = s2s_launch_jobs(T, st)) return rc; }
    if (int rc = nri_one(st, s2s_job(4, p->mlp3_w0, he, p->mlp3_b0, wp(L.X0), he, wp(L.X1), he, he, he, Nn), im(P.i_mlp3_0))) return rc;
    if (int rc = nri_one(st, s2s_job(4, p->mlp3_w3, he, p->mlp3_b3, wp(L.X1), he, wp(L.X3), he, he, he, Nn), im(P.i_mlp3_3), bn3s,
                         bn3b)) return rc;
    // mlp4 on [x_send | x_recv | edge] (:396-398), one LSTM step per edge (:400-407), prior_fc_out (:408): host_nri_chain.inc
    float* Ps = wp(L.PsPr);
    float* x4 = a.features_out ? a.features_out : wp(L.X4);
    if (int rc = nri_edge_mlp4(NriMlp4{p->mlp4_w0, p->mlp4_b0, p->mlp4_w3, p->mlp4_b3, bn4s, bn4b, im(P.i_ps), im(P.i_pr),
                                       im(P.i_mlp4e), im(P.i_mlp4_3), wp(L.X3), wp(L.eaf), a.send, a.recv, Ps, Ps + (size_t)Nn * he,
                                       wp(L.T1e), x4, he, Nn, E}, st)) return rc;
    if (a.features_out) return AETHER_OK;
    if (int rc = nri_lstm_head(NriLstmHead{p->lstm_w_ih, p->lstm_w_hh, pl(P.lb), pl(P.lbp), im(P.i_ih), im(P.i_hh), p->prior_w,
                                           p->prior_b, {im(P.i_prior[0]), im(P.i_prior[1]), im(P.i_prior[2]), im(P.i_prior[3])},
                                           x4, h0, c0, wp(L.G), h1, c1, wp(L.Y1), wp(L.Y2), wp(L.logits), he, R, a.prior_layers,
                                           a.ph, K, E}, st)) return rc;
    } else {                           // (given logits: what rides in the prior's res1 launch goes alone)
        T.n = 0;
        if (int rc = res1_jobs(T)) return rc;
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    }
    // ---- hard Gumbel sample (:92-98) and the per-type edge lists of the decoder
    if (edges != nullptr)
        k_s2s_gumbel_select<<<blocks(E), dim3(256), 0, st>>>(a.ext_logits ? a.ext_logits : wp(L.logits), uniform, a.tau, K, k0, edges, lists, counts, E);
    return AETHER_OK;
}

// The end of both decoders: the output MLP on `in` [Nn][hd], its last layer with globalise and residual (aether.py:649-654;
// q: either decoder's parameters, both name the layers out0 / out3 / out6)
template <class DecoderParams>
int s2s_out_tail(const S2SStepArgs& a, char* ws, const DecoderParams* q, const float* in, const float* x_in, float* x_out,
                 hipStream_t st) {
    const int hd = a.hd;
    const int64_t Nn = a.Nn;
    const NriMem m{ws, a.plan};
    if (int rc = nri_one(st, s2s_job(2, q->out0_w, hd, q->out0_b, in, hd, m.wp(a.L.o1), hd, hd, hd, Nn), m.im(a.P.i_out0))) return rc;
    { S2SJob J = s2s_job(2, q->out3_w, hd, q->out3_b, m.wp(a.L.o1), hd, m.wp(a.L.o2), hd, hd, hd, Nn);
      if (a.chg) { J.scale = a.chg->nscale; J.sstride = 1; }       // 1, or NaN for a node whose charge index was out of range
      if (int rc = nri_one(st, J, m.im(a.P.i_out3))) return rc; }
    dispatch_dim(a.D, [&](auto DD) {
        k_s2s_out_globalize<decltype(DD)::value><<<dim3((unsigned)((Nn + 3) / 4)), dim3(256), 0, st>>>(
            m.wp(a.L.o2), q->out6_w, q->out6_b, hd, x_in, m.wp(a.L.Rinv), x_out, Nn);
    });
    return AETHER_OK;
}
}  // extern "C++"

// The recurrent decoder's step.  x_in [Nn][2D], dh_in [Nn][hd], h0 / c0 [E][R], uniform [E][K] -> x_out, dh_out, h1, c1
// (+ edges_out [E][K] when not null)
int s2s_step_impl(const S2SStepArgs& a, char* ws, const float* x_in, const float* ext_field, const float* dh_in,
                  const float* h0, const float* c0, const float* uniform, float* x_out, float* dh_out, float* h1, float* c1,
                  float* edges_out, hipStream_t st) {
    const int D = a.D, hd = a.hd, K = a.K, k0 = a.skip_first ? 1 : 0;
    const int64_t Nn = a.Nn, E = a.E;
    const S2SDims d(D, a.locs);
    const S2SPlanLayout& P = a.P;
    const S2SStepLayout& L = a.L;
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto pl = [&](size_t off) { return reinterpret_cast<const float*>(a.plan + off); };
    auto im = [&](size_t off) { return off ? reinterpret_cast<const void*>(a.plan + off) : nullptr; };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    const AetherS2SDecoderParams* q = a.dp;
    S2SJobs T;
    const int ldg = P.ldg;
    float* A = wp(L.A);
    float* S = wp(L.S);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int64_t* lists = reinterpret_cast<int64_t*>(ws + L.lists);
    float* edges = edges_out ? edges_out : wp(L.edges);
    // ---- field query, prior step, sample; the field query's first layer shares a launch with the decoder's four
    // first-layer products of the hidden state (aether.py:596-601, receiver | sender halves of msg_fc1)
    auto first_jobs = [&](S2SJobs& F) {
        if (E > 0)
            for (int k = k0; k < K; ++k) {
                F.j[F.n++] = s2s_job(0, q->msg_fc1_w[k], 2 * hd, q->msg_fc1_b[k], dh_in, hd, A + (size_t)k * Nn * hd, hd, hd, hd, Nn);
                F.j[F.n - 1].Wimg = im(P.i_a[k]);
                F.j[F.n++] = s2s_job(0, q->msg_fc1_w[k] + hd, 2 * hd, nullptr, dh_in, hd, S + (size_t)k * Nn * hd, hd, hd, hd, Nn);
                F.j[F.n - 1].Wimg = im(P.i_s[k]);
                if (F.n > S2S_MAX_JOBS - 2) { if (int rc = s2s_launch_jobs(F, st)) return rc; F.n = 0; }
            }
        return (int)AETHER_OK;
    };
    auto no_jobs = [](S2SJobs&) { return (int)AETHER_OK; };
    if (int rc = s2s_front_impl(a, L, P, ws, x_in, ext_field, h0, c0, uniform, h1, c1, edges, first_jobs, no_jobs, st)) return rc;
    // ---- decoder (:590-654): messages from the hidden states
    // (hard samples: an edge sits in at most one type's list, so the second-layer jobs below WRITE their rows of M1 / M2;
    // the rows of edges sampled as a skipped type are cleared here)
    k_s2s_pair_tanh_all<<<blocks(E * (hd / 4)), dim3(256), 0, st>>>(A, S, Nn, a.send, a.recv, edges, K, k0, wp(L.Tm), wp(L.M1),
                                                                   wp(L.M2), hd, E, 0);
    // second layer of the hidden-state messages and first layer of the present-state messages (:624-635) of every edge type
    // in one launch (independent of each other), then the second present-state layer
    auto msg2 = [&](int k) {
        S2SJob J = s2s_job(3, q->msg_fc2_w[k], hd, q->msg_fc2_b[k], wp(L.Tm) + (size_t)k * E * hd, hd, wp(L.M1), hd, hd, hd, E);
        J.xidx = lists + (size_t)k * E; J.yidx = lists + (size_t)k * E; J.n_dev = counts + k;
        J.scale = edges + k; J.sstride = K; J.Wimg = im(P.i_msg2[k]);
        return J;
    };
    auto pmsg1 = [&](int k) {
        S2SJob J = s2s_job(2, pl(P.p1p[k]), d.EAp, a.chg ? nullptr : q->pmsg_fc1_b[k], wp(L.eap), d.EAp,
                           wp(L.T1p) + (size_t)k * E * hd, hd, hd, d.EAp, E);
        J.xidx = lists + (size_t)k * E; J.n_dev = counts + k; J.Wimg = im(P.i_pmsg1[k]);
        if (a.chg) { J.btab = a.chg->t_p1[k]; J.bidx = a.chg->eidx; J.bstride = hd; }     // (row of the table: by edge id, after xidx)
        return J;
    };
    auto pmsg2 = [&](int k) {
        S2SJob J = s2s_job(2, q->pmsg_fc2_w[k], hd, q->pmsg_fc2_b[k], wp(L.T1p) + (size_t)k * E * hd, hd, wp(L.M2), hd, hd, hd, E);
        J.yidx = lists + (size_t)k * E; J.n_dev = counts + k; J.scale = edges + k; J.sstride = K;
        J.Wimg = im(P.i_pmsg2[k]);
        return J;
    };
    T.n = 0;
    for (int k = k0; k < K; ++k) { T.j[T.n++] = msg2(k); T.j[T.n++] = pmsg1(k); }      // K <= 4: at most eight jobs
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    T.n = 0;
    for (int k = k0; k < K; ++k) T.j[T.n++] = pmsg2(k);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    // both in-edge means into the wide gate row [rel | agg_p | agg_h]
    float* wide = wp(L.wide);
    k_s2s_segment_mean2<<<dim3((unsigned)Nn, 2), dim3(128), 0, st>>>(wp(L.M2), wp(L.M1), a.order, a.rowptr, wide + S2S_RFG,
                                                                     wide + S2S_RFG + hd, ldg, hd);
    // GRU-style gate (:638-646): four K-concatenated products in one launch
    T.n = 0;
    T.j[T.n++] = s2s_job(0, pl(P.wr), ldg, a.chg ? nullptr : pl(P.br), wide, ldg, wp(L.rp), hd, hd, S2S_RFG + 2 * hd, Nn);
    T.j[T.n - 1].Wimg = im(P.i_wr);
    T.j[T.n++] = s2s_job(0, pl(P.wi), ldg, a.chg ? nullptr : pl(P.bi), wide, ldg, wp(L.ip), hd, hd, S2S_RFG + 2 * hd, Nn);
    T.j[T.n - 1].Wimg = im(P.i_wi);
    T.j[T.n++] = s2s_job(0, pl(P.wn), ldg, a.chg ? nullptr : pl(P.bn_), wide, ldg, wp(L.np_), hd, hd, S2S_RFG + hd, Nn);
    T.j[T.n - 1].Wimg = im(P.i_wn);
    if (a.chg) {                                               // rows of the summed gate biases + the charge term
        const float* gate_tables[3] = {a.chg->t_gr, a.chg->t_gi, a.chg->t_gn};
        for (int g = 0; g < 3; ++g) { T.j[g].btab = gate_tables[g]; T.j[g].bidx = a.chg->nidx; T.j[g].bstride = hd; }
    }
    T.j[T.n++] = s2s_job(0, q->hidden_h_w, hd, nullptr, wide + S2S_RFG + hd, ldg, wp(L.hh), hd, hd, hd, Nn);
    T.j[T.n - 1].Wimg = im(P.i_hh2);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    if (a.chg)
        k_s2s_gate_charges<<<blocks(Nn * hd), dim3(256), 0, st>>>(wp(L.rp), wp(L.ip), wp(L.np_), wp(L.hh), dh_in, dh_out, Nn * hd,
                                                                 a.chg->nidx, hd);
    else
        k_s2s_gate<<<blocks(Nn * hd), dim3(256), 0, st>>>(wp(L.rp), wp(L.ip), wp(L.np_), wp(L.hh), dh_in, dh_out, Nn * hd);
    return s2s_out_tail(a, ws, q, dh_out, x_in, x_out, st);
}

int s2s_markov_step_impl(const S2SStepArgs& a, char* ws, const float* x_in, const float* ext_field, const float* h0,
                         const float* c0, const float* uniform, float* x_out, float* h1, float* c1, float* edges_out,
                         bool decode, hipStream_t st);                     // host_s2s_markov.inc
int s2s_markov_check(const AetherS2SMarkovParams* mp, int D, int h, int K, int skip_first);

// One step of whichever decoder the arguments name.  decode = false (Markov decoder only): the prior alone -- no sample, no
// decoder, next.x not written.
int s2s_step(const S2SStepArgs& a, char* ws, const S2SStateIn& cur, const float* ext_field, const float* uniform,
             const S2SStateOut& next, float* edges_out, bool decode, hipStream_t st) {
    if (a.mp) return s2s_markov_step_impl(a, ws, cur.x, ext_field, cur.h, cur.c, uniform, next.x, next.h, next.c, edges_out, decode, st);
    return s2s_step_impl(a, ws, cur.x, ext_field, cur.dh, cur.h, cur.c, uniform, next.x, next.dh, next.h, next.c, edges_out, st);
}

// The checks of the four step / rollout entries (`what`: the entry's name in the messages) but the workspace's size, which
// s2s_run_step / s2s_run_rollout compare with the layout of the arguments made afterwards.  markov: the entry's decoder is mp, not dp
// (the other one is null); need_field: no field is handed in, so fp is needed; pointers: the entry's own buffers are all
// there; burn_in_steps, steps: of a rollout (a single step: 0, 1).
int s2s_entry_check(const char* what, bool markov, const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp,
                    const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, const void* plan, const S2SSizes& z,
                    bool need_field, bool pointers, int burn_in_steps, int steps) {
    if (markov)
        if (int rc = s2s_markov_check(mp, z.D, z.hd, z.K, z.skip_first)) return rc;
    if (!pp || !(markov ? mp != nullptr : dp != nullptr) || !plan || (need_field && !fp))
        return fail(AETHER_EINVAL, "s2s_step: null pointer");
    if (z.D != 2 && z.D != 3) return fail(AETHER_EINVAL, "s2s_step: num_dims must be 2 or 3");
    if (z.he < 128 || z.he % 128 != 0) return fail(AETHER_EINVAL, "s2s_step: encoder hidden must be a multiple of 128");
    if (z.hd < 32 || z.hd % 32 != 0) return fail(AETHER_EINVAL, "s2s_step: decoder hidden must be a multiple of 32");
    if (z.R < 16 || z.R % 16 != 0) return fail(AETHER_EINVAL, "s2s_step: rnn_hidden must be a multiple of 16");
    if (z.prior_layers < 1 || z.prior_layers > 4 || (z.prior_layers > 1 && (z.ph < 16 || z.ph % 16 != 0)))
        return fail(AETHER_EINVAL, "s2s_step: 1..4 prior layers, prior_hidden a multiple of 16");
    if (z.K < 1 || z.K > 4 || z.num_vars < 2 || z.Nn <= 0 || z.E <= 0) return fail(AETHER_EINVAL, "s2s_step: bad sizes");
    if (!pointers) return s2s_fail(AETHER_EINVAL, what, "null pointer");
    if (burn_in_steps < 0 || steps < 0 || burn_in_steps + steps == 0) return s2s_fail(AETHER_EINVAL, what, "no steps");
    if (!(z.tau > 0.0f)) return s2s_fail(AETHER_EINVAL, what, "tau must be positive");
    return AETHER_OK;
}

// (after s2s_entry_check: the layouts take the sizes as valid)
extern "C++" S2SStepArgs s2s_step_args(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp,
                                       const AetherS2SDecoderParams* dp, const AetherS2SMarkovParams* mp, const void* plan,
                                       const S2SSizes& z, const int64_t* send, const int64_t* recv, const int64_t* order,
                                       const int64_t* rowptr) {
    return S2SStepArgs{z, fp, pp, dp, mp, (const char*)plan, send, recv, order, rowptr, fp != nullptr,
                       S2SPlanLayout(z.D, z.he, z.hd, z.K, z.R, z.prior_layers, z.ph, dp ? -1 : z.K - (z.skip_first ? 1 : 0)),
                       S2SStepLayout(z.D, z.he, z.hd, z.R, z.ph, z.K, z.Nn, z.E)};
}

// (`what`, workspace_bytes: the last of the entry's checks, on the one layout its call builds)
int s2s_run_step(const char* what, const S2SStepArgs& a, void* workspace, size_t workspace_bytes, const S2SStateIn& cur,
                 const float* ext_field, const float* uniform, const S2SStateOut& next, float* edges_out, void* stream) {
    if (workspace_bytes < a.L.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    if (int rc = s2s_step(a, (char*)workspace, cur, ext_field, uniform, next, edges_out, true, (hipStream_t)stream)) return rc;
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

// burn_in [T0][Nn][2D] teacher-forced, then `steps` steps from inputs; decoder_state (null: the Markov decoder), h, c are
// read first and written last.  burn_in_field [T0][Nn][D] (or null): the field of the burn-in frames, known before the loop
// starts (one batched query instead of one per step); the prediction steps always query theirs.
int s2s_run_rollout(const char* what, const S2SStepArgs& a, void* workspace, size_t workspace_bytes, int burn_in_steps,
                    const float* burn_in, int steps, const float* inputs, float* decoder_state, float* h, float* c,
                    const float* uniform, float* predictions, float* edges_out, void* stream,
                    const float* burn_in_field = nullptr) {
    if (workspace_bytes < a.L.total) return s2s_fail(AETHER_ESPACE, what, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const S2SStepLayout& L = a.L;
    auto step = [&](int t, bool teacher, const S2SStateIn& cur, const float* u, const S2SStateOut& next, float* eout, bool decode) {
        const float* ext = teacher && burn_in_field ? burn_in_field + (size_t)t * a.Nn * a.D : nullptr;
        return s2s_step(a, ws, cur, ext, u, next, eout, decode, st);
    };
    return nri_rollout(ws, NriRolloutWs{L.xa, L.da, L.db, L.ha, L.hb, L.ca, L.cb, a.D, a.hd, a.R, a.K, a.Nn, a.E}, burn_in_steps,
                       burn_in, steps, inputs, decoder_state, h, c, uniform, predictions, edges_out, step, st);
}

// Bytes of the plan of either decoder, 0 for sizes the fused step does not take.  markov_ku: the Markov decoder's count of
// used edge types (at least one), -1 for the recurrent decoder.
size_t s2s_plan_size(int D, int he, int hd, int R, int prior_layers, int ph, int K, int markov_ku) {
    if ((D != 2 && D != 3) || he < 128 || he % 128 != 0 || hd < 32 || hd % 32 != 0 || R < 16 || R % 16 != 0 || K < 1 || K > 4 ||
        prior_layers < 1 || prior_layers > 4 || markov_ku == 0 || markov_ku < -1)
        return 0;
    return S2SPlanLayout(D, he, hd, K, R, prior_layers, ph, markov_ku).total;
}

// need: s2s_plan_size of the model
int s2s_plan_buffer_check(const char* what, size_t need, const void* plan, size_t plan_bytes) {
    if (need == 0) return s2s_fail(AETHER_EINVAL, what, "bad sizes");
    if (plan_bytes < need || ((size_t)plan & 255)) return s2s_fail(AETHER_ESPACE, what, "plan buffer too small or not 256-byte aligned");
    return AETHER_OK;
}

// The fp16 x 2 image of W [M][Kk] (row stride ldw) at its place in the plan (off == 0: the layout has none)
void s2s_image(char* base, hipStream_t st, size_t off, const float* W, int M, int Kk, int ldw, int gate_units = 0) {
    if (off) k_s2s_gemm_image<<<dim3((unsigned)(((int64_t)M * (Kk / 8) + 255) / 256)), dim3(256), 0, st>>>(
                 W, M, Kk, ldw, reinterpret_cast<f16x8*>(base + off), gate_units);
}

// The images of the output MLP's two hidden layers, which both decoders have
void s2s_out_images(char* base, hipStream_t st, const S2SPlanLayout& P, const float* out0_w, const float* out3_w, int hd) {
    s2s_image(base, st, P.i_out0, out0_w, hd, hd, hd);
    s2s_image(base, st, P.i_out3, out3_w, hd, hd, hd);
}

// The prepared weights of the shared half of the step (field query, prior) into a plan of either layout.
void s2s_plan_build_front(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, int D, int he, int rnn_hidden,
                          int prior_layers, int prior_hidden, const S2SPlanLayout& P, char* base, hipStream_t st, int filt_R = 0,
                          int locs = 0) {
    const S2SDims d(D, locs);
    auto fl = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    filter_images_launch(pp->filt_w2, filt_R > 0 ? filt_R : d.EA, he, base + P.fimg, st);
    k_s2s_pad_rows<<<blocks((int64_t)he * d.RFp), dim3(256), 0, st>>>(pp->res1_w, d.RF, d.RF, fl(P.res1p), d.RFp, he);
    k_s2s_bn_affine<<<blocks(he), dim3(256), 0, st>>>(pp->mlp3_bn_w, pp->mlp3_bn_b, pp->mlp3_bn_mean, pp->mlp3_bn_var, fl(P.bn),
                                                     fl(P.bn) + he, he);
    k_s2s_bn_affine<<<blocks(he), dim3(256), 0, st>>>(pp->mlp4_bn_w, pp->mlp4_bn_b, pp->mlp4_bn_mean, pp->mlp4_bn_var,
                                                     fl(P.bn) + 2 * he, fl(P.bn) + 3 * he, he);
    k_s2s_add_vec<<<blocks(4 * rnn_hidden), dim3(256), 0, st>>>(pp->lstm_b_ih, pp->lstm_b_hh, fl(P.lb), 4 * rnn_hidden);
    k_s2s_lstm_bias_interleave<<<blocks(4 * rnn_hidden), dim3(256), 0, st>>>(pp->lstm_b_ih, pp->lstm_b_hh, fl(P.lbp), rnn_hidden);
    s2s_image(base, st, P.i_mlp4e, pp->mlp4_w0 + 2 * he, he, he, 3 * he);
    s2s_image(base, st, P.i_mlp4_3, pp->mlp4_w3, he, he, he);
    s2s_image(base, st, P.i_ih, pp->lstm_w_ih, 4 * rnn_hidden, he, he, rnn_hidden);             // gates interleaved by unit (S2SJob act 5)
    s2s_image(base, st, P.i_hh, pp->lstm_w_hh, 4 * rnn_hidden, rnn_hidden, rnn_hidden, rnn_hidden);
    for (int l = 0; l + 1 < prior_layers; ++l)
        s2s_image(base, st, P.i_prior[l], pp->prior_w[l], prior_hidden, l == 0 ? rnn_hidden : prior_hidden,
                  l == 0 ? rnn_hidden : prior_hidden);
    if (fp) { s2s_image(base, st, P.i_f0, fp->w0, he, he, he); s2s_image(base, st, P.i_f2, fp->w2, he, he, he); }
    s2s_image(base, st, P.i_mlp3_0, pp->mlp3_w0, he, he, he);
    s2s_image(base, st, P.i_mlp3_3, pp->mlp3_w3, he, he, he);
    s2s_image(base, st, P.i_ps, pp->mlp4_w0, he, he, 3 * he);
    s2s_image(base, st, P.i_pr, pp->mlp4_w0 + he, he, he, 3 * he);
}

// The recurrent decoder's prepared weights into a plan of its layout.
void s2s_plan_build_recurrent(const AetherS2SDecoderParams* dp, int D, int hd, int K, const S2SPlanLayout& P, char* base,
                              hipStream_t st, int locs = 0) {
    const S2SDims d(D, locs);
    auto fl = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    for (int k = 0; k < K; ++k)
        k_s2s_pad_rows<<<blocks((int64_t)hd * d.EAp), dim3(256), 0, st>>>(dp->pmsg_fc1_w[k], d.EA, d.EA, fl(P.p1p[k]), d.EAp, hd);
    const int64_t gitems = (int64_t)hd * P.ldg;
    k_s2s_concat_rows<<<blocks(gitems), dim3(256), 0, st>>>(dp->input_r_w, d.RF, S2S_RFG, dp->present_r_w, hd, dp->hidden_r_w, hd,
                                                           fl(P.wr), P.ldg, hd);
    k_s2s_concat_rows<<<blocks(gitems), dim3(256), 0, st>>>(dp->input_i_w, d.RF, S2S_RFG, dp->present_i_w, hd, dp->hidden_i_w, hd,
                                                           fl(P.wi), P.ldg, hd);
    k_s2s_concat_rows<<<blocks(gitems), dim3(256), 0, st>>>(dp->input_n_w, d.RF, S2S_RFG, dp->present_n_w, hd, nullptr, hd, fl(P.wn),
                                                           P.ldg, hd);
    k_s2s_add_vec<<<blocks(hd), dim3(256), 0, st>>>(dp->input_r_b, dp->present_r_b, fl(P.br), hd);
    k_s2s_add_vec<<<blocks(hd), dim3(256), 0, st>>>(dp->input_i_b, dp->present_i_b, fl(P.bi), hd);
    k_s2s_add_vec<<<blocks(hd), dim3(256), 0, st>>>(dp->input_n_b, dp->present_n_b, fl(P.bn_), hd);
    s2s_image(base, st, P.i_wr, fl(P.wr), hd, P.ldg, P.ldg);
    s2s_image(base, st, P.i_wi, fl(P.wi), hd, P.ldg, P.ldg);
    s2s_image(base, st, P.i_wn, fl(P.wn), hd, S2S_RFG + hd, P.ldg);
    s2s_image(base, st, P.i_hh2, dp->hidden_h_w, hd, hd, hd);
    s2s_out_images(base, st, P, dp->out0_w, dp->out3_w, hd);
    for (int k = 0; k < K; ++k) {
        s2s_image(base, st, P.i_a[k], dp->msg_fc1_w[k], hd, hd, 2 * hd);
        s2s_image(base, st, P.i_s[k], dp->msg_fc1_w[k] + hd, hd, hd, 2 * hd);
        s2s_image(base, st, P.i_msg2[k], dp->msg_fc2_w[k], hd, hd, hd);
        s2s_image(base, st, P.i_pmsg1[k], fl(P.p1p[k]), hd, d.EAp, d.EAp);            // the zero-padded copy built above
        s2s_image(base, st, P.i_pmsg2[k], dp->pmsg_fc2_w[k], hd, hd, hd);
    }
}
}  // namespace

size_t aether_s2s_plan_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                             int prior_hidden, int num_edge_types) {
    return s2s_plan_size(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, -1);
}

int aether_s2s_plan_build(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp, int num_dims,
                          int encoder_hidden,
                          int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, void* plan,
                          size_t plan_bytes, void* stream) {
    if (!pp || !dp || !plan) return fail(AETHER_EINVAL, "s2s_plan_build: null pointer");
    const int D = num_dims, he = encoder_hidden, hd = decoder_hidden, K = num_edge_types;
    if (int rc = s2s_plan_buffer_check("s2s_plan_build", s2s_plan_size(D, he, hd, rnn_hidden, prior_layers, prior_hidden, K, -1),
                                       plan, plan_bytes)) return rc;
    const S2SPlanLayout P(D, he, hd, K, rnn_hidden, prior_layers, prior_hidden);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)plan;
    s2s_plan_build_front(fp, pp, D, he, rnn_hidden, prior_layers, prior_hidden, P, base, st);
    s2s_plan_build_recurrent(dp, D, hd, K, P, base, st);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}

size_t aether_s2s_step_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                       int num_edge_types, int64_t n_nodes, int64_t n_edges) {
    if ((num_dims != 2 && num_dims != 3) || encoder_hidden <= 0 || decoder_hidden <= 0 || rnn_hidden <= 0 || num_edge_types < 1 ||
        num_edge_types > 4 || n_nodes <= 0 || n_edges <= 0)
        return 0;
    return S2SStepLayout(num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_hidden, num_edge_types, n_nodes, n_edges).total;
}

int aether_s2s_step(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                    const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                    int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                    int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                    const float* inputs, const float* ext_field, const float* decoder_hidden_in, const float* h0, const float* c0,
                    const float* uniform, void* workspace, size_t workspace_bytes, float* outputs, float* decoder_hidden_out,
                    float* h1, float* c1, float* edges_out, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    if (int rc = s2s_entry_check("s2s_step", false, fp, pp, dp, nullptr, plan, z, ext_field == nullptr,
                                 send && recv && order && rowptr && inputs && decoder_hidden_in && h0 && c0 && uniform &&
                                     workspace && outputs && decoder_hidden_out && h1 && c1,
                                 0, 1)) return rc;
    return s2s_run_step("s2s_step", s2s_step_args(fp, pp, dp, nullptr, plan, z, send, recv, order, rowptr), workspace,
                        workspace_bytes, {inputs, decoder_hidden_in, h0, c0}, ext_field, uniform,
                        {outputs, decoder_hidden_out, h1, c1}, edges_out, stream);
}

int aether_s2s_rollout(const AetherS2SFieldParams* fp, const AetherS2SPriorParams* pp, const AetherS2SDecoderParams* dp,
                       const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                       int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                       int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                       int burn_in_steps, const float* burn_in, int steps, const float* inputs, float* decoder_state, float* h,
                       float* c, const float* uniform, void* workspace, size_t workspace_bytes, float* predictions,
                       float* edges_out, void* stream) {
    const S2SSizes z{num_dims, encoder_hidden, decoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, skip_first,
                     polar, num_vars, tau, n_nodes, n_edges};
    if (int rc = s2s_entry_check("s2s_rollout", false, fp, pp, dp, nullptr, plan, z, true,
                                 send && recv && order && rowptr && inputs && decoder_state && h && c && uniform && workspace &&
                                     (steps <= 0 || predictions) && (burn_in_steps <= 0 || burn_in),
                                 burn_in_steps, steps)) return rc;
    return s2s_run_rollout("s2s_rollout", s2s_step_args(fp, pp, dp, nullptr, plan, z, send, recv, order, rowptr), workspace,
                           workspace_bytes, burn_in_steps, burn_in, steps, inputs, decoder_state, h, c, uniform, predictions,
                           edges_out, stream);
}
