// edge_acc.h -- edge MLP backward of one layer for LARGE graphs with the layer's edge-level weight gradients
// accumulated on chip.  Included after backward.h and fused_bwd.h.
//
// backward.h's kb_edge writes, per edge and layer, the rows G = dL/dpre1, h and dpre2 (768 B) for k_outer to multiply
// afterwards (which reads them again, with e_prev: 1 KB): at the 33.5 M-edge shard of BASELINE config 5 that is 34 GB of
// HBM traffic per layer for the two products and 24 ms of a 106 ms training step (profiles/r02_cfg5shard_bench.json).
// kb_edge_acc8 stages the tile's operands in wave-private LDS rows and accumulates
//     dW2 += dpre2 (x) h          dW_e += G (x) e_prev   (layer 1: dW1 += G (x) features)         db2 += dpre2, db1 += G
// in registers over all tiles of the workgroup, as k_fused_bwd does for small graphs; only G (read by the node-sum kernels)
// and the message gradient DE / DA still go to memory.  Every workgroup writes its partial, k_edge_acc8_reduce adds the
// partials in workgroup order (fixed 16-group tree): no atomics, bit-stable.  Used when the deferred all-in-one product
// launch does not apply (E > outer_defer_max_edges).
#pragma once

namespace {

// Two waves per SIMD (round 4):
//   * the transposed products (W2^T dpre2, W_in^T G) read the forward's split images transposed (gemm_split_T): two images
//     in LDS;
//   * the weight-gradient accumulators are partitioned by output rows: a workgroup works in ROUNDS of NW tiles (one per
//     wave); after a round's tiles are staged, wave w adds the rows 16 (w & 3) .. of the product over the four tiles
//     4 (w >> 2) .. of the round -- 16 accumulator registers per product, nothing to reduce over the waves but the tile
//     halves, which go out as NW / 4 partials per workgroup;
//   * bias sums ride along as one more MFMA per k step against a column of ones.
// The library launches NW = 4: TWO workgroups of four waves per CU, <= 256 registers.  (Eight waves of one workgroup take
// their barriers together, so a SIMD's two waves are always in the SAME phase -- both in their GEMMs, then both in their
// weight-gradient products -- and nothing overlaps; two independent workgroups drift apart.)
// The staged tensors are the fp16 pieces their GEMMs make (fused_bwd.h: fb_stage_pieces), the weight-gradient products
// run on the 16-bit matrix pipe from transposed reads with per-tile power-of-two scales (fb_outer16_issue /
// fb_outer16_consume).  LDS per workgroup: 2 x 16 KB images + 4 x 8.5 KB staging = 67 KB.
constexpr int EA8_WAVE_STG = 2 * 16 * FB_SA;     // staging floats per wave: one operand pair at a time, as fp16 pieces
__host__ __device__ constexpr size_t ea8_lds_bytes(int nw) { return (size_t)(2 * SPLIT_WIMG + nw * EA8_WAVE_STG + 2 * nw) * 4; }
template <bool FIRST, int NW>
__global__ void __launch_bounds__(64 * NW, NW == 4 ? 2 : 1)
kb_edge_acc8(const float* __restrict__ b_in, const float* __restrict__ b2g, const float* __restrict__ Ps,
             const float* __restrict__ Pr, const float* __restrict__ e_prev, const float* __restrict__ feat,
             const int32_t* __restrict__ send_s, const int32_t* __restrict__ recv_s, const int32_t* __restrict__ rowptr,
             const float* __restrict__ DN, float* __restrict__ DE, int have_de, float* __restrict__ G,
             float* __restrict__ DA, float* __restrict__ partial /* [n_wgs][2][FB_PART] */,
             const float* __restrict__ img_in /*split image of W_e (FIRST: of W1, K padded to 32)*/,
             const float* __restrict__ img_2 /*split image of W2*/, int64_t n_edges, int n_wgs) {
    constexpr int NBE = FIRST ? 2 : 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wi = smem;                  // split image of W_in (FIRST: half of it is used)
    float* w2 = wi + SPLIT_WIMG;       // split image of W2
    float* stg = w2 + SPLIT_WIMG;      // [NW waves][2 arrays][2 fp16 pieces][16][FB_RH bytes] (fused_bwd.h: fb_stage_pieces)
    constexpr int EA8_STG = EA8_WAVE_STG;
    float* scl = stg + NW * EA8_STG;   // [NW][2]: the staged pair's 1 / (s_x s_y), 1 / s_x
    static_assert(NW == 4 || NW == 8, "one or two groups of four row quarters");
    for (int idx = threadIdx.x; idx < (FIRST ? SPLIT_WIMG / 2 : SPLIT_WIMG) / 4; idx += 64 * NW) st4(wi + 4 * idx, ld4(img_in + 4 * idx));
    for (int idx = threadIdx.x; idx < SPLIT_WIMG / 4; idx += 64 * NW) st4(w2 + 4 * idx, ld4(img_2 + 4 * idx));
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, q = lane >> 4;
    float* sa = stg + wave * EA8_STG;   // dpre2, then G
    float* sb = sa + 16 * FB_SA;        // h, then e_prev / features
    const int wq = wave & 3, whalf = wave >> 2;          // accumulator rows 16 wq .., tiles 4 whalf .. of a round
    const int64_t tiles = (n_edges + 15) >> 4;
    const int64_t stride = (int64_t)n_wgs * NW;
    f32x4 accW2[4], accWe[NBE], bs2 = f32x4{0.f, 0.f, 0.f, 0.f}, bs1 = bs2;
#pragma unroll
    for (int b = 0; b < 4; ++b) accW2[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NBE; ++b) accWe[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto clampk = [&](int64_t tt) { const int64_t k = 16 * tt + i; return k < n_edges ? k : n_edges - 1; };
    // the HBM stream of the next round (e_prev / features and the incoming message gradient) is requested a round ahead;
    // the gathered rows (P_s, P_r, dn: L2 hits) when the tile starts -- the SIMD's other wave covers that round trip
    f32x4 nbop[4], ndev[4];
    int64_t t0 = (int64_t)blockIdx.x * NW;
    {
        const int64_t k0 = clampk(t0 + wave < tiles ? t0 + wave : tiles - 1);
        if (FIRST) { nbop[0] = ld4(feat + k0 * FPAD + 4 * q); nbop[1] = ld4(feat + k0 * FPAD + 16 + 4 * q); }
        else load_tile64(nbop, e_prev, k0, H, q);
        if (have_de) load_tile64(ndev, DE, k0, H, q);
    }
    for (; t0 < tiles; t0 += stride) {                   // rounds: workgroup-uniform
        const int64_t t = t0 + wave;
        const bool active = t < tiles;                   // wave-uniform
        f32x4 g[4], bop[4];
        SplitScale s_ep{false, 1.0f, 1.0f}, s_g{false, 1.0f, 1.0f};
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) { g[mb] = f32x4{0.f, 0.f, 0.f, 0.f}; bop[mb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        if (active) {
            const int64_t k = 16 * t + i;
            const bool ok = k < n_edges;
            const int64_t kc = ok ? k : n_edges - 1;
            const int32_t s = send_s[kc], r = recv_s[kc];
            const int deg = rowptr[r + 1] - rowptr[r];
            f32x4 p1[4], dnv[4], dev[4];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) { bop[mb] = nbop[mb]; dev[mb] = ndev[mb]; }
            if (FIRST) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) p1[mb] = ld4(b_in + 16 * mb + 4 * q);
            } else {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
                    p1[mb] = ld4(Ps + (int64_t)s * H + 16 * mb + 4 * q) + ld4(Pr + (int64_t)r * H + 16 * mb + 4 * q);
            }
            load_tile64(dnv, DN, r, H, q);
            {   // next round's stream
                const int64_t tn = t + stride < tiles ? t + stride : t;
                const int64_t kn = clampk(tn);
                if (FIRST) { nbop[0] = ld4(feat + kn * FPAD + 4 * q); nbop[1] = ld4(feat + kn * FPAD + 16 + 4 * q); }
                else load_tile64(nbop, e_prev, kn, H, q);
                if (have_de) load_tile64(ndev, DE, kn, H, q);
            }
            const float inv = own_reg(1.0f / (float)(deg > 1 ? deg : 1));
            // ---- forward recompute: pre1, h = silu(pre1), pre2
            f32x4 p2[4], h[4], sg1[4];
            if (FIRST) {
                f32x4 b2[2] = {bop[0], bop[1]};
                f16x8 ph[1], pl[1];
                s_ep = gemm_split_keep<4, 1>(wi, b2, p1, lane, ph, pl);
            } else {
                f16x8 ph[2], pl[2];
                s_ep = gemm_split_keep<4, 2>(wi, bop, p1, lane, ph, pl);
            }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                sg1[mb] = sigmoid4(p1[mb]);
                h[mb] = p1[mb] * sg1[mb];
                p2[mb] = ld4(b2g + 16 * mb + 4 * q);
            }
            SplitScale s_h;
            {   // h's pieces go to the staging rows as its GEMM makes them
                f16x8 ph[2], pl[2];
                s_h = gemm_split_keep<4, 2>(w2, h, p2, lane, ph, pl);
                fb_stage_pieces<2>(sb, i, q, ph, pl);
            }
            // ---- de = dn[recv] / deg (+ gradient through the next layer's edge input); back through both Linears
            f32x4 d2[4], dh[4];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                f32x4 de = dnv[mb] * inv;
                if (have_de) de += dev[mb];
                d2[mb] = de * dsilu_from_sigmoid(p2[mb], sigmoid4(p2[mb]));
                if (!ok) d2[mb] = f32x4{0.f, 0.f, 0.f, 0.f};             // rows past the end contribute nothing to the products
                dh[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            {
                f16x8 ph[2], pl[2];
                const SplitScale s_d2 = gemm_split_T_keep<2>(w2, d2, dh, lane, ph, pl);        // W2^T dpre2 from the forward's image
                fb_stage_pieces<2>(sa, i, q, ph, pl);
                if (lane == 0) { scl[2 * wave] = s_d2.inv_s * s_h.inv_s; scl[2 * wave + 1] = s_d2.inv_s; }
            }
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) g[mb] = dh[mb] * dsilu_from_sigmoid(p1[mb], sg1[mb]);
            if (FIRST) {
                f32x4 da[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
                f16x8 ph[2], pl[2];
                s_g = gemm_split_T_keep<1>(wi, g, da, lane, ph, pl);    // W1^T G
                if (ok) { st4(DA + k * FPAD + 4 * q, da[0]); st4(DA + k * FPAD + 16 + 4 * q, da[1]); }
            } else {
                f32x4 dep[4];
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) dep[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
                f16x8 ph[2], pl[2];
                s_g = gemm_split_T_keep<2>(wi, g, dep, lane, ph, pl);   // W_e^T G
                if (ok) store_tile64(DE, k, H, q, dep);
            }
            if (ok) store_tile64(G, k, H, q, g);
            if (!ok) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) bop[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        // ---- dW2 += dpre2 (x) h, db2: the round's tiles are staged; this wave's row quarter over its four tiles
        lds_barrier();
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            if (t0 + 4 * whalf + tt < tiles) {
                const float* ta = stg + (4 * whalf + tt) * EA8_STG;
                const float c0 = scl[2 * (4 * whalf + tt)], c1 = scl[2 * (4 * whalf + tt) + 1];
                const unsigned lo_ = fb_tr_lane_offset(lane);
                FbOuterRegs<4> R;
                fb_outer16_issue<4>(fb_lds_addr(ta) + lo_ + 32u * (unsigned)wq, fb_lds_addr(ta + 16 * FB_SA) + lo_, R);
                fb_outer16_consume<4, true, 0>(R, accW2, bs2, c0, c1);
            }
        }
        lds_barrier();
        // ---- dW_e += G (x) e_prev (layer 1: dW1 += G (x) features, db1)
        if (active) {                      // (the pieces are made again from the live tiles, with the scales their GEMMs used: 40 vector
                                           //  instructions per tensor against 32 registers held across the first product)
            f16x8 ph[2], pl[2];
            split8(g[0] * s_g.s, g[1] * s_g.s, ph[0], pl[0]);          // (g of a row past the end is 0: dh = W2^T 0)
            split8(g[2] * s_g.s, g[3] * s_g.s, ph[1], pl[1]);
            fb_stage_pieces<2>(sa, i, q, ph, pl);
            split8(bop[0] * s_ep.s, bop[1] * s_ep.s, ph[0], pl[0]);
            if constexpr (FIRST) {
                const f16x8 h1[1] = {ph[0]}, l1[1] = {pl[0]};
                fb_stage_pieces<1>(sb, i, q, h1, l1);
            } else {
                split8(bop[2] * s_ep.s, bop[3] * s_ep.s, ph[1], pl[1]);
                fb_stage_pieces<2>(sb, i, q, ph, pl);
            }
            if (lane == 0) { scl[2 * wave] = s_g.inv_s * s_ep.inv_s; scl[2 * wave + 1] = s_g.inv_s; }
        }
        lds_barrier();
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            if (t0 + 4 * whalf + tt < tiles) {
                const float* ta = stg + (4 * whalf + tt) * EA8_STG;
                const float c0 = scl[2 * (4 * whalf + tt)], c1 = scl[2 * (4 * whalf + tt) + 1];
                const unsigned lo_ = fb_tr_lane_offset(lane);
                FbOuterRegs<NBE> R;
                fb_outer16_issue<NBE>(fb_lds_addr(ta) + lo_ + 32u * (unsigned)wq, fb_lds_addr(ta + 16 * FB_SA) + lo_, R);
                fb_outer16_consume<NBE, FIRST, 0>(R, accWe, bs1, c0, c1);
            }
        }
        lds_barrier();
    }
    // ---- two partials per workgroup (tile halves 0 / 1), each wave its row quarter: [dW2 64 x 64 | dW_e 64 x 64 (64 x 32) | db2 | db1]
    float* dst = partial + ((size_t)blockIdx.x * (NW / 4) + whalf) * FB_PART;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
        const int mrow = 16 * wq + 4 * q + r4;           // accumulator block nb holds columns 16 nb + i
#pragma unroll
        for (int nbx = 0; nbx < 4; ++nbx) dst[mrow * H + 16 * nbx + i] = accW2[nbx][r4];
        if constexpr (FIRST) {
            dst[H * H + mrow * FPAD + i] = accWe[0][r4];
            dst[H * H + mrow * FPAD + 16 + i] = accWe[1][r4];
        } else {
#pragma unroll
            for (int nbx = 0; nbx < 4; ++nbx) dst[H * H + mrow * H + 16 * nbx + i] = accWe[nbx][r4];
        }
        if (i == 0) {
            dst[2 * H * H + mrow] = bs2[r4];
            dst[2 * H * H + H + mrow] = FIRST ? bs1[r4] : 0.0f;
        }
    }
}

// The gradient tensors k_edge_acc8_reduce writes.
struct EdgeAccOut {
    float* w2; float* b2;              // [64][64], [64]
    float* we; int ldwe; int ncols;    // dW_e -> we[m * ldwe + n], n < ncols (layer 1: [64][F1], NB = 2; else columns 128..191 of [64][192])
    float* b1;                         // layer 1 only (layers 2-4: the bias gradient comes with dP_r)
    int nb_e;                          // 2 (layer 1) or 4
};

// Sum of kb_edge_acc8's partials ([n_parts][FB_PART], part order = workgroup order, fixed 16-group tree) into the gradient
// tensors.  Element e < H*H: dW2[m][n]; < 2 H*H: dW_e (layer 1: [64][FPAD] rows, columns < f1); then db2, db1.
__global__ void __launch_bounds__(1024)
k_edge_acc8_reduce(const float* __restrict__ partial, int n_parts, EdgeAccOut O) {
    const int t = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + t;
    const bool valid = e < FB_PART;
    const int per = (n_parts + 15) / 16;
    const int w0 = grp * per, w1 = w0 + per < n_parts ? w0 + per : n_parts;
    float s = 0.0f;
    if (valid)
        for (int w = w0; w < w1; ++w) s += partial[(size_t)w * FB_PART + e];
    __shared__ float red[16][64];
    red[grp][t] = s;
    __syncthreads();
    if (grp != 0 || !valid) return;
    float tot = red[0][t];
#pragma unroll
    for (int g = 1; g < 16; ++g) tot += red[g][t];
    if (e < H * H) {
        O.w2[e] = tot;
    } else if (e < 2 * H * H) {
        const int o = e - H * H;
        if (O.nb_e == 2) {                               // layer 1: [64][FPAD]
            const int mrow = o / FPAD, c = o % FPAD;
            if (o < H * FPAD && c < O.ncols) O.we[(size_t)mrow * O.ldwe + c] = tot;
        } else {
            O.we[(size_t)(o >> 6) * O.ldwe + (o & 63)] = tot;
        }
    } else if (e < 2 * H * H + H) {
        O.b2[e - 2 * H * H] = tot;
    } else if (O.b1 != nullptr) {
        O.b1[e - 2 * H * H - H] = tot;
    }
}

}  // namespace
