// egnn.h -- EGNN-Aether (EGNN_vel_Aether, nn/state2state/egnn_aether.py) forward and parameter backward, gfx950.
//
// One workgroup of H threads (H = hidden_nf, 64 or 128) owns one node r and the edges whose FIRST index is r
// (row = edges[0]: every aggregation of E_GCL runs over it, nn/state2state/egnn/gcl.py:69-70,95-101).  The row-sorted
// view is aether_graph_build called with the two index rows swapped: its rowptr / perm / send_s are then the CSR by
// row, and its sender lists (sperm / srowptr) group the same sorted positions by col.  Sums run over a node's edges in
// that stable order: no float atomics, bit-identical from run to run.
//
// Thread j owns output channel j of every H-wide layer.  Forward products read transposed weight images ([in][H], one
// coalesced row per input channel; k_egnn_wt writes them per call); backward products W^T g read the torch layout
// [out][in] directly, which is then the coalesced one.  Everything is fp32 on the vector ALU, including the two
// H -> 1 projections (phi's last layer is initialised with xavier gain 0.001, |w| ~ 3e-4): no fp16 operand anywhere.
//
// Edge input layout (edge_mlp.0, 2H + 9 columns, gcl.py:54-57 + egnn/gcl.py:62-66):
//   [h[row] (H) | h[col] (H) | radial | edge_attr (2) | f[row] (3) | f[col] (3)]

#pragma once

#include "gnn_common.h"

namespace egnn {

constexpr int EB = 4;            // edges of one node processed side by side (each weight load feeds EB products)
constexpr int FIN = 22;          // field net input: x (3), vel (3), class embedding (16)
constexpr int FH = 32;           // field net hidden width
constexpr int WG_CH_MAX = 256;   // row chunks of a weight-gradient reduction (partials summed in chunk order)

using gnn::dsilu;
using gnn::sig;
using gnn::silu;
using gnn::WgJob;
using gnn::WgJobs;

// one layer's parameters: transposed images (t suffix, [in][H]) for the forward products, torch layout for W^T g
struct LayerW {
    const float *e_w0t, *e_w2t, *c_w0t, *n_w0t, *n_w2t, *v_w0t;
    const float *e_w0, *e_b0, *e_w2, *e_b2, *n_w0, *n_b0, *n_w2, *n_b2, *c_w0, *c_b0, *c_w2, *v_w0, *v_b0, *v_w2, *v_b2;
};

struct FieldW { const float *w0, *b0, *w2, *b2, *w4, *b4, *emb; };

// transposed images of one layer's six H-row matrices: blockIdx.y picks the matrix
struct WtJob { const float* src[6]; float* dst[6]; int cols[6]; };

template <int H>
__global__ __launch_bounds__(256) void k_egnn_wt(WtJob J) {
    const int m = blockIdx.y;
    const int cols = J.cols[m];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // destination index k * H + j
    if (i >= (int64_t)cols * H) return;
    const int k = (int)(i / H), j = (int)(i % H);
    J.dst[m][i] = J.src[m][(int64_t)j * cols + k];
}

__device__ __forceinline__ int class_index(float q) {        // (charges + 1).long(), aether.py:123-124
    int c = (int)(q + 1.0f);
    return c < 0 ? 0 : (c > 2 ? 2 : c);
}

// field net (aether.py:108-134) and embedding (egnn_aether.py:37) of node r; F[r][3], h0[r][H]
template <int H>
__global__ __launch_bounds__(H) void k_egnn_prep(FieldW fw, const float* __restrict__ emb_w, const float* __restrict__ emb_b,
                                                 int in_nf, const float* __restrict__ hin, const float* __restrict__ x,
                                                 const float* __restrict__ vel, const float* __restrict__ charges,
                                                 float* __restrict__ F, float* __restrict__ h0) {
    const int64_t r = blockIdx.x;
    const int j = threadIdx.x;
    __shared__ float fin[FIN], z1[FH], z2[FH];
    if (j < 3) { fin[j] = x[r * 3 + j]; fin[3 + j] = vel[r * 3 + j]; }
    if (j < 16) fin[6 + j] = fw.emb[class_index(charges[r]) * 16 + j];
    float hv = emb_b[j];
    for (int k = 0; k < in_nf; ++k) hv += emb_w[(int64_t)j * in_nf + k] * hin[r * in_nf + k];
    h0[r * H + j] = hv;
    __syncthreads();
    if (j < FH) {
        float a = fw.b0[j];
        for (int k = 0; k < FIN; ++k) a += fw.w0[j * FIN + k] * fin[k];
        z1[j] = silu(a);
    }
    __syncthreads();
    if (j < FH) {
        float a = fw.b2[j];
        for (int k = 0; k < FH; ++k) a += fw.w2[j * FH + k] * z1[k];
        z2[j] = silu(a);
    }
    __syncthreads();
    if (j < 3) {
        float a = fw.b4[j];
        for (int k = 0; k < FH; ++k) a += fw.w4[j * FH + k] * z2[k];
        F[r * 3 + j] = a;
    }
}

template <int H>
__device__ __forceinline__ void reduce_rows(float (&red)[EB][H], int j) {    // red[e][0] = sum over j, fixed tree
#pragma unroll
    for (int s = H / 2; s > 0; s >>= 1) {
        if (j < s)
#pragma unroll
            for (int e = 0; e < EB; ++e) red[e][j] += red[e][j + s];
        __syncthreads();
    }
}

// Edge inputs of a chunk: h[col] rows into hc, and per edge {radial, ea0, ea1, f[col] 0..2, d 0..2} into ext.
template <int H>
__device__ __forceinline__ void load_chunk(int j, int base, int ne, const float* __restrict__ h, const float* __restrict__ x,
                                           const float* __restrict__ F, const float* __restrict__ ea, const int32_t* __restrict__ perm,
                                           const int32_t* __restrict__ col_s, const float (&xr)[3], float (&hc)[EB][H],
                                           float (&ext)[EB][12]) {
    for (int e = 0; e < ne; ++e) hc[e][j] = h[(int64_t)col_s[base + e] * H + j];
    if (j < ne) {
        const int64_t c = col_s[base + j], oe = perm[base + j];
        const float d0 = xr[0] - x[c * 3], d1 = xr[1] - x[c * 3 + 1], d2 = xr[2] - x[c * 3 + 2];
        ext[j][0] = d0 * d0 + d1 * d1 + d2 * d2;
        ext[j][1] = ea[oe * 2];
        ext[j][2] = ea[oe * 2 + 1];
        ext[j][3] = F[c * 3]; ext[j][4] = F[c * 3 + 1]; ext[j][5] = F[c * 3 + 2];
        ext[j][6] = d0; ext[j][7] = d1; ext[j][8] = d2;
    }
}

// pre-activation of edge_mlp.0 for the chunk's edges: the h[row] / f[row] part (pre) is the node's, shared by its edges
template <int H>
__device__ __forceinline__ void edge_mlp0(const LayerW& W, int j, float pre, const float (&hc)[EB][H], const float (&ext)[EB][12],
                                          float (&a)[EB]) {
    constexpr int KIN = 2 * H + 9;
#pragma unroll
    for (int e = 0; e < EB; ++e) a[e] = pre;
    for (int k = 0; k < H; ++k) {
        const float w = W.e_w0t[(H + k) * H + j];
#pragma unroll
        for (int e = 0; e < EB; ++e) a[e] += w * hc[e][k];
    }
    // radial, edge_attr (2): columns 2H .. 2H+2; f[col]: 2H+6 .. 2H+8
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int col = q < 3 ? 2 * H + q : 2 * H + 3 + q;
        const float w = W.e_w0t[col * H + j];
#pragma unroll
        for (int e = 0; e < EB; ++e) a[e] += w * ext[e][q];
    }
    (void)KIN;
}

template <int H>
__device__ __forceinline__ float node_pre(const LayerW& W, int j, const float* hr, const float (&fr)[3]) {
    float pre = W.e_b0[j];
    for (int k = 0; k < H; ++k) pre += W.e_w0t[k * H + j] * hr[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) pre += W.e_w0t[(2 * H + 3 + i) * H + j] * fr[i];
    return pre;
}

// phi's output and the translation of one edge (egnn/gcl.py:92-96 with coord2radial :104-113)
template <bool NORM, bool TANH>
__device__ __forceinline__ void edge_trans(const float* ext, float phi0, float (&dn)[3], float& phi, float (&raw)[3]) {
    float s = 1.0f;
    if (NORM) s = sqrtf(ext[0]) + 1.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) dn[i] = NORM ? ext[6 + i] / s : ext[6 + i];
    phi = TANH ? tanhf(phi0) : phi0;
#pragma unroll
    for (int i = 0; i < 3; ++i) raw[i] = dn[i] * phi;
}

__device__ __forceinline__ float clamp100(float v) { return fminf(fmaxf(v, -100.0f), 100.0f); }

// One E_GCL_vel_field layer (gcl.py:59-83), node r per workgroup: edge MLP + phi over r's edges, the row sums of m and
// of the clamped translations, then psi (coord_mlp_vel), the x update, node_mlp and the residual.
// Reads h / x (the layer's input), writes h_out / x_out (+ x_out2 when not null: the caller's output of the last layer)
// and, when agg_out is not null, the row sums of m (kept for the backward).
template <int H, bool NORM, bool TANH>
__global__ __launch_bounds__(H) void k_egnn_layer(LayerW W, const float* __restrict__ h, const float* __restrict__ x,
                                                  const float* __restrict__ vel, const float* __restrict__ F,
                                                  const float* __restrict__ ea, const int32_t* __restrict__ perm,
                                                  const int32_t* __restrict__ col_s, const int32_t* __restrict__ rowptr,
                                                  float* __restrict__ h_out, float* __restrict__ x_out,
                                                  float* __restrict__ x_out2, float* __restrict__ agg_out) {
    const int64_t r = blockIdx.x;
    const int j = threadIdx.x;
    __shared__ float hr[H], agg[H];
    __shared__ float hc[EB][H], z1[EB][H], mm[EB][H], red[EB][H];
    __shared__ float ext[EB][12];
    hr[j] = h[r * H + j];
    const float xr[3] = {x[r * 3], x[r * 3 + 1], x[r * 3 + 2]};
    const float fr[3] = {F[r * 3], F[r * 3 + 1], F[r * 3 + 2]};
    __syncthreads();
    const float pre = node_pre<H>(W, j, hr, fr);
    const int e0 = rowptr[r], e1 = rowptr[r + 1];
    float msum = 0.0f, ts[3] = {0.0f, 0.0f, 0.0f};
    for (int base = e0; base < e1; base += EB) {
        const int ne = e1 - base < EB ? e1 - base : EB;
        load_chunk<H>(j, base, ne, h, x, F, ea, perm, col_s, xr, hc, ext);
        __syncthreads();
        float a[EB];
        edge_mlp0<H>(W, j, pre, hc, ext, a);
#pragma unroll
        for (int e = 0; e < EB; ++e) z1[e][j] = silu(a[e]);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) a[e] = W.e_b2[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.e_w2t[k * H + j];
#pragma unroll
            for (int e = 0; e < EB; ++e) a[e] += w * z1[e][k];
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const float m = silu(a[e]);
            mm[e][j] = m;
            if (e < ne) msum += m;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) a[e] = W.c_b0[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.c_w0t[k * H + j];
#pragma unroll
            for (int e = 0; e < EB; ++e) a[e] += w * mm[e][k];
        }
        const float wc = W.c_w2[j];
#pragma unroll
        for (int e = 0; e < EB; ++e) red[e][j] = wc * silu(a[e]);
        __syncthreads();
        reduce_rows<H>(red, j);
        if (j == 0) {
            for (int e = 0; e < ne; ++e) {
                float dn[3], phi, raw[3];
                edge_trans<NORM, TANH>(ext[e], red[e][0], dn, phi, raw);
#pragma unroll
                for (int i = 0; i < 3; ++i) ts[i] += clamp100(raw[i]);
            }
        }
        __syncthreads();
    }
    agg[j] = msum;
    if (agg_out) agg_out[r * H + j] = msum;
    __syncthreads();
    // psi = coord_mlp_vel([h, f]) (gcl.py:80) and node_mlp([h, agg]) (egnn/gcl.py:79-89), both on the layer's input h
    float p = W.v_b0[j], n = W.n_b0[j];
    for (int k = 0; k < H; ++k) {
        p += W.v_w0t[k * H + j] * hr[k];
        n += W.n_w0t[k * H + j] * hr[k] + W.n_w0t[(H + k) * H + j] * agg[k];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) p += W.v_w0t[(H + i) * H + j] * fr[i];
    red[0][j] = W.v_w2[j] * silu(p);
    z1[0][j] = silu(n);
    __syncthreads();
    float o = W.n_b2[j];
    for (int k = 0; k < H; ++k) o += W.n_w2t[k * H + j] * z1[0][k];
    h_out[r * H + j] = hr[j] + o;
#pragma unroll
    for (int s = H / 2; s > 0; s >>= 1) {
        if (j < s) red[0][j] += red[0][j + s];
        __syncthreads();
    }
    if (j == 0) {
        const float psi = red[0][0] + W.v_b2[0];
        const int cnt = e1 - e0 > 1 ? e1 - e0 : 1;                  // count.clamp(min=1), gnn/gcl.py:210
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float v = (xr[i] + ts[i] / (float)cnt) + psi * vel[r * 3 + i];
            x_out[r * 3 + i] = v;
            if (x_out2) x_out2[r * 3 + i] = v;
        }
    }
}

// ------------------------------------------------------------------ backward
// Per-layer scratch of the backward (row-sorted edge positions for the [E] arrays)
struct BwdBufs {
    float *gh_in, *gx_in, *gf;                       // results: d/dh, d/dx of the layer's input; d/dF accumulated
    float *ghn, *gagg, *zn, *gn1, *zp, *gp1, *gpsi, *gxm, *gfn, *ghe, *gxe, *gfe;   // [n] rows
    float *in, *z1, *m, *z3, *ga1, *ga2, *gc1, *gphi, *ghc, *gd, *gfc;            // [E] rows
};

// node part of a layer's backward: node_mlp + residual, psi, and the mean's d/dt per row
template <int H>
__global__ __launch_bounds__(H) void kb_egnn_node(LayerW W, BwdBufs B, const float* __restrict__ h, const float* __restrict__ aggl,
                                                  const float* __restrict__ vel, const float* __restrict__ F,
                                                  const int32_t* __restrict__ rowptr, const float* __restrict__ gh_out,
                                                  const float* __restrict__ gx_out) {
    const int64_t r = blockIdx.x;
    const int j = threadIdx.x;
    __shared__ float hr[H], agg[H], g2[H], gn1s[H], gp1s[H];
    hr[j] = h[r * H + j];
    agg[j] = aggl[r * H + j];
    g2[j] = gh_out[r * H + j];
    const float fr[3] = {F[r * 3], F[r * 3 + 1], F[r * 3 + 2]};
    const float gx[3] = {gx_out[r * 3], gx_out[r * 3 + 1], gx_out[r * 3 + 2]};
    __syncthreads();
    float p = W.v_b0[j], n = W.n_b0[j];
    for (int k = 0; k < H; ++k) {
        p += W.v_w0t[k * H + j] * hr[k];
        n += W.n_w0t[k * H + j] * hr[k] + W.n_w0t[(H + k) * H + j] * agg[k];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) p += W.v_w0t[(H + i) * H + j] * fr[i];
    float gzn = 0.0f;
    for (int i = 0; i < H; ++i) gzn += W.n_w2[i * H + j] * g2[i];
    const float gn1 = gzn * dsilu(n);
    const float gpsi = gx[0] * vel[r * 3] + gx[1] * vel[r * 3 + 1] + gx[2] * vel[r * 3 + 2];
    const float gp1 = gpsi * W.v_w2[j] * dsilu(p);
    B.zn[r * H + j] = silu(n);
    B.gn1[r * H + j] = gn1;
    B.zp[r * H + j] = silu(p);
    B.gp1[r * H + j] = gp1;
    gn1s[j] = gn1;
    gp1s[j] = gp1;
    __syncthreads();
    float gh = g2[j], ga = 0.0f;
    for (int i = 0; i < H; ++i) {
        gh += W.n_w0[i * 2 * H + j] * gn1s[i] + W.v_w0[i * (H + 3) + j] * gp1s[i];
        ga += W.n_w0[i * 2 * H + H + j] * gn1s[i];
    }
    B.ghn[r * H + j] = gh;
    B.gagg[r * H + j] = ga;
    if (j < 3) {
        float gf = 0.0f;
        for (int i = 0; i < H; ++i) gf += W.v_w0[i * (H + 3) + H + j] * gp1s[i];
        B.gfn[r * 3 + j] = gf;
        const int e0 = rowptr[r], e1 = rowptr[r + 1];
        const int cnt = e1 - e0 > 1 ? e1 - e0 : 1;
        B.gxm[r * 3 + j] = gx[j] / (float)cnt;
    }
    if (j == 0) B.gpsi[r] = gpsi;
}

// edge part: recompute each edge of row r, back through phi, the clamp, coord2radial and edge_mlp; the row's own
// contributions (h[row], x[row], f[row]) are summed here in edge order, the col contributions are stored per edge
template <int H, bool NORM, bool TANH>
__global__ __launch_bounds__(H) void kb_egnn_edge(LayerW W, BwdBufs B, const float* __restrict__ h, const float* __restrict__ x,
                                                  const float* __restrict__ F, const float* __restrict__ ea,
                                                  const int32_t* __restrict__ perm, const int32_t* __restrict__ col_s,
                                                  const int32_t* __restrict__ rowptr) {
    constexpr int KIN = 2 * H + 9;
    const int64_t r = blockIdx.x;
    const int j = threadIdx.x;
    __shared__ float hr[H];
    __shared__ float hc[EB][H], z1[EB][H], mm[EB][H], red[EB][H];
    __shared__ float ext[EB][12], gphi0[EB], gtail[EB][9];
    hr[j] = h[r * H + j];
    const float xr[3] = {x[r * 3], x[r * 3 + 1], x[r * 3 + 2]};
    const float fr[3] = {F[r * 3], F[r * 3 + 1], F[r * 3 + 2]};
    const float gxm[3] = {B.gxm[r * 3], B.gxm[r * 3 + 1], B.gxm[r * 3 + 2]};
    const float gaggr = B.gagg[r * H + j];
    __syncthreads();
    const float pre = node_pre<H>(W, j, hr, fr);
    const int e0 = rowptr[r], e1 = rowptr[r + 1];
    float ghr = 0.0f, gxr[3] = {0.0f, 0.0f, 0.0f}, gfr[3] = {0.0f, 0.0f, 0.0f};
    for (int base = e0; base < e1; base += EB) {
        const int ne = e1 - base < EB ? e1 - base : EB;
        load_chunk<H>(j, base, ne, h, x, F, ea, perm, col_s, xr, hc, ext);
        __syncthreads();
        float a1[EB], a2[EB], c1[EB];
        edge_mlp0<H>(W, j, pre, hc, ext, a1);
#pragma unroll
        for (int e = 0; e < EB; ++e) z1[e][j] = silu(a1[e]);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) a2[e] = W.e_b2[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.e_w2t[k * H + j];
#pragma unroll
            for (int e = 0; e < EB; ++e) a2[e] += w * z1[e][k];
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) mm[e][j] = silu(a2[e]);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) c1[e] = W.c_b0[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.c_w0t[k * H + j];
#pragma unroll
            for (int e = 0; e < EB; ++e) c1[e] += w * mm[e][k];
        }
        const float wc = W.c_w2[j];
#pragma unroll
        for (int e = 0; e < EB; ++e) red[e][j] = wc * silu(c1[e]);
        // operands of the weight gradients, by sorted position (loops over e unrolled with a guard: a register array
        // indexed by a run-time bound would live in scratch memory)
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            if (e >= ne) continue;
            const int64_t pos = base + e;
            B.z1[pos * H + j] = z1[e][j];
            B.m[pos * H + j] = mm[e][j];
            B.z3[pos * H + j] = silu(c1[e]);
            for (int k = j; k < KIN; k += H) {
                float v;
                if (k < H) v = hr[k];
                else if (k < 2 * H) v = hc[e][k - H];
                else if (k < 2 * H + 3) v = ext[e][k - 2 * H];
                else if (k < 2 * H + 6) v = fr[k - 2 * H - 3];
                else v = ext[e][k - 2 * H - 3];
                B.in[pos * KIN + k] = v;
            }
        }
        __syncthreads();
        reduce_rows<H>(red, j);
        // phi, the clamp (torch: gradient where min <= v <= max), d/dphi0 and d/d(coord_diff) per edge
        if (j < ne) {
            float dn[3], phi, raw[3];
            edge_trans<NORM, TANH>(ext[j], red[j][0], dn, phi, raw);
            float gphi = 0.0f, gdn[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float gt = (raw[i] >= -100.0f && raw[i] <= 100.0f) ? gxm[i] : 0.0f;
                gphi += gt * dn[i];
                gdn[i] = gt * phi;
            }
            const float g0 = TANH ? gphi * (1.0f - phi * phi) : gphi;
            gphi0[j] = g0;
            B.gphi[base + j] = g0;
#pragma unroll
            for (int i = 0; i < 3; ++i) ext[j][9 + i] = gdn[i];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            const float g = gphi0[e] * wc * dsilu(c1[e]);
            red[e][j] = g;
            if (e < ne) B.gc1[(int64_t)(base + e) * H + j] = g;
        }
        __syncthreads();
        float g[EB];
#pragma unroll
        for (int e = 0; e < EB; ++e) g[e] = gaggr;                   // m feeds the row sum (node_mlp's agg) and phi
        for (int i = 0; i < H; ++i) {
            const float w = W.c_w0[i * H + j];
#pragma unroll
            for (int e = 0; e < EB; ++e) g[e] += w * red[e][i];
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            g[e] *= dsilu(a2[e]);
            if (e < ne) B.ga2[(int64_t)(base + e) * H + j] = g[e];
        }
        __syncthreads();                                             // red read above; z1 free as scratch
#pragma unroll
        for (int e = 0; e < EB; ++e) z1[e][j] = g[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EB; ++e) g[e] = 0.0f;
        for (int i = 0; i < H; ++i) {
            const float w = W.e_w2[i * H + j];
#pragma unroll
            for (int e = 0; e < EB; ++e) g[e] += w * z1[e][i];
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) {
            g[e] *= dsilu(a1[e]);
            red[e][j] = g[e];
            if (e < ne) B.ga1[(int64_t)(base + e) * H + j] = g[e];
        }
        __syncthreads();
        // d/d(edge input) = W0^T ga1: column k per thread, k = j, j + H, j + 2H (< KIN)
        for (int k = j; k < KIN; k += H) {
            float gi[EB];
#pragma unroll
            for (int e = 0; e < EB; ++e) gi[e] = 0.0f;
            for (int i = 0; i < H; ++i) {
                const float w = W.e_w0[i * KIN + k];
#pragma unroll
                for (int e = 0; e < EB; ++e) gi[e] += w * red[e][i];
            }
#pragma unroll
            for (int e = 0; e < EB; ++e) {
                if (e >= ne) continue;
                if (k < H) ghr += gi[e];
                else if (k < 2 * H) B.ghc[(int64_t)(base + e) * H + (k - H)] = gi[e];
                else gtail[e][k - 2 * H] = gi[e];
            }
        }
        __syncthreads();
        if (j == 0) {
            for (int e = 0; e < ne; ++e) {
                const int64_t pos = base + e;
                const float* d = &ext[e][6];
                const float* gdn = &ext[e][9];
                float grad = gtail[e][0], gd[3];
                if (NORM) {
                    const float sq = sqrtf(ext[e][0]), s = sq + 1.0f;
                    float gs = 0.0f;
#pragma unroll
                    for (int i = 0; i < 3; ++i) gs -= gdn[i] * d[i] / (s * s);
                    grad += gs * (0.5f / sq);
#pragma unroll
                    for (int i = 0; i < 3; ++i) gd[i] = gdn[i] / s + 2.0f * d[i] * grad;
                } else {
#pragma unroll
                    for (int i = 0; i < 3; ++i) gd[i] = gdn[i] + 2.0f * d[i] * grad;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    gxr[i] += gd[i];
                    gfr[i] += gtail[e][3 + i];
                    B.gd[pos * 3 + i] = gd[i];
                    B.gfc[pos * 3 + i] = gtail[e][6 + i];
                }
            }
        }
        __syncthreads();
    }
    B.ghe[r * H + j] = ghr;
    if (j == 0)
#pragma unroll
        for (int i = 0; i < 3; ++i) { B.gxe[r * 3 + i] = gxr[i]; B.gfe[r * 3 + i] = gfr[i]; }
}

// d/dh, d/dx of the layer's input and d/dF: the node's own terms + its col edges (sender lists of the view, in order)
template <int H>
__global__ __launch_bounds__(H) void kb_egnn_gather(BwdBufs B, const float* __restrict__ gx_out, const int32_t* __restrict__ sperm,
                                                    const int32_t* __restrict__ srowptr) {
    const int64_t v = blockIdx.x;
    const int j = threadIdx.x;
    const int q0 = srowptr[v], q1 = srowptr[v + 1];
    float gh = B.ghn[v * H + j] + B.ghe[v * H + j];
    for (int q = q0; q < q1; ++q) gh += B.ghc[(int64_t)sperm[q] * H + j];
    B.gh_in[v * H + j] = gh;
    if (j < 3) {
        float gx = gx_out[v * 3 + j] + B.gxe[v * 3 + j], gf = B.gfn[v * 3 + j] + B.gfe[v * 3 + j];
        for (int q = q0; q < q1; ++q) {
            const int64_t pos = sperm[q];
            gx -= B.gd[pos * 3 + j];
            gf += B.gfc[pos * 3 + j];
        }
        B.gx_in[v * 3 + j] = gx;
        B.gf[v * 3 + j] += gf;
    }
}

// field net backward per node: stores the operands of its weight gradients
struct FieldBufs { float *fin, *z1, *z2, *ga1, *ga2, *onehot, *gemb; };

__global__ __launch_bounds__(64) void kb_egnn_field(FieldW fw, FieldBufs Fb, const float* __restrict__ x,
                                                    const float* __restrict__ vel, const float* __restrict__ charges,
                                                    const float* __restrict__ gF) {
    const int64_t r = blockIdx.x;
    const int j = threadIdx.x;
    __shared__ float fin[FIN], z1[FH], z2[FH], g2[FH], g1[FH];
    const int cls = class_index(charges[r]);
    if (j < 3) { fin[j] = x[r * 3 + j]; fin[3 + j] = vel[r * 3 + j]; Fb.onehot[r * 3 + j] = j == cls ? 1.0f : 0.0f; }
    if (j < 16) fin[6 + j] = fw.emb[cls * 16 + j];
    __syncthreads();
    float a1 = 0.0f, a2 = 0.0f;
    if (j < FIN) Fb.fin[r * FIN + j] = fin[j];
    if (j < FH) {
        a1 = fw.b0[j];
        for (int k = 0; k < FIN; ++k) a1 += fw.w0[j * FIN + k] * fin[k];
        z1[j] = silu(a1);
        Fb.z1[r * FH + j] = z1[j];
    }
    __syncthreads();
    if (j < FH) {
        a2 = fw.b2[j];
        for (int k = 0; k < FH; ++k) a2 += fw.w2[j * FH + k] * z1[k];
        z2[j] = silu(a2);
        Fb.z2[r * FH + j] = z2[j];
        float g = 0.0f;
        for (int i = 0; i < 3; ++i) g += fw.w4[i * FH + j] * gF[r * 3 + i];
        g2[j] = g * dsilu(a2);
        Fb.ga2[r * FH + j] = g2[j];
    }
    __syncthreads();
    if (j < FH) {
        float g = 0.0f;
        for (int i = 0; i < FH; ++i) g += fw.w2[i * FH + j] * g2[i];
        g1[j] = g * dsilu(a1);
        Fb.ga1[r * FH + j] = g1[j];
    }
    __syncthreads();
    if (j < 16) {
        float g = 0.0f;
        for (int i = 0; i < FH; ++i) g += fw.w0[i * FIN + 6 + j] * g1[i];
        Fb.gemb[r * 16 + j] = g;
    }
}

// ------------------------------------------------------------------ weight gradients
// First stage of gnn_common.h's weight-gradient reduction: row chunk c of every 64 x 64 output tile -> part[c][...], a
// 4 x 4 block per thread.  No job here has an activation (WgJob::act is 0 and is not read).
__global__ __launch_bounds__(256) void k_egnn_wgrad_part(WgJobs T, float* __restrict__ part) {
    const int t = blockIdx.x, c = blockIdx.y;
    int q = 0;
    while (q + 1 < T.n && T.j[q + 1].tile0 <= t) ++q;
    const WgJob& J = T.j[q];
    const int tk = (J.K + 63) / 64;
    const int tt = t - J.tile0;
    const int j0 = (tt / tk) * 64 + (threadIdx.x / 16) * 4, k0 = (tt % tk) * 64 + (threadIdx.x % 16) * 4;
    const int64_t per = (J.rows + T.n_ch - 1) / T.n_ch;
    const int64_t i0 = c * per, i1 = i0 + per < J.rows ? i0 + per : J.rows;
    float acc[4][4] = {};
    for (int64_t i = i0; i < i1; ++i) {
        float g[4], a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            g[u] = j0 + u < J.J ? J.G[i * J.ldg + j0 + u] : 0.0f;
            a[u] = k0 + u < J.K ? (J.A ? J.A[i * J.lda + k0 + u] : 1.0f) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int w = 0; w < 4; ++w) acc[u][w] += g[u] * a[w];
    }
    float* P = part + (int64_t)c * T.n_out + J.poff;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (j0 + u < J.J && k0 + w < J.K) P[(j0 + u) * J.K + k0 + w] = acc[u][w];
}

}  // namespace egnn
