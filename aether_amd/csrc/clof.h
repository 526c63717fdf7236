// clof.h -- ClofNet (ClofNet / ClofNet_vel / ClofNet_vel_gbf, nn/state2state/clof/clof.py with Clof_GCL,
// nn/state2state/clof/gcl.py) forward and parameter backward, gfx950.
//
// Edges are grouped by row = edges[0] (every sum and mean of Clof_GCL runs over it, egnn/gcl.py:69-101): the row-sorted
// view is aether_graph_build with the two index rows swapped, so its rowptr / recv_s / send_s are the CSR by row and its
// sender lists (sperm / srowptr) group the same sorted positions by col.  Every edge-level buffer here is in sorted order.
// Sums run in a fixed order: no float atomics, two runs give identical bits.
//
// Edge MLPs on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, a k-ordered fma chain).  A wave owns
// CG groups of 16 edges; products are computed transposed, OUT^T[ch][edge] = W[ch][k] ACT^T[k][edge], so that
//   lane l holds edge (l & 15) and, in register i of channel block b, channel 16 b + 4 (l >> 4) + i
// for every activation.  An accumulator is then the B operand of the next layer as it stands: k-step (b, i) of the next
// product takes register i of block b, and the A operand (weights) of that k-step is W[16 mo + (l & 15)][16 b + 4 (l >> 4)
// + i] -- one 16-byte load per lane gives four k-steps.  Weights are read from packed images in the workspace
// (k_clof_pack), W and W^T, 16-byte aligned.  Node-level products (h_row / h_col blocks of edge_mlp.0, node_mlp,
// coord_mlp_vel, LayerNorm) are per-node vector loops, thread j = channel j.
//
// Weight gradients: fp32 MFMA with the rows (edges or nodes) as K, per job a 32 x 32 output tile per wave and a row chunk
// per workgroup; chunk partials are summed in chunk order by a second launch (gnn_common.h).

#pragma once

#include "gnn_common.h"

namespace clof {

constexpr int CG = 2;            // 16-edge groups per wave
constexpr int EW = 4;            // waves per edge workgroup
constexpr int ET = 16 * CG * EW; // edges per edge workgroup
constexpr int NB = 4;            // nodes per node workgroup
constexpr int FMAX = 16;         // fuse_edge input width (ClofNet 10, ClofNet_vel 16, ClofNet_vel_gbf 14)
constexpr int NTYPES = 8;        // GaussianLayer edge_types (clof.py:196)
constexpr int WG_CH_MAX = 64;    // row chunks of a weight-gradient reduction
constexpr int PACK_MAX = 16;     // jobs of one k_clof_pack launch

using gnn::dsilu;
using gnn::sig;
using gnn::silu;
using gnn::WgJob;
using gnn::WgJobs;
// torch.clamp(t, -100, 100): NaN passes through (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp100(float t) { return t < -100.0f ? -100.0f : (t > 100.0f ? 100.0f : t); }
__device__ __forceinline__ bool in100(float t) { return t >= -100.0f && t <= 100.0f; }   // clamp's gradient mask

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// ------------------------------------------------------------------ weight images
// dst[a][b] (row stride B) = trans ? src[b * lds + c0 + a] : src[a * lds + c0 + b]
struct PackJob { const float* src; float* dst; int lds, c0, A, B, trans; };
struct PackJobs { PackJob j[PACK_MAX]; int n; };

__global__ __launch_bounds__(256) void k_clof_pack(PackJobs T) {
    const int q = blockIdx.y;
    if (q >= T.n) return;
    const PackJob& J = T.j[q];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)J.A * J.B) return;
    const int a = (int)(i / J.B), b = (int)(i % J.B);
    J.dst[i] = J.trans ? J.src[(int64_t)b * J.lds + J.c0 + a] : J.src[(int64_t)a * J.lds + J.c0 + b];
}

// per-layer weights: packed images (16-byte aligned) and the torch tensors
struct LayerW {
    // images: [out][in] for the transposed edge products, [in][out] ("t") for their backward and the node products
    const float *w0ef, *w0eft, *w2, *w2t, *w4, *w4t, *wc0, *wc0t, *w0rt, *w0ct, *wv0t, *wn0t, *wn2t, *wrad;
    const float *e_w0, *e_b0, *e_b2, *e_b4, *n_w0, *n_b0, *n_w2, *n_b2, *c_b0, *c_w2, *v_w0, *v_b0, *v_w2, *v_b2;
    const float *ln_w, *ln_b;
};

// ------------------------------------------------------------------ block helpers
template <int H>
__device__ __forceinline__ float wg_sum(float v, float* red) {        // sum over the H threads, fixed order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (H == 64) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1];
}

// ------------------------------------------------------------------ MFMA edge products
// out[g][mo] += W[16 mo + n][...] * in[g][kb] for NOB output blocks and NKB input blocks (layout: top of file)
template <int NOB, int NKB>
__device__ __forceinline__ void mm(const float* __restrict__ W, int ldw, const f32x4 (&in)[CG][NKB], f32x4 (&out)[CG][NOB],
                                   int lane) {
    const float* wl = W + (int64_t)(lane & 15) * ldw + 4 * (lane >> 4);
#pragma unroll
    for (int mo = 0; mo < NOB; ++mo) {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(wl + (int64_t)16 * mo * ldw + 16 * kb);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int g = 0; g < CG; ++g) out[g][mo] = mfma16(w[i], in[g][kb][i], out[g][mo]);
        }
    }
}

template <int NB_>
__device__ __forceinline__ void ld_rows(const float* __restrict__ src, int ld, const int64_t (&p)[CG], const bool (&ok)[CG],
                                        int lane, f32x4 (&v)[CG][NB_]) {
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NB_; ++b)
            v[g][b] = ok[g] ? *reinterpret_cast<const f32x4*>(src + p[g] * ld + 16 * b + 4 * (lane >> 4)) : f32x4{0, 0, 0, 0};
}

template <int NB_>
__device__ __forceinline__ void st_rows(float* __restrict__ dst, int ld, const int64_t (&p)[CG], const bool (&ok)[CG],
                                        int lane, const f32x4 (&v)[CG][NB_]) {
#pragma unroll
    for (int g = 0; g < CG; ++g)
        if (ok[g])
#pragma unroll
            for (int b = 0; b < NB_; ++b) *reinterpret_cast<f32x4*>(dst + p[g] * ld + 16 * b + 4 * (lane >> 4)) = v[g][b];
}

template <int NB_>
__device__ __forceinline__ void silu_all(const f32x4 (&a)[CG][NB_], f32x4 (&z)[CG][NB_]) {
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NB_; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) z[g][b][i] = silu(a[g][b][i]);
}

// bias (scalar loads: torch tensors carry no alignment promise) into every group's accumulator
template <int NB_>
__device__ __forceinline__ void bias_init(const float* __restrict__ b, int lane, f32x4 (&acc)[CG][NB_]) {
#pragma unroll
    for (int bb = 0; bb < NB_; ++bb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = b[16 * bb + 4 * (lane >> 4) + i];
#pragma unroll
            for (int g = 0; g < CG; ++g) acc[g][bb][i] = v;
        }
}

// sum over the four lanes of an edge (l, l ^ 16, l ^ 32, l ^ 48): every one of them gets the same bits
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// the local frame of Clof_GCL.coord2localframe (gcl.py:25-37): radial, diff, cross, vertical
template <bool NORM>
__device__ __forceinline__ void frame(const float* xr, const float* xc, float& rad, float* d, float* cr, float* v) {
    float dr[3], crr[3];
    for (int k = 0; k < 3; ++k) dr[k] = xr[k] - xc[k];
    rad = dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2];
    cross3(xr, xc, crr);
    if (NORM) {
        const float nd = sqrtf(rad) + 1.0f;
        const float nc = sqrtf(crr[0] * crr[0] + crr[1] * crr[1] + crr[2] * crr[2]) + 1.0f;
        for (int k = 0; k < 3; ++k) { d[k] = dr[k] / nd; cr[k] = crr[k] / nc; }
    } else {
        for (int k = 0; k < 3; ++k) { d[k] = dr[k]; cr[k] = crr[k]; }
    }
    cross3(d, cr, v);
}

// ------------------------------------------------------------------ forward
// per node: centroid of its graph (n_per contiguous rows, clof.py:77-79), centred x, embedding_node, and the node
// products of layer 0 (P = [h W0r^T | h W0c^T])
template <int H>
__device__ __forceinline__ void node_proj(const LayerW& W, const float (*hs)[H], int64_t r0, int64_t Nn, float* __restrict__ P) {
    const int j = threadIdx.x;
    float pr[NB] = {}, pc[NB] = {};
    for (int k = 0; k < H; ++k) {
        const float wr = W.w0rt[k * H + j], wc = W.w0ct[k * H + j];
#pragma unroll
        for (int n = 0; n < NB; ++n) { pr[n] += wr * hs[n][k]; pc[n] += wc * hs[n][k]; }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (r0 + n < Nn) { P[(r0 + n) * 2 * H + j] = pr[n]; P[(r0 + n) * 2 * H + H + j] = pc[n]; }
}

template <int H>
__global__ __launch_bounds__(H) void k_clof_prep(LayerW W0, const float* __restrict__ emb_w, const float* __restrict__ emb_b,
                                                 int in_nf, int n_per, int64_t Nn, const float* __restrict__ hin,
                                                 const float* __restrict__ x, float* __restrict__ xc, float* __restrict__ cen,
                                                 float* __restrict__ h0, float* __restrict__ P) {
    __shared__ float hs[NB][H];
    const int64_t r0 = (int64_t)blockIdx.x * NB;
    const int j = threadIdx.x;
    for (int n = 0; n < NB; ++n) {
        const int64_t r = r0 + n;
        float hv = 0.0f;
        if (r < Nn) {
            hv = emb_b[j];
            for (int k = 0; k < in_nf; ++k) hv += emb_w[(int64_t)j * in_nf + k] * hin[r * in_nf + k];
            h0[r * H + j] = hv;
            if (j < 3) {
                const int64_t g0 = (r / n_per) * n_per;
                float s = 0.0f;
                for (int q = 0; q < n_per; ++q) s += x[(g0 + q) * 3 + j];
                const float c = s / (float)n_per;
                cen[r * 3 + j] = c;
                xc[r * 3 + j] = x[r * 3 + j] - c;
            }
        }
        hs[n][j] = hv;
    }
    __syncthreads();
    node_proj<H>(W0, hs, r0, Nn, P);
}

// the prologue, one thread per edge (sorted position p): scalarization (clof.py:66-83 / 158-185), fuse_edge
// (Linear SiLU Linear SiLU) and, for ClofNet_vel_gbf, the Gaussian embedding of (edge type, distance) (layers.py).
// VARIANT 0 ClofNet, 1 ClofNet_vel, 2 ClofNet_vel_gbf.
struct ProW { const float *f_w0, *f_b0, *f_w2, *f_b2, *g_means, *g_stds, *g_mul, *g_bias; };

__device__ __forceinline__ int gbf_type(float ea0) {     // (edge_attr[:, 0] * 0.5 + 0.5).long(), clamped to [0, 7]
    const float t = ea0 * 0.5f + 0.5f;
    if (!(t >= 0.0f)) return 0;                           // negatives and NaN (the reference raises on an index < 0)
    return t >= (float)NTYPES ? NTYPES - 1 : (int)t;
}

template <int VARIANT, bool NORM>
__device__ __forceinline__ int scalarize(const float* xr, const float* xc, const float* vr, const float* vc, const float* ea,
                                         float* in) {
    float rad, d[3], cr[3], v[3];
    frame<NORM>(xr, xc, rad, d, cr, v);
    const float* basis[3] = {d, cr, v};
    float ci[3], cj[3], vi[3], vj[3];
    for (int b = 0; b < 3; ++b) {
        ci[b] = basis[b][0] * xr[0] + basis[b][1] * xr[1] + basis[b][2] * xr[2];
        cj[b] = basis[b][0] * xc[0] + basis[b][1] * xc[1] + basis[b][2] * xc[2];
        vi[b] = basis[b][0] * vr[0] + basis[b][1] * vr[1] + basis[b][2] * vr[2];
        vj[b] = basis[b][0] * vc[0] + basis[b][1] * vc[1] + basis[b][2] * vc[2];
    }
    const float ni = sqrtf(ci[0] * ci[0] + ci[1] * ci[1] + ci[2] * ci[2]);
    const float nj = sqrtf(cj[0] * cj[0] + cj[1] * cj[1] + cj[2] * cj[2]);
    const float cs = (ci[0] * cj[0] + ci[1] * cj[1] + ci[2] * cj[2]) / (ni + 1e-5f) / (nj + 1e-5f);
    const float sn = sqrtf(1.0f - cs * cs);              // no clamp: NaN where |cos| rounds above 1, as the reference
    int f = 0;
    if (VARIANT != 2) { in[f++] = ea[0]; in[f++] = ea[1]; }
    in[f++] = sn; in[f++] = cs;
    for (int b = 0; b < 3; ++b) in[f++] = ci[b];
    for (int b = 0; b < 3; ++b) in[f++] = cj[b];
    if (VARIANT != 0) {
        for (int b = 0; b < 3; ++b) in[f++] = vi[b];
        for (int b = 0; b < 3; ++b) in[f++] = vj[b];
    }
    return f;
}

// gaussian(x, mean, std) of layers.py with pi = 3.14159, in fp32 as the reference computes it (x.float())
__device__ __forceinline__ float gauss(float x, float mean, float sd) {
    const float a = 2.5066272f;                           // float((2 * 3.14159) ** 0.5)
    const float z = (x - mean) / sd;
    return expf(-0.5f * (z * z)) / (a * sd);
}

template <int H, int VARIANT, bool NORM, bool KEEP>
__global__ __launch_bounds__(64) void k_clof_prologue(ProW W, int64_t E, const int32_t* __restrict__ perm,
                                                      const int32_t* __restrict__ row_s, const int32_t* __restrict__ col_s,
                                                      const float* __restrict__ xc, const float* __restrict__ vel,
                                                      const float* __restrict__ ea, float* __restrict__ ef,
                                                      float* __restrict__ fin, float* __restrict__ af1, float* __restrict__ af2) {
    constexpr int H2 = H / 2;
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= E) return;
    const int64_t e = perm[p], r = row_s[p], c = col_s[p];
    float xr[3], xcc[3], vr[3], vc[3], eav[2] = {ea[e * 2], ea[e * 2 + 1]};
    for (int k = 0; k < 3; ++k) { xr[k] = xc[r * 3 + k]; xcc[k] = xc[c * 3 + k]; vr[k] = vel[r * 3 + k]; vc[k] = vel[c * 3 + k]; }
    float in[FMAX];
    const int F = scalarize<VARIANT, NORM>(xr, xcc, vr, vc, eav, in);
    if (KEEP)
        for (int k = 0; k < FMAX; ++k) fin[p * FMAX + k] = k < F ? in[k] : 0.0f;
    float z1[H2];
    for (int j = 0; j < H2; ++j) {
        float a = W.f_b0[j];
        for (int k = 0; k < F; ++k) a += W.f_w0[j * F + k] * own_reg(in[k]);   // own_reg: rule R3
        if (KEEP) af1[p * H2 + j] = a;
        z1[j] = silu(a);
    }
    int t = 0;
    float xg = 0.0f;
    if (VARIANT == 2) {
        t = gbf_type(eav[0]);
        xg = W.g_mul[t] * eav[1] + W.g_bias[t];
    }
    for (int j = 0; j < H2; ++j) {
        float a = W.f_b2[j];
        for (int k = 0; k < H2; ++k) a += W.f_w2[j * H2 + k] * own_reg(z1[k]);
        if (KEEP) af2[p * H2 + j] = a;
        float o = silu(a);
        if (VARIANT == 2) o = o + gauss(xg, W.g_means[j], fabsf(W.g_stds[j]) + 1e-5f);
        ef[p * H2 + j] = o;
    }
}

// one layer's edges (gcl.py:54-66, the edge model and the coordinate model): a1 = h_row W0r^T + h_col W0c^T + radial
// w_rad + edge_feat W0ef^T + b0; m = SiLU-MLP(a1) (three layers); coff = coord_mlp(m) (tanh); the translation, clamped.
// Writes m and the translation in sorted order (the node kernel sums them by row); KEEP: the pre-activations and radial.
struct EdgeBufs {
    const float *x, *P, *ef;
    float *m, *trans, *a1, *a2, *a3, *ac1, *rad;
};

template <int H, bool NORM, bool TANH, bool KEEP>
__global__ __launch_bounds__(64 * EW) void k_clof_edge(LayerW W, EdgeBufs B, int64_t E, const int32_t* __restrict__ row_s,
                                                       const int32_t* __restrict__ col_s) {
    constexpr int NH = H / 16, NH2 = H / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t p[CG], r[CG], c[CG];
    bool ok[CG];
    float d[CG][3], cr[CG][3], v[CG][3], rad[CG];
    for (int g = 0; g < CG; ++g) {
        const int64_t pp = (int64_t)blockIdx.x * ET + wave * 16 * CG + g * 16 + (lane & 15);
        ok[g] = pp < E;
        p[g] = ok[g] ? pp : 0;
        r[g] = ok[g] ? row_s[pp] : 0;
        c[g] = ok[g] ? col_s[pp] : 0;
        float xr[3], xc[3];
        for (int k = 0; k < 3; ++k) { xr[k] = B.x[r[g] * 3 + k]; xc[k] = B.x[c[g] * 3 + k]; }
        frame<NORM>(xr, xc, rad[g], d[g], cr[g], v[g]);
    }
    f32x4 acc[CG][NH], z[CG][NH];
    // a1: bias + node products + radial column, then the edge_feat block on the matrix cores
#pragma unroll
    for (int b = 0; b < NH; ++b) {
        const int ch = 16 * b + 4 * (lane >> 4);
        const f32x4 wr = *reinterpret_cast<const f32x4*>(W.wrad + ch);
        f32x4 b0;
#pragma unroll
        for (int i = 0; i < 4; ++i) b0[i] = W.e_b0[ch + i];
#pragma unroll
        for (int g = 0; g < CG; ++g) {
            const f32x4 pr = *reinterpret_cast<const f32x4*>(B.P + r[g] * 2 * H + ch);
            const f32x4 pc = *reinterpret_cast<const f32x4*>(B.P + c[g] * 2 * H + H + ch);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[g][b][i] = b0[i] + pr[i] + pc[i] + rad[g] * wr[i];
        }
    }
    {
        f32x4 efv[CG][NH2];
        ld_rows<NH2>(B.ef, H / 2, p, ok, lane, efv);
        mm<NH, NH2>(W.w0ef, H / 2, efv, acc, lane);
    }
    if (KEEP) st_rows<NH>(B.a1, H, p, ok, lane, acc);
    silu_all<NH>(acc, z);
    bias_init<NH>(W.e_b2, lane, acc);
    mm<NH, NH>(W.w2, H, z, acc, lane);
    if (KEEP) st_rows<NH>(B.a2, H, p, ok, lane, acc);
    silu_all<NH>(acc, z);
    bias_init<NH>(W.e_b4, lane, acc);
    mm<NH, NH>(W.w4, H, z, acc, lane);
    if (KEEP) st_rows<NH>(B.a3, H, p, ok, lane, acc);
    silu_all<NH>(acc, z);
    st_rows<NH>(B.m, H, p, ok, lane, z);
    bias_init<NH>(W.c_b0, lane, acc);
    mm<NH, NH>(W.wc0, H, z, acc, lane);
    if (KEEP) st_rows<NH>(B.ac1, H, p, ok, lane, acc);
    silu_all<NH>(acc, z);
    // coord_mlp.2 (H -> 3, no bias) on the vector ALU: the lane's channels, then the four lanes of the edge
    for (int g = 0; g < CG; ++g) {
        float cf[3];
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int b = 0; b < NH; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) s += W.c_w2[j * H + 16 * b + 4 * (lane >> 4) + i] * z[g][b][i];
            cf[j] = quad_sum(s);
            if (TANH) cf[j] = tanhf(cf[j]);
        }
        if (ok[g] && (lane >> 4) < 3) {
            const int k = lane >> 4;
            B.trans[p[g] * 3 + k] = clamp100(d[g][k] * cf[0] + cr[g][k] * cf[1] + v[g][k] * cf[2]);
        }
        if (KEEP && ok[g] && (lane >> 4) == 3) B.rad[p[g]] = rad[g];
    }
}

// one layer's nodes (gcl.py:62-66 with E_GCL.node_model): x += mean_row(trans) coords_weight + coord_mlp_vel(h) vel;
// unless LAST without KEEP, h = LayerNorm(h + (h + node_mlp([h, sum_row m])))  (recurrent; h + node_mlp(...) otherwise), and the node
// products of the next layer.  LAST writes the output x + centroid and skips node_mlp (its h is never read).
struct NodeBufs {
    const float *h, *x, *vel, *m, *trans, *cen;
    float *h2, *x2, *out, *P, *av, *an1, *agg, *xhat, *rstd;
};

template <int H, bool LAST, bool KEEP>
__global__ __launch_bounds__(H) void k_clof_node(LayerW W, LayerW Wn, NodeBufs B, float cw, int recurrent, int64_t Nn,
                                                 const int32_t* __restrict__ rowptr) {
    __shared__ float hs[NB][H], ag[NB][H], zs[NB][H], red[2];
    __shared__ float psi[NB];
    const int j = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * NB;
    for (int n = 0; n < NB; ++n) {
        const int64_t r = r0 + n;
        float hv = 0.0f, s = 0.0f;
        if (r < Nn) {
            hv = B.h[r * H + j];
            for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) s += B.m[(int64_t)q * H + j];
            if (KEEP) B.agg[r * H + j] = s;
        }
        hs[n][j] = hv;
        ag[n][j] = s;
    }
    __syncthreads();
    // coord_mlp_vel on the layer's input h
    {
        float a[NB];
        for (int n = 0; n < NB; ++n) a[n] = W.v_b0[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.wv0t[k * H + j];
#pragma unroll
            for (int n = 0; n < NB; ++n) a[n] += w * hs[n][k];
        }
        for (int n = 0; n < NB; ++n) {
            if (KEEP && r0 + n < Nn) B.av[(r0 + n) * H + j] = a[n];
            zs[n][j] = silu(a[n]) * W.v_w2[j];
        }
    }
    __syncthreads();
    if (j < NB) {
        float s = 0.0f;
        for (int k = 0; k < H; ++k) s += zs[j][k];
        psi[j] = s + W.v_b2[0];
    }
    __syncthreads();
    if (j < 3)
        for (int n = 0; n < NB; ++n) {
            const int64_t r = r0 + n;
            if (r >= Nn) continue;
            const int q0 = rowptr[r], q1 = rowptr[r + 1];
            float s = 0.0f;
            for (int q = q0; q < q1; ++q) s += B.trans[(int64_t)q * 3 + j];
            const int cnt = q1 - q0 < 1 ? 1 : q1 - q0;
            const float xn = (B.x[r * 3 + j] + (s / (float)cnt) * cw) + psi[n] * B.vel[r * 3 + j];
            if (LAST) B.out[r * 3 + j] = xn + B.cen[r * 3 + j];
            else B.x2[r * 3 + j] = xn;
            if (KEEP && LAST) B.x2[r * 3 + j] = xn;
        }
    if (LAST && !KEEP) return;     // the last layer's h reaches nothing; kept forwards compute it for forward_layers
    // node_mlp on [h, agg]
    {
        float a[NB];
        for (int n = 0; n < NB; ++n) a[n] = W.n_b0[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.wn0t[k * H + j], w2 = W.wn0t[(H + k) * H + j];
#pragma unroll
            for (int n = 0; n < NB; ++n) a[n] += w * hs[n][k] + w2 * ag[n][k];
        }
        __syncthreads();
        for (int n = 0; n < NB; ++n) {
            if (KEEP && r0 + n < Nn) B.an1[(r0 + n) * H + j] = a[n];
            zs[n][j] = silu(a[n]);
        }
    }
    __syncthreads();
    float u[NB];
    {
        float o[NB];
        for (int n = 0; n < NB; ++n) o[n] = W.n_b2[j];
        for (int k = 0; k < H; ++k) {
            const float w = W.wn2t[k * H + j];
#pragma unroll
            for (int n = 0; n < NB; ++n) o[n] += w * zs[n][k];
        }
        for (int n = 0; n < NB; ++n) u[n] = recurrent ? hs[n][j] + (hs[n][j] + o[n]) : hs[n][j] + o[n];
    }
    __syncthreads();
    for (int n = 0; n < NB; ++n) {                          // LayerNorm (eps 1e-5, biased variance)
        const float mu = wg_sum<H>(u[n], red) / (float)H;
        const float dv = u[n] - mu;
        const float var = wg_sum<H>(dv * dv, red) / (float)H;
        const float rs = 1.0f / sqrtf(var + 1e-5f);
        const float xh = dv * rs;
        const float hn = xh * W.ln_w[j] + W.ln_b[j];
        const int64_t r = r0 + n;
        if (r < Nn) {
            B.h2[r * H + j] = hn;
            if (KEEP) { B.xhat[r * H + j] = xh; if (j == 0) B.rstd[r] = rs; }
        }
        hs[n][j] = hn;
    }
    if (LAST) return;
    __syncthreads();
    node_proj<H>(Wn, hs, r0, Nn, B.P);
}

// ------------------------------------------------------------------ backward
// per node, layer l from the top: dL/dx_{l+1} (gx), dL/dh_{l+1} (gh; LAST: zero) ->
//   gtr = gx cw / count (the translation mean), coord_mlp_vel's gradient into h, and unless LAST the LayerNorm and
//   node_mlp backward into h and into agg (gagg); ghp: dL/dh_l without the edge model's share
struct BNodeBufs {
    const float *gx, *gh, *h, *vel, *av, *an1, *xhat, *rstd;
    float *gtr, *gav, *gpsi, *gu, *gn1, *glnw, *gagg, *ghp;
};

template <int H, bool LAST>
__global__ __launch_bounds__(H) void kb_clof_node(LayerW W, BNodeBufs B, float cw, int recurrent, int64_t Nn,
                                                  const int32_t* __restrict__ rowptr) {
    __shared__ float ga[NB][H], gb[NB][H], red[2];
    const int j = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * NB;
    float gh[NB];
    for (int n = 0; n < NB; ++n) {
        const int64_t r = r0 + n;
        float g = 0.0f;
        if (r < Nn) {
            const float gp = B.gx[r * 3] * B.vel[r * 3] + B.gx[r * 3 + 1] * B.vel[r * 3 + 1] + B.gx[r * 3 + 2] * B.vel[r * 3 + 2];
            g = W.v_w2[j] * gp * dsilu(B.av[r * H + j]);
            B.gav[r * H + j] = g;
            if (j == 0) B.gpsi[r] = gp;
            if (j < 3) {
                const int cnt = rowptr[r + 1] - rowptr[r] < 1 ? 1 : rowptr[r + 1] - rowptr[r];
                B.gtr[r * 3 + j] = B.gx[r * 3 + j] * cw / (float)cnt;
            }
        }
        ga[n][j] = g;
        gh[n] = 0.0f;
    }
    __syncthreads();
    for (int k = 0; k < H; ++k) {                          // + Wv0^T g_av (thread j = input channel)
        const float w = W.v_w0[k * H + j];
        for (int n = 0; n < NB; ++n) gh[n] += w * ga[n][k];
    }
    if (LAST) {
        for (int n = 0; n < NB; ++n)
            if (r0 + n < Nn) { B.ghp[(r0 + n) * H + j] = gh[n]; B.gagg[(r0 + n) * H + j] = 0.0f; }
        return;
    }
    __syncthreads();
    for (int n = 0; n < NB; ++n) {                         // LayerNorm backward
        const int64_t r = r0 + n;
        const bool v = r < Nn;
        const float g = v ? B.gh[r * H + j] : 0.0f, xh = v ? B.xhat[r * H + j] : 0.0f, rs = v ? B.rstd[r] : 0.0f;
        const float gx = g * W.ln_w[j];
        const float m1 = wg_sum<H>(gx, red) / (float)H;
        const float m2 = wg_sum<H>(gx * xh, red) / (float)H;
        const float gu = rs * (gx - m1 - xh * m2);
        if (v) { B.glnw[r * H + j] = g * xh; B.gu[r * H + j] = gu; }
        gb[n][j] = gu;
        gh[n] += recurrent ? 2.0f * gu : gu;
    }
    __syncthreads();
    {
        float g[NB] = {};
        for (int k = 0; k < H; ++k) {                       // Wn2^T g_u
            const float w = W.n_w2[k * H + j];
            for (int n = 0; n < NB; ++n) g[n] += w * gb[n][k];
        }
        for (int n = 0; n < NB; ++n) {
            const int64_t r = r0 + n;
            const float gn = r < Nn ? g[n] * dsilu(B.an1[r * H + j]) : 0.0f;
            if (r < Nn) B.gn1[r * H + j] = gn;
            ga[n][j] = gn;
        }
    }
    __syncthreads();
    float gg[NB] = {};
    for (int k = 0; k < H; ++k) {                          // Wn0^T g_n1: [h | agg]
        const float w = W.n_w0[(int64_t)k * 2 * H + j], w2 = W.n_w0[(int64_t)k * 2 * H + H + j];
        for (int n = 0; n < NB; ++n) { gh[n] += w * ga[n][k]; gg[n] += w2 * ga[n][k]; }
    }
    for (int n = 0; n < NB; ++n)
        if (r0 + n < Nn) { B.ghp[(r0 + n) * H + j] = gh[n]; B.gagg[(r0 + n) * H + j] = gg[n]; }
}

// per edge, layer l: the coordinate model and the three-layer edge MLP backward on the matrix cores.  Writes the
// pre-activation gradients (weight-gradient operands), gc (coord_mlp.2's), the edge_feat gradient summed over layers
// (gef; top: the first layer visited, which starts the sum), and unless first (layer 0) the per-edge dL/dx_row, dL/dx_col.
struct BEdgeBufs {
    const float *x, *a1, *a2, *a3, *ac1, *gtr, *gagg;
    float *ga1, *ga2, *ga3, *gac1, *gc, *gef, *gxr, *gxc;
};

template <int H, bool NORM, bool TANH>
__global__ __launch_bounds__(64 * EW) void kb_clof_edge(LayerW W, BEdgeBufs B, int64_t E, const int32_t* __restrict__ row_s,
                                                        const int32_t* __restrict__ col_s, int top, int first) {
    constexpr int NH = H / 16, NH2 = H / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    int64_t p[CG], r[CG], c[CG];
    bool ok[CG];
    for (int g = 0; g < CG; ++g) {
        const int64_t pp = (int64_t)blockIdx.x * ET + wave * 16 * CG + g * 16 + (lane & 15);
        ok[g] = pp < E;
        p[g] = ok[g] ? pp : 0;
        r[g] = ok[g] ? row_s[pp] : 0;
        c[g] = ok[g] ? col_s[pp] : 0;
    }
    f32x4 pre[CG][NH], gacc[CG][NH], gz[CG][NH];
    // coefficients again (same arithmetic as the forward: same bits), then the coordinate model's backward
    ld_rows<NH>(B.ac1, H, p, ok, lane, pre);
    float gfr[CG][3][3];                                   // dL/d(diff, cross, vertical) of each group's edge
    for (int g = 0; g < CG; ++g) {
        float xr[3], xc[3], rad, d[3], cr[3], v[3];
        for (int k = 0; k < 3; ++k) { xr[k] = B.x[r[g] * 3 + k]; xc[k] = B.x[c[g] * 3 + k]; }
        frame<NORM>(xr, xc, rad, d, cr, v);
        float cf[3];
        for (int jj = 0; jj < 3; ++jj) {
            float s = 0.0f;
#pragma unroll
            for (int b = 0; b < NH; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) s += W.c_w2[jj * H + 16 * b + 4 * q + i] * silu(pre[g][b][i]);
            cf[jj] = quad_sum(s);
            if (TANH) cf[jj] = tanhf(cf[jj]);
        }
        float gt[3];
        for (int k = 0; k < 3; ++k) {
            const float raw = d[k] * cf[0] + cr[k] * cf[1] + v[k] * cf[2];
            gt[k] = in100(raw) ? B.gtr[r[g] * 3 + k] : 0.0f;
        }
        float gcf[3];
        const float* basis[3] = {d, cr, v};
        for (int jj = 0; jj < 3; ++jj) {
            gcf[jj] = gt[0] * basis[jj][0] + gt[1] * basis[jj][1] + gt[2] * basis[jj][2];
            for (int k = 0; k < 3; ++k) gfr[g][jj][k] = gt[k] * cf[jj];
            if (TANH) gcf[jj] = gcf[jj] * (1.0f - cf[jj] * cf[jj]);
        }
        if (ok[g] && q < 3) B.gc[p[g] * 3 + q] = gcf[q];
#pragma unroll
        for (int b = 0; b < NH; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ch = 16 * b + 4 * q + i;
                const float gzc = W.c_w2[ch] * gcf[0] + W.c_w2[H + ch] * gcf[1] + W.c_w2[2 * H + ch] * gcf[2];
                gz[g][b][i] = gzc * dsilu(pre[g][b][i]);
            }
    }
    st_rows<NH>(B.gac1, H, p, ok, lane, gz);
    // g_m = Wc0^T g_ac1 + the row's agg gradient
    ld_rows<NH>(B.gagg, H, r, ok, lane, gacc);
    mm<NH, NH>(W.wc0t, H, gz, gacc, lane);
    ld_rows<NH>(B.a3, H, p, ok, lane, pre);
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NH; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) gz[g][b][i] = gacc[g][b][i] * dsilu(pre[g][b][i]);
    st_rows<NH>(B.ga3, H, p, ok, lane, gz);
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NH; ++b) gacc[g][b] = f32x4{0, 0, 0, 0};
    mm<NH, NH>(W.w4t, H, gz, gacc, lane);
    ld_rows<NH>(B.a2, H, p, ok, lane, pre);
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NH; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) gz[g][b][i] = gacc[g][b][i] * dsilu(pre[g][b][i]);
    st_rows<NH>(B.ga2, H, p, ok, lane, gz);
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NH; ++b) gacc[g][b] = f32x4{0, 0, 0, 0};
    mm<NH, NH>(W.w2t, H, gz, gacc, lane);
    ld_rows<NH>(B.a1, H, p, ok, lane, pre);
#pragma unroll
    for (int g = 0; g < CG; ++g)
#pragma unroll
        for (int b = 0; b < NH; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) gz[g][b][i] = gacc[g][b][i] * dsilu(pre[g][b][i]);
    st_rows<NH>(B.ga1, H, p, ok, lane, gz);
    // edge_feat gradient, summed over the layers from the top down
    {
        f32x4 ge[CG][NH2];
        if (top) {
#pragma unroll
            for (int g = 0; g < CG; ++g)
#pragma unroll
                for (int b = 0; b < NH2; ++b) ge[g][b] = f32x4{0, 0, 0, 0};
        } else {
            ld_rows<NH2>(B.gef, H / 2, p, ok, lane, ge);
        }
        mm<NH2, NH>(W.w0eft, H, gz, ge, lane);
        st_rows<NH2>(B.gef, H / 2, p, ok, lane, ge);
    }
    if (first) return;                                     // layer 0's frame is built from the (detached) input
    for (int g = 0; g < CG; ++g) {
        float s = 0.0f;
#pragma unroll
        for (int b = 0; b < NH; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) s += W.wrad[16 * b + 4 * q + i] * gz[g][b][i];
        const float grad_rad = quad_sum(s);
        float xr[3], xc[3], dr[3], crr[3];
        for (int k = 0; k < 3; ++k) { xr[k] = B.x[r[g] * 3 + k]; xc[k] = B.x[c[g] * 3 + k]; dr[k] = xr[k] - xc[k]; }
        cross3(xr, xc, crr);
        float rad, d[3], cr[3], v[3];
        frame<NORM>(xr, xc, rad, d, cr, v);
        float gd[3], gcr[3], t[3];
        cross3(cr, gfr[g][2], t);                          // v = d x cr
        for (int k = 0; k < 3; ++k) gd[k] = gfr[g][0][k] + t[k];
        cross3(gfr[g][2], d, t);
        for (int k = 0; k < 3; ++k) gcr[k] = gfr[g][1][k] + t[k];
        float gdr[3], gcrr[3], grad_tot = grad_rad;
        if (NORM) {                                        // d = dr / (|dr| + 1), cr = crr / (|crr| + 1), torch's order
            const float s1 = sqrtf(rad), nd = s1 + 1.0f;
            const float csq = crr[0] * crr[0] + crr[1] * crr[1] + crr[2] * crr[2];
            const float s2 = sqrtf(csq), nc = s2 + 1.0f;
            float gnd = 0.0f, gnc = 0.0f;
            for (int k = 0; k < 3; ++k) {
                gdr[k] = gd[k] / nd;
                gcrr[k] = gcr[k] / nc;
                gnd += -gd[k] * dr[k] / (nd * nd);
                gnc += -gcr[k] * crr[k] / (nc * nc);
            }
            grad_tot += gnd / (2.0f * s1);                 // SqrtBackward: NaN at 0 / 0, as torch
            const float gcsq = gnc / (2.0f * s2);
            for (int k = 0; k < 3; ++k) gcrr[k] += 2.0f * crr[k] * gcsq;
        } else {
            for (int k = 0; k < 3; ++k) { gdr[k] = gd[k]; gcrr[k] = gcr[k]; }
        }
        for (int k = 0; k < 3; ++k) gdr[k] += 2.0f * dr[k] * grad_tot;
        float ga[3], gb[3];
        cross3(xc, gcrr, ga);                              // crr = xr x xc
        cross3(gcrr, xr, gb);
        if (ok[g] && q < 3) {
            B.gxr[p[g] * 3 + q] = gdr[q] + ga[q];
            B.gxc[p[g] * 3 + q] = -gdr[q] + gb[q];
        }
    }
}

// per node: the row and col sums of g_a1 (the weight-gradient operands of edge_mlp.0's h blocks), dL/dh_l = ghp +
// W0r^T srow + W0c^T scol, and unless first dL/dx_l = gx_{l+1} + the row sums of gxr + the col sums of gxc
struct BGatherBufs {
    const float *ga1, *ghp, *gx, *gxr, *gxc;
    float *srow, *scol, *gh, *gxo;
};

template <int H>
__global__ __launch_bounds__(H) void kb_clof_gather(LayerW W, BGatherBufs B, int kin, int64_t Nn,
                                                    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ sperm,
                                                    const int32_t* __restrict__ srowptr, int first) {
    __shared__ float sr[NB][H], sc[NB][H];
    const int j = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * NB;
    for (int n = 0; n < NB; ++n) {
        const int64_t r = r0 + n;
        float a = 0.0f, b = 0.0f;
        if (r < Nn) {
            for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) a += B.ga1[(int64_t)q * H + j];
            for (int q = srowptr[r]; q < srowptr[r + 1]; ++q) b += B.ga1[(int64_t)sperm[q] * H + j];
            B.srow[r * H + j] = a;
            B.scol[r * H + j] = b;
            if (!first && j < 3) {
                float g = B.gx[r * 3 + j];
                for (int q = rowptr[r]; q < rowptr[r + 1]; ++q) g += B.gxr[(int64_t)q * 3 + j];
                for (int q = srowptr[r]; q < srowptr[r + 1]; ++q) g += B.gxc[(int64_t)sperm[q] * 3 + j];
                B.gxo[r * 3 + j] = g;
            }
        }
        sr[n][j] = a;
        sc[n][j] = b;
    }
    __syncthreads();
    float g[NB];
    for (int n = 0; n < NB; ++n) g[n] = r0 + n < Nn ? B.ghp[(r0 + n) * H + j] : 0.0f;
    for (int k = 0; k < H; ++k) {
        const float wr = W.e_w0[(int64_t)k * kin + j], wc = W.e_w0[(int64_t)k * kin + H + j];
        for (int n = 0; n < NB; ++n) g[n] += wr * sr[n][k] + wc * sc[n][k];
    }
    for (int n = 0; n < NB; ++n)
        if (r0 + n < Nn) B.gh[(r0 + n) * H + j] = g[n];
}

// per edge: edge_feat's gradient through fuse_edge and, for ClofNet_vel_gbf, the Gaussian layer
struct BProBufs {
    const float *gef, *fin, *af1, *af2, *ea;
    float *gaf1, *gaf2, *gmean, *gstd, *gmul, *gbias;
};

template <int H, int VARIANT>
__global__ __launch_bounds__(64) void kb_clof_prologue(ProW W, BProBufs B, int F, int64_t E, const int32_t* __restrict__ perm) {
    constexpr int H2 = H / 2;
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= E) return;
    float g2[H2];
    float gx = 0.0f;
    float xg = 0.0f;
    int t = 0;
    if (VARIANT == 2) {
        const int64_t e = perm[p];
        const float ea0 = B.ea[e * 2], dist = B.ea[e * 2 + 1];
        t = gbf_type(ea0);
        xg = W.g_mul[t] * dist + W.g_bias[t];
    }
    for (int j = 0; j < H2; ++j) {
        const float ge = B.gef[p * H2 + j];
        g2[j] = ge * dsilu(B.af2[p * H2 + j]);
        B.gaf2[p * H2 + j] = g2[j];
        if (VARIANT == 2) {
            const float s = W.g_stds[j], sd = fabsf(s) + 1e-5f, mean = W.g_means[j];
            const float gv = gauss(xg, mean, sd), z = (xg - mean) / sd;
            gx += ge * gv * (-z / sd);
            B.gmean[p * H2 + j] = ge * gv * z / sd;
            const float sg = s > 0.0f ? 1.0f : (s < 0.0f ? -1.0f : 0.0f);
            B.gstd[p * H2 + j] = ge * gv * (z * z - 1.0f) / sd * sg;
        }
    }
    if (VARIANT == 2) {
        const float dist = B.ea[(int64_t)perm[p] * 2 + 1];
        for (int k = 0; k < NTYPES; ++k) {
            B.gmul[p * NTYPES + k] = k == t ? gx * dist : 0.0f;
            B.gbias[p * NTYPES + k] = k == t ? gx : 0.0f;
        }
    }
    for (int k = 0; k < H2; ++k) {
        float s = 0.0f;
        for (int j = 0; j < H2; ++j) s += W.f_w2[j * H2 + k] * own_reg(g2[j]);
        B.gaf1[p * H2 + k] = s * dsilu(B.af1[p * H2 + k]);
    }
    (void)F;
}

// ------------------------------------------------------------------ weight gradients
// First stage of gnn_common.h's weight-gradient reduction:
// one wave per (32 x 32 output tile, row chunk); rows are the MFMA's k
__global__ __launch_bounds__(64) void k_clof_wgrad_part(WgJobs T, float* __restrict__ part) {
    const int t = blockIdx.x, ch = blockIdx.y;
    int q = 0;
    while (q + 1 < T.n && T.j[q + 1].tile0 <= t) ++q;
    const WgJob& J = T.j[q];
    const int tk = (J.K + 31) / 32;
    const int tt = t - J.tile0;
    const int j0 = (tt / tk) * 32, k0 = (tt % tk) * 32;
    const int lane = threadIdx.x, n = lane & 15, kq = lane >> 4;
    const int64_t per = (J.rows + T.n_ch - 1) / T.n_ch;
    const int64_t i0 = ch * per, i1 = i0 + per < J.rows ? i0 + per : J.rows;
    f32x4 acc[2][2] = {};
    for (int64_t i = i0; i < i1; i += 4) {
        const int64_t row = i + kq;
        const bool rv = row < i1;
        float a[2], b[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int jj = j0 + 16 * u + n, kk = k0 + 16 * u + n;
            a[u] = rv && jj < J.J ? J.G[row * J.ldg + jj] : 0.0f;
            float bv = 0.0f;
            if (rv && kk < J.K) {
                bv = J.A ? J.A[row * J.lda + kk] : 1.0f;
                if (J.act == 1) bv = silu(bv);
            }
            b[u] = bv;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int w = 0; w < 2; ++w) acc[u][w] = mfma16(a[u], b[w], acc[u][w]);
    }
    float* P = part + (int64_t)ch * T.n_out + J.poff;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int jj = j0 + 16 * u + 4 * kq + i, kk = k0 + 16 * w + n;
                if (jj < J.J && kk < J.K) P[(int64_t)jj * J.K + kk] = acc[u][w][i];
            }
}

}  // namespace clof
