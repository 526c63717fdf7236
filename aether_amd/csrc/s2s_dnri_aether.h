// The seq2seq ablation DNRIAether (nn/seq2seq/ablations/dnri_aether.py): dNRI whose encoder and decoders also read the field
// the model discovers -- no local frames.  Every layer that reads the raw 2D-wide state in dNRI reads ext = [inputs | field]
// here, 3D <= 9 columns: more than the narrow kernels of s2s_dnri.h / s2s_step.h hold (xin[6], x[8]).  The kernels below stand
// in their place where the width asks for it; everything else is the dNRI engine (s2s_dnri.h, host_nri_chain.inc) and the
// field query of the seq2seq Aether (k_s2s_rff, two job-table layers).  None of them takes a struct by value or reads a hidden
// kernel argument.
#pragma once
#include "s2s_dnri.h"

namespace {

constexpr int S2S_DNRIA_C = 9;          // widest ext row: 3D at D = 3

// Node side of a step (in the place of k_s2s_dnri_node_prep; the field half as k_s2s_node_prep): a wave per node.
//   * fh2 != nullptr: the last field layer, field[n] = W4 fh2[n] + b4 (dnri_aether.py:81-85; D rows of he weights, 64 lanes x
//     he / 64 products each, butterfly sum); else the field is field_in [n][D] and the wave only concatenates;
//   * ext[n] = [inputs[n] | field[n]] (3D columns; :416, :446, :564, :633), the field to field_out when that is not null, and
//     the per-type edge counters of the step cleared;
//   * for the MLP decoder (wide != nullptr): ext zero-padded to the S2S_RFG columns in front of the aggregated messages in
//     the row out_fc1 reads (:669), and the node halves of msg_fc1[k] on [ext_recv | ext_send] (:635-650) for every used type:
//     A_k[n][:] = b_k + W_k[:, :3D] ext[n], S_k[n][:] = W_k[:, 3D:] ext[n], W_k [h][6D], A / S [K][n_nodes][h] (lane l: units
//     l, l + 64, ..).
template <int D>
__global__ void __launch_bounds__(256)
k_s2s_dnria_node_prep(const float* __restrict__ inputs, const float* __restrict__ field_in, const float* __restrict__ fh2,
                      const float* __restrict__ w4, const float* __restrict__ b4, int he, float* __restrict__ field_out,
                      float* __restrict__ ext, float* __restrict__ wide, int ldwide, int* __restrict__ counts, int64_t n_nodes,
                      const float* W0, const float* W1, const float* W2, const float* W3, const float* b0, const float* b1,
                      const float* b2, const float* b3, int K, int k0, float* __restrict__ A, float* __restrict__ S, int h) {
    constexpr int C = 3 * D;
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x < 8) counts[threadIdx.x] = 0;
    if (n >= n_nodes) return;
    float xi[C];
#pragma unroll
    for (int t = 0; t < 2 * D; ++t) xi[t] = inputs[n * 2 * D + t];
    if (fh2 != nullptr) {
        float part[D];
#pragma unroll
        for (int dd = 0; dd < D; ++dd) part[dd] = 0.0f;
        for (int k = 4 * lane; k < he; k += 256) {
            const f32x4 xv = ld4(fh2 + (size_t)n * he + k);
#pragma unroll
            for (int dd = 0; dd < D; ++dd) {
                const f32x4 wv = ld4(w4 + (size_t)dd * he + k);
                part[dd] += wv[0] * xv[0] + wv[1] * xv[1] + wv[2] * xv[2] + wv[3] * xv[3];
            }
        }
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) part[dd] += __shfl_xor(part[dd], off);
            xi[2 * D + dd] = part[dd] + b4[dd];
        }
    } else {
#pragma unroll
        for (int t = 0; t < D; ++t) xi[2 * D + t] = field_in[n * D + t];
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < C; ++t) ext[n * C + t] = xi[t];
        if (field_out != nullptr) {
#pragma unroll
            for (int t = 0; t < D; ++t) field_out[n * D + t] = xi[2 * D + t];
        }
    }
    if (wide == nullptr) return;
    if (lane < S2S_RFG) {
        float v = 0.0f;
#pragma unroll
        for (int t = 0; t < C; ++t) v = lane == t ? xi[t] : v;
        wide[n * ldwide + lane] = v;
    }
    for (int k = k0; k < K; ++k) {
        const float* Wk = k == 0 ? W0 : k == 1 ? W1 : k == 2 ? W2 : W3;
        const float* bk = k == 0 ? b0 : k == 1 ? b1 : k == 2 ? b2 : b3;
        for (int m = lane; m < h; m += 64) {
            const float* wrow = Wk + (size_t)m * 2 * C;
            float sa = bk[m], ss = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) { sa = fmaf(wrow[c], xi[c], sa); ss = fmaf(wrow[C + c], xi[c], ss); }
            A[((size_t)k * n_nodes + n) * h + m] = sa;
            S[((size_t)k * n_nodes + n) * h + m] = ss;
        }
    }
}

// mlp1's first Linear and its ELU on the ext rows (dnri_aether.py:320, :416): Y[n][m] = ELU(b[m] + sum_{c < C} W[m][c] X[n][c]),
// W [M][C], C <= 9 -- k_s2s_narrow_layers holds 8 columns.  One thread per (row, 4 outputs).
__global__ void __launch_bounds__(256)
k_s2s_dnria_narrow_elu(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ X, int C,
                       float* __restrict__ Y, int M, int64_t n_rows) {
    const int q4 = M >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_rows * q4) return;
    const int64_t n = idx / q4;
    const int m = (int)(idx - n * q4) * 4;
    float x[S2S_DNRIA_C];
#pragma unroll
    for (int c = 0; c < S2S_DNRIA_C; ++c) x[c] = c < C ? X[n * C + c] : 0.0f;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float sv = b[m + r];
#pragma unroll
        for (int c = 0; c < S2S_DNRIA_C; ++c)
            if (c < C) sv = fmaf(W[(size_t)(m + r) * C + c], x[c], sv);
        v[r] = elu1(sv);
    }
    st4(Y + (size_t)n * M + m, v);
}

// The GRU-style gate of the recurrent decoder (dnri_aether.py:564-578) as k_s2s_dnri_gate, whose input_r / _i / _n act on the
// C = 3D <= 9 columns of ext [n][C] instead of the raw inputs.  A thread per (node, 4 units).
__global__ void __launch_bounds__(256)
k_s2s_dnria_gate(const float* __restrict__ x, int C, const float* __restrict__ wr, const float* __restrict__ br,
                 const float* __restrict__ wi, const float* __restrict__ bi, const float* __restrict__ wn,
                 const float* __restrict__ bn, const float* __restrict__ hr, const float* __restrict__ hi,
                 const float* __restrict__ hh, const float* __restrict__ hidden, float* __restrict__ hidden_out, int h,
                 int64_t n_nodes) {
    const int q4 = h >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_nodes * q4) return;
    const int64_t n = idx / q4;
    const int m = (int)(idx - n * q4) * 4;
    float xin[S2S_DNRIA_C];
#pragma unroll
    for (int t = 0; t < S2S_DNRIA_C; ++t) xin[t] = t < C ? x[n * C + t] : 0.0f;
    const size_t o = (size_t)n * h + m;
    const f32x4 vr = ld4(hr + o), vi = ld4(hi + o), vh = ld4(hh + o), hv = ld4(hidden + o);
    f32x4 res;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float ir = br[m + j], ii = bi[m + j], in_ = bn[m + j];
#pragma unroll
        for (int t = 0; t < S2S_DNRIA_C; ++t)
            if (t < C) {
                ir = fmaf(wr[(size_t)(m + j) * C + t], xin[t], ir);
                ii = fmaf(wi[(size_t)(m + j) * C + t], xin[t], ii);
                in_ = fmaf(wn[(size_t)(m + j) * C + t], xin[t], in_);
            }
        const float r = sigmoid1(ir + vr[j]);
        const float i = sigmoid1(ii + vi[j]);
        const float nn = tanh1(in_ + r * vh[j]);
        res[j] = (1.0f - i) * nn + i * hv[j];
    }
    st4(hidden_out + o, res);
}

}  // namespace
