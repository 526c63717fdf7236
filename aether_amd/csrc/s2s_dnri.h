// The seq2seq dNRI baseline (nn/seq2seq/dnri.py): the job-table engine of s2s_step.h around a model without local frames --
// no localizer, no edge attributes, no hyper-network filter, no rotate-back.  The encoder's prior step (dnri.py:403-424) is the
// NRI stack mlp1 (nodes) -> node2edge -> mlp2 -> edge2node -> mlp3 -> node2edge | skip -> mlp4, one LSTM step per edge and
// prior_fc_out; both decoders read the raw inputs:
//   DNRI_Decoder      dnri.py:479-534   pre_msg = [h_recv | h_send], tanh, / norm, sum / (N - 1), GRU gate whose input_r / _i / _n
//                                       act on the raw inputs (2D columns), pred = inputs + out
//   DNRI_MLP_Decoder  dnri.py:574-624   pre_msg = [x_recv | x_send] (4D columns), ReLU, plain sum, out_fc1 on [inputs | agg]
// The dense layers, the LSTM cell, the Gumbel sample and the per-type lists are s2s_step.h's; the kernels here are what stands
// in the place of the frame kernels (k_s2s_locs_node_prep / _edge_prep / k_s2s_out_globalize) and of the gate and the message
// front that read frame features there.  None of them takes a struct by value or reads a hidden kernel argument.
#pragma once
#include "s2s_step.h"

namespace {

// Node side of a step: clears the per-type edge counters (k_s2s_gumbel_select adds to them) and, for the MLP decoder (wide !=
// nullptr), does what that decoder needs of the raw state x [n][C], C = 2D <= 6:
//   * stages it, zero-padded to the S2S_RFG columns in front of the aggregated messages, in the row out_fc1 reads (row stride
//     ldwide: a whole 32-wide k block for the split GEMM);
//   * the first message layer on the raw input pair (DNRI_MLP_Decoder :582-605): msg_fc1[k] on [x_recv | x_send] is the sum of
//     its two halves' products of the node rows, A_k[n][:] = b_k + W_k[:, :C] x[n], S_k[n][:] = W_k[:, C:] x[n] for every used
//     type k (W_k [h][2C] = Wk; the types' tensors are separate allocations, handed over as plain pointers), A / S
//     [K][n_nodes][h] -- per node, not per edge: an edge then costs two row reads (k_s2s_dnri_pair).
// `per` = max(S2S_RFG, h / 4) threads per node: thread t stages column t and computes units 4t .. 4t + 3.
__global__ void __launch_bounds__(256)
k_s2s_dnri_node_prep(const float* __restrict__ inputs, int C, float* __restrict__ wide, int ldwide, int* __restrict__ counts,
                     int64_t n_nodes, const float* W0, const float* W1, const float* W2, const float* W3, const float* b0,
                     const float* b1, const float* b2, const float* b3, int K, int k0, float* __restrict__ A,
                     float* __restrict__ S, int h, int per) {
    if (blockIdx.x == 0 && threadIdx.x < 8) counts[threadIdx.x] = 0;
    if (wide == nullptr) return;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_nodes * per) return;
    const int64_t n = idx / per;
    const int t = (int)(idx - n * per);
    if (t < S2S_RFG) wide[n * ldwide + t] = t < C ? inputs[n * C + t] : 0.0f;
    const int m = 4 * t;
    if (m >= h) return;
    float xin[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) xin[c] = c < C ? inputs[n * C + c] : 0.0f;
    for (int k = k0; k < K; ++k) {
        const float* Wk = k == 0 ? W0 : k == 1 ? W1 : k == 2 ? W2 : W3;
        const float* bk = k == 0 ? b0 : k == 1 ? b1 : k == 2 ? b2 : b3;
        f32x4 va, vs;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* wrow = Wk + (size_t)(m + j) * 2 * C;
            float sa = bk[m + j], ss = 0.0f;
#pragma unroll
            for (int c = 0; c < 6; ++c)
                if (c < C) { sa = fmaf(wrow[c], xin[c], sa); ss = fmaf(wrow[C + c], xin[c], ss); }
            va[j] = sa; vs[j] = ss;
        }
        st4(A + ((size_t)k * n_nodes + n) * h + m, va);
        st4(S + ((size_t)k * n_nodes + n) * h + m, vs);
    }
}

// node2edge + the first Linear of mlp2 + ELU (dnri.py:334-342, :406-407): the Linear on [x_send | x_recv] is the sum of its
// two halves' products of the node rows, T[e][:] = ELU(Ps[send[e]][:] + Pr[recv[e]][:]) (the bias is in Ps).
__global__ void __launch_bounds__(256)
k_s2s_dnri_pair_elu(const float* __restrict__ Ps, const float* __restrict__ Pr, const int64_t* __restrict__ send,
                    const int64_t* __restrict__ recv, float* __restrict__ T, int h, int64_t n_edges) {
    const int q4 = h >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_edges * q4) return;
    const int64_t e = idx / q4;
    const int c = (int)(idx - e * q4) * 4;
    f32x4 v = ld4(Ps + (size_t)send[e] * h + c) + ld4(Pr + (size_t)recv[e] * h + c);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = elu1(v[r]);
    st4(T + (size_t)e * h + c, v);
}

// First message layer of every edge type k >= k0 whose weight on edge e is not zero, from the layer's node products:
// T[k][e][:] = act(A_k[recv[e]][:] + S_k[send[e]][:]), A / S [K][n_nodes][h] the receiver / sender halves (bias in A), rows by
// edge id (the second layer gathers them through the type's list); M[e][:] = 0 for the edges no type will write (hard
// samples: an edge sits in at most one list, whose second-layer job writes its row of M without reading it).
//   RELU = false (DNRI_Decoder :489-508):      pre_msg = [h_recv | h_send] of the hidden state, tanh
//   RELU = true  (DNRI_MLP_Decoder :582-605):  pre_msg = [x_recv | x_send] of the raw inputs (k_s2s_dnri_node_prep), ReLU
template <bool RELU>
__global__ void __launch_bounds__(256)
k_s2s_dnri_pair(const float* __restrict__ A, const float* __restrict__ S, int64_t n_nodes, const int64_t* __restrict__ send,
                const int64_t* __restrict__ recv, const float* __restrict__ edge_w, int K, int k0, float* __restrict__ T,
                float* __restrict__ M, int h, int64_t n_edges) {
    const int q4 = h >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_edges * q4) return;
    const int64_t e = idx / q4;
    const int c = (int)(idx - e * q4) * 4;
    const int64_t r = recv[e], s = send[e];
    bool written = false;
    for (int k = k0; k < K; ++k) {
        if (edge_w[e * K + k] == 0.0f) continue;
        written = true;
        f32x4 v = ld4(A + ((size_t)k * n_nodes + r) * h + c) + ld4(S + ((size_t)k * n_nodes + s) * h + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = RELU ? fmaxf(v[j], 0.0f) : tanh1(v[j]);
        st4(T + ((size_t)k * n_edges + e) * h + c, v);
    }
    if (!written) st4(M + (size_t)e * h + c, f32x4{0.f, 0.f, 0.f, 0.f});
}

// Messages to their receivers: out[n][:] = (sum over the node's in-edges of M[e][:] / msg_div) / agg_div, in edge order.
// Both divisors are the caller's: DNRI_Decoder divides every message by the number of used edge types (:512) and the sum by
// N - 1 (:516); DNRI_MLP_Decoder takes the plain sum (:609-613), msg_div = agg_div = 1.  ldo: row stride of out.
__global__ void __launch_bounds__(128)
k_s2s_dnri_aggregate(const float* __restrict__ M, const int64_t* __restrict__ order, const int64_t* __restrict__ rowptr,
                     float* __restrict__ out, int ldo, int h, float msg_div, float agg_div) {
    const int64_t n = blockIdx.x;
    const int64_t beg = rowptr[n], end = rowptr[n + 1];
    for (int c = threadIdx.x * 4; c < h; c += 128 * 4) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t k = beg; k < end; ++k) s += ld4(M + (size_t)order[k] * h + c) / msg_div;
        st4(out + (size_t)n * ldo + c, s / agg_div);
    }
}

// GRU-style gate of DNRI_Decoder (:519-525).  input_r / _i / _n act on the raw inputs x [n][C] (C = 2D <= 6: three narrow
// layers, computed here); hr / hi / hh [n][h] are hidden_r / _i / _h of the aggregated messages (no bias).  There are no
// present-message terms:  r = sig(inp_r + hr), i = sig(inp_i + hi), n = tanh(inp_n + r hh), hidden' = (1 - i) n + i hidden.
// A thread per (node, 4 units).
__global__ void __launch_bounds__(256)
k_s2s_dnri_gate(const float* __restrict__ x, int C, const float* __restrict__ wr, const float* __restrict__ br,
                const float* __restrict__ wi, const float* __restrict__ bi, const float* __restrict__ wn,
                const float* __restrict__ bn, const float* __restrict__ hr, const float* __restrict__ hi,
                const float* __restrict__ hh, const float* __restrict__ hidden, float* __restrict__ hidden_out, int h,
                int64_t n_nodes) {
    const int q4 = h >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_nodes * q4) return;
    const int64_t n = idx / q4;
    const int m = (int)(idx - n * q4) * 4;
    float xin[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) xin[t] = t < C ? x[n * C + t] : 0.0f;
    const size_t o = (size_t)n * h + m;
    const f32x4 vr = ld4(hr + o), vi = ld4(hi + o), vh = ld4(hh + o), hv = ld4(hidden + o);
    f32x4 res;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float ir = br[m + j], ii = bi[m + j], in_ = bn[m + j];
#pragma unroll
        for (int t = 0; t < 6; ++t)
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

// Last layer of either decoder's output MLP and the residual (:530-532, :621-624): out[n] = inputs[n] + W3 o2[n] + b3, W3
// [2D][hd].  No frame: the prediction is added as it is.  A wave per node, butterfly sums (as k_s2s_out_globalize).
template <int D>
__global__ void __launch_bounds__(256)
k_s2s_dnri_out(const float* __restrict__ o2, const float* __restrict__ w3, const float* __restrict__ b3, int hd,
               const float* __restrict__ inputs, float* __restrict__ out, int64_t n_nodes) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_nodes) return;
    float pred[2 * D];
#pragma unroll
    for (int t = 0; t < 2 * D; ++t) pred[t] = 0.0f;
    for (int k = 4 * lane; k < hd; k += 256) {
        const f32x4 xv = ld4(o2 + (size_t)n * hd + k);
#pragma unroll
        for (int t = 0; t < 2 * D; ++t) {
            const f32x4 wv = ld4(w3 + (size_t)t * hd + k);
            pred[t] += wv[0] * xv[0] + wv[1] * xv[1] + wv[2] * xv[2] + wv[3] * xv[3];
        }
    }
#pragma unroll
    for (int t = 0; t < 2 * D; ++t) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) pred[t] += __shfl_xor(pred[t], off);
    }
    if (lane != 0) return;
#pragma unroll
    for (int t = 0; t < 2 * D; ++t) out[n * 2 * D + t] = inputs[n * 2 * D + t] + (pred[t] + b3[t]);
}

// Plan helper: dst[r][0 .. pad + rest) = [src[r][0 .. c0) zero-padded to pad | src[r][c0 .. c0 + rest)], src row stride
// c0 + rest (out_fc1 of the MLP decoder, whose input is [inputs | agg]: the row the step stages is [inputs, 0 .. | agg]).
__global__ void __launch_bounds__(256)
k_s2s_dnri_pad_front(const float* __restrict__ src, int c0, int pad, int rest, float* __restrict__ dst, int64_t rows) {
    const int ld = pad + rest;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * ld) return;
    const int64_t r = idx / ld;
    const int c = (int)(idx - r * ld);
    float v = 0.0f;
    if (c < pad) v = c < c0 ? src[r * (c0 + rest) + c] : 0.0f;
    else v = src[r * (c0 + rest) + c0 + (c - pad)];
    dst[idx] = v;
}

}  // namespace
