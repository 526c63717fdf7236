// The charge-aware seq2seq Aether (nn/seq2seq/ablations/aether_charges.py): the fused step of s2s_step.h for a model whose
// field query, encoder and decoder layers also see a 16-wide embedding emb[c] of every particle's charge sign, c in {0, 1}
// (aether_charges.py:86, :100-102).  The embedding has two rows, so whatever it feeds is a TABLE, not a GEMM operand:
//   * a Linear over [features | emb[c]] is W_f . features + (b + W_c . emb[c]): one of 2 bias rows per node; over
//     [features | emb[c_recv] | emb[c_send]] one of 4 rows per edge (row 2 c_recv + c_send).  The dense kernels add the row
//     in their epilogue (S2SJob::btab / bidx); where a gate sums several biases the rows carry the sum.
//   * the anisotropic filter, out_o = sum_f a_f (W2[f out + o, :] . g + b2[f out + o]), has a_f = emb[c_recv][j] for its 16
//     receiver-charge features: their contribution is (sum_j emb[c][j] W2_block_j) . g + sum_j emb[c][j] b2_block_j, ONE
//     [out][h] block per charge value, selected by an indicator feature of value 1.  The 32 embedding features become four
//     one-hot features [recv 0, recv 1, send 0, send 1]; the filter GEMM runs on EA + 4 = 28 / 43 features instead of 56 / 71.
// The algebra is exact; only the association of the fp32 sums changes.  Everything here runs once per weight version (the
// plan) or once per entry call (the index arrays); a step launches what the plain model's step launches.
#pragma once
#include "s2s_step.h"

namespace {

constexpr int S2S_CE = 16;             // charge_embedding_dim (aether_charges.py:72, :333, :477, :583)
constexpr int S2S_ERR_CHARGE = 3;      // async error word: a charge index outside {0, 1}

// out[row][m] = b1[m] (+ b2[m]) + sum_j W[m][col0 + j] emb[c][j] (+ sum_j W[m][col0 + 16 + j] emb[c'][j]).
// pair = 0: rows c = 0, 1 and a third row of NaN (where an index outside {0, 1} is sent); pair = 1: rows 2 c + c'.
__global__ void __launch_bounds__(256)
k_s2s_charge_table(const float* __restrict__ W, int ldw, int col0, const float* __restrict__ b1, const float* __restrict__ b2,
                   const float* __restrict__ emb, int pair, int M, float* __restrict__ out) {
    const int rows = pair ? 4 : 3;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * M) return;
    const int row = idx / M, m = idx - row * M;
    if (!pair && row == 2) { out[idx] = __int_as_float(0x7fc00000); return; }
    const int c = pair ? row >> 1 : row, c2 = row & 1;
    float s = b1[m] + (b2 != nullptr ? b2[m] : 0.0f);
    const float* w = W + (size_t)m * ldw + col0;
    for (int j = 0; j < S2S_CE; ++j) s = fmaf(w[j], emb[c * S2S_CE + j], s);
    if (pair)
        for (int j = 0; j < S2S_CE; ++j) s = fmaf(w[S2S_CE + j], emb[c2 * S2S_CE + j], s);
    out[idx] = s;
}

// The filter bank [(EA + 32) h][h] (+ bias [(EA + 32) h]) of the charge-aware encoder -> [(EA + 4) h][h] (+ [(EA + 4) h]):
// feature blocks 0 .. EA - 1 as they are, block EA + 2 s + c = sum_j emb[c][j] block(EA + 16 s + j) (s = 0: receiver, 1: sender).
// One thread per four columns of an output row; the bias rides along as column block h / 4.
__global__ void __launch_bounds__(256)
k_s2s_charge_filter_fold(const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ emb, int EA, int h,
                         float* __restrict__ W2f, float* __restrict__ b2f) {
    const int q4 = h >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rows = (int64_t)(EA + 4) * h;
    if (idx >= rows * (q4 + 1)) return;
    const int64_t row = idx / (q4 + 1);
    const int cb = (int)(idx - row * (q4 + 1));
    const int f = (int)(row / h), o = (int)(row - (int64_t)f * h);
    if (cb == q4) {                                            // the bias of this row
        float s;
        if (f < EA) s = b2[row];
        else {
            const int sd = (f - EA) >> 1, c = (f - EA) & 1;
            s = 0.0f;
            for (int j = 0; j < S2S_CE; ++j) s = fmaf(emb[c * S2S_CE + j], b2[(size_t)(EA + S2S_CE * sd + j) * h + o], s);
        }
        b2f[row] = s;
        return;
    }
    f32x4 v;
    if (f < EA) v = ld4(W2 + row * h + 4 * cb);
    else {
        const int sd = (f - EA) >> 1, c = (f - EA) & 1;
        v = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < S2S_CE; ++j) {
            const f32x4 w = ld4(W2 + ((size_t)(EA + S2S_CE * sd + j) * h + o) * h + 4 * cb);
            const float e = emb[c * S2S_CE + j];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaf(w[r], e, v[r]);      // (component by component: no packed fp32 math)
        }
    }
    st4(W2f + row * h + 4 * cb, v);
}

// Per entry call: the table rows of every node and edge.  nidx[n] = charge_index[n] in {0, 1}, else 2 (the NaN row of the
// node tables) with the async error word set, nscale[n] (may be null) = 1 or, for such a node, NaN: the row scale of the
// output MLP's last hidden layer, which makes that node's output row NaN; eidx[e] = 2 c_recv + c_send of the indices
// clamped to {0, 1}.  Nothing downstream reads a table with an index that was not made here.
__global__ void __launch_bounds__(256)
k_s2s_charge_index(const int32_t* __restrict__ charge_index, int64_t n_nodes, const int64_t* __restrict__ send,
                   const int64_t* __restrict__ recv, int64_t n_edges, int32_t* __restrict__ nidx, float* __restrict__ nscale,
                   int32_t* __restrict__ eidx, int* __restrict__ errword) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_nodes) {
        const int32_t c = charge_index[t];
        const bool ok = c == 0 || c == 1;
        nidx[t] = ok ? c : 2;
        if (nscale != nullptr) nscale[t] = ok ? 1.0f : __int_as_float(0x7fc00000);
        if (!ok && errword != nullptr) *errword = S2S_ERR_CHARGE;
    }
    if (t < n_edges) {
        const int64_t r = recv[t], s = send[t];
        const int32_t cr = (r >= 0 && r < n_nodes) ? charge_index[r] : 0, cs = (s >= 0 && s < n_nodes) ? charge_index[s] : 0;
        eidx[t] = 2 * (cr == 1 ? 1 : 0) + (cs == 1 ? 1 : 0);
    }
}

// The edge features of the charge-aware step: what k_s2s_edge_prep (s2s_step.h) writes, with rows of edge_attr EA + 4 wide --
// the last four the one-hot indicator features [recv 0, recv 1, send 0, send 1] of the edge's charge pair eidx[e] =
// 2 c_recv + c_send, staged in the LDS row next to the other features (one read of eidx per edge).
template <int D>
__global__ void __launch_bounds__(256)
k_s2s_edge_prep_charges(const float* __restrict__ x, const int64_t* __restrict__ send, const int64_t* __restrict__ recv,
                        const float* __restrict__ rel_feat, int polar, float* __restrict__ edge_attr, float* __restrict__ eap,
                        float* __restrict__ edge_pos, int64_t n_edges, const int32_t* __restrict__ eidx) {
    using A = AugDims<D>;
    constexpr int EAp = (A::EA + 31) / 32 * 32;
    constexpr int W = A::EA + 4;
    constexpr int LDR = W + 1 + (W & 1);                             // odd row stride: conflict-free column writes
    __shared__ float rows[256 * LDR];
    __shared__ float prow[256 * (A::EP + 1)];
    const int64_t e0 = (int64_t)blockIdx.x * 256;
    const int64_t e = e0 + threadIdx.x;
    if (e < n_edges) {
        const int64_t j = send[e], i = recv[e];
        float xj[3 * D], xi[3 * D], o[A::NF];
#pragma unroll
        for (int t = 0; t < 3 * D; ++t) { xj[t] = x[j * 3 * D + t]; xi[t] = x[i * 3 * D + t]; }
        aug_edge<D>(xj, xi, o);
        float* out = rows + threadIdx.x * LDR;
#pragma unroll
        for (int t = 0; t < A::NF; ++t) out[t] = o[t];
#pragma unroll
        for (int t = 0; t < A::RF; ++t) out[A::NF + t] = rel_feat[i * A::RF + t];
        const int pair = eidx[e];
        out[A::EA + 0] = (pair >> 1) == 0 ? 1.0f : 0.0f; out[A::EA + 1] = (pair >> 1) == 1 ? 1.0f : 0.0f;
        out[A::EA + 2] = (pair & 1) == 0 ? 1.0f : 0.0f;  out[A::EA + 3] = (pair & 1) == 1 ? 1.0f : 0.0f;
        const int p0 = polar ? (D == 2 ? 2 : 3) : 0;
#pragma unroll
        for (int t = 0; t < A::EP; ++t) prow[threadIdx.x * (A::EP + 1) + t] = o[p0 + t];
    }
    __syncthreads();
    const int64_t left = n_edges - e0;
    const int cnt = (int)(left < 256 ? left : 256);
    for (int idx = threadIdx.x; idx < cnt * W; idx += 256) {
        const int r = idx / W, c = idx - r * W;
        edge_attr[e0 * W + idx] = rows[r * LDR + c];
    }
    for (int idx = threadIdx.x; idx < cnt * EAp; idx += 256) {
        const int r = idx / EAp, c = idx - r * EAp;
        eap[e0 * EAp + idx] = c < A::EA ? rows[r * LDR + c] : 0.0f;
    }
    for (int idx = threadIdx.x; idx < cnt * A::EP; idx += 256) {
        const int r = idx / A::EP, c = idx - r * A::EP;
        edge_pos[e0 * A::EP + idx] = prow[r * (A::EP + 1) + c];
    }
}

// k_s2s_gate (seq2seq.h) with the guard: the hidden row of a node whose index was outside {0, 1} (nidx 2) is NaN -- the
// activations in between (ReLU, the clamped sigmoid / tanh) do not carry the table's NaN row through on their own.
__global__ void __launch_bounds__(256)
k_s2s_gate_charges(const float* __restrict__ rp, const float* __restrict__ ip, const float* __restrict__ np_,
                   const float* __restrict__ hh, const float* __restrict__ hidden, float* __restrict__ hidden_out, int64_t count,
                   const int32_t* __restrict__ nidx, int hd) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const float r = sigmoid1(rp[idx]);
    const float i = sigmoid1(ip[idx]);
    const float n = tanh1(np_[idx] + r * hh[idx]);
    hidden_out[idx] = nidx[idx / hd] == 2 ? __int_as_float(0x7fc00000) : (1.0f - i) * n + i * hidden[idx];
}

}  // namespace
