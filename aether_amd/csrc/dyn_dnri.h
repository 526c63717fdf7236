// dyn_dnri.h -- the variable-N dNRI baseline (nn/dynamicvars/dnri_dynamicvars.py: DNRIDynamicVars) on the scene engine of
// dyn_step.h.  The model has no local frames and no field: the encoder's prior step (:386-461, :544-570) is the NRI stack on
// the raw 4 columns of the present objects over the encoder's own kNN graph -- mlp1 (nodes) -> [x_send | x_recv] -> mlp2 ->
// index_add_ over the receiver (a SUM, no divisor) -> mlp3 -> [x_send | x_recv | skip] -> mlp4 -- one LSTM step per edge in the
// slot of the CALLER's edge of the same position, and prior_fc_out; the decoder (:618-688) passes tanh messages between hidden
// states on the caller's graph, sums them over the edge2node rows / (num_vars - 1) of the scene and gates them GRU-style with
// input_r / _i / _n of the raw inputs.  The scene bookkeeping (k_dynb_present, k_dynb_csr, k_dyn_scatter_sample, k_dyn_mix),
// the kNN builder, the dense job tables, the LSTM cell and the sample are the engine's; s2s_dnri.h gives the index-generic
// pair / gate kernels.  The kernels here are what the ragged, many-scene case needs on top.  Only k_dynb_dnri_index takes a
// struct by value (the scene table), and none reads a hidden kernel argument (tools/isa_check.py R4).
#pragma once
#include "dyn_step.h"
#include "s2s_dnri.h"

namespace {

// k_dynb_index without the frame side: the caller's graphs, scene-local numbering -> send / recv in the consecutive numbering
// of all scenes, slot = s n_max (n_max - 1) + gs (n_max - 1) + gr - (gr >= gs) with gs / gr the object rows of the ends
// (dnri_dynamicvars.py:554-556), h0 / c0 = the LSTM state rows of the slots, and order[j] = edge2node[j] + the scene's first
// edge.  No ext_full, no un-compacted send / recv: nothing here reads a state through an edge.
__global__ void __launch_bounds__(256)
k_dynb_dnri_index(const DynScenes S, const int64_t* __restrict__ gsend, const int64_t* __restrict__ grecv,
                  const int64_t* __restrict__ node_inds /* scene-local rows, concatenated; null: from idx */,
                  const int64_t* __restrict__ idx, const int64_t* __restrict__ e2n, int R, const float* __restrict__ prior_h,
                  const float* __restrict__ prior_c, int64_t* __restrict__ send, int64_t* __restrict__ recv,
                  int64_t* __restrict__ slot, float* __restrict__ h0, float* __restrict__ c0, int64_t* __restrict__ order) {
    __shared__ int off[3 * (DYN_MAX_SCENES + 1)];
    __shared__ int part[257];
    dyn_scene_offsets(S, off, part);
    const int* nb = off; const int* eb = off + (DYN_MAX_SCENES + 1); const int* ob = off + 2 * (DYN_MAX_SCENES + 1);
    const int E = eb[DYN_MAX_SCENES], O = ob[DYN_MAX_SCENES];
    const int r4 = R >> 2, n_max = S.n_max;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < O) {
        const int s = dyn_scene_of(ob, S.n_scenes, (int)t);
        const int Es = eb[s + 1] - eb[s];
        int64_t v = e2n[t];
        v = v < 0 ? 0 : (v >= Es ? Es - 1 : v);                  // (refused on the host side of the module; clamped here)
        order[t] = v + eb[s];
    }
    if (t >= (int64_t)E * r4) return;
    const int e = (int)(t / r4), o = (int)(t - (int64_t)e * r4);
    const int s = dyn_scene_of(eb, S.n_scenes, e);
    const int n = S.n[s], nbase = nb[s];
    int64_t a = gsend[e], b = grecv[e];
    a = a < 0 ? 0 : (a >= n ? n - 1 : a);
    b = b < 0 ? 0 : (b >= n ? n - 1 : b);
    int64_t gs, gr;
    if (node_inds != nullptr) { gs = node_inds[nbase + a]; gr = node_inds[nbase + b]; }
    else { gs = idx[nbase + a] - (int64_t)s * n_max; gr = idx[nbase + b] - (int64_t)s * n_max; }
    gs = gs < 0 ? 0 : (gs >= n_max ? n_max - 1 : gs);
    gr = gr < 0 ? 0 : (gr >= n_max ? n_max - 1 : gr);
    const int64_t per = (int64_t)n_max * (n_max - 1);
    int64_t sl = gs * (n_max - 1) + gr - (gr >= gs ? 1 : 0);
    sl = (sl < 0 ? 0 : (sl >= per ? per - 1 : sl)) + (int64_t)s * per;
    if (o == 0) { slot[e] = sl; send[e] = nbase + a; recv[e] = nbase + b; }
    st4(h0 + (size_t)e * R + 4 * o, ld4(prior_h + sl * R + 4 * o));
    st4(c0 + (size_t)e * R + 4 * o, ld4(prior_c + sl * R + 4 * o));
}

// The node front of the prior step in one launch: mlp1's first Linear on the 4 raw columns + ELU (:412; a K = 4 product is
// no matrix-core job), Y[n][m] = ELU(b[m] + sum_c W[m][c] x[n][c]), a thread per (node, 4 units) -- and, by the first
// threads of the grid, what the step needs of the parameters: the eval-mode BatchNorm affines of mlp1 .. mlp4 (scale | shift,
// bn [4][2][h]; a layer without statistics -- no_encoder_bn -- is skipped and never read) and the summed LSTM biases lb [4R].
// The host sizes the grid for the largest of the three.
__global__ void __launch_bounds__(256)
k_dyn_dnri_node_in(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                   float* __restrict__ Y, int h, int64_t n_nodes, const float* w0, const float* w1, const float* w2,
                   const float* w3, const float* s0, const float* s1, const float* s2, const float* s3, const float* m0,
                   const float* m1, const float* m2, const float* m3, const float* v0, const float* v1, const float* v2,
                   const float* v3, float* __restrict__ bn, const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                   float* __restrict__ lb, int R) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < 4 * (int64_t)h) {
        const int l = (int)(idx / h), c = (int)(idx - (int64_t)l * h);
        const float* w = l == 0 ? w0 : l == 1 ? w1 : l == 2 ? w2 : w3;
        if (w != nullptr) {
            const float* sh = l == 0 ? s0 : l == 1 ? s1 : l == 2 ? s2 : s3;
            const float* mean = l == 0 ? m0 : l == 1 ? m1 : l == 2 ? m2 : m3;
            const float* var = l == 0 ? v0 : l == 1 ? v1 : l == 2 ? v2 : v3;
            const float sc = w[c] / sqrtf(var[c] + 1e-5f);
            bn[(size_t)(2 * l) * h + c] = sc;
            bn[(size_t)(2 * l + 1) * h + c] = sh[c] - mean[c] * sc;
        }
    }
    if (idx < 4 * (int64_t)R) lb[idx] = b_ih[idx] + b_hh[idx];
    const int q4 = h >> 2;
    if (idx >= n_nodes * q4) return;
    const int64_t n = idx / q4;
    const int m = (int)(idx - n * q4) * 4;
    const f32x4 xv = ld4(x + n * 4);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const f32x4 wv = ld4(W + (size_t)(m + r) * 4);
        float sv = b[m + r];
        sv = fmaf(wv[0], xv[0], sv); sv = fmaf(wv[1], xv[1], sv); sv = fmaf(wv[2], xv[2], sv); sv = fmaf(wv[3], xv[3], sv);
        v[r] = elu1(sv);
    }
    st4(Y + (size_t)n * h + m, v);
}

// batch_edge2node (:374-377): out[n][:] = sum over the in-edges of n in the kNN graph of X[e][:], in edge order (order / rowptr:
// the receiver CSR k_dynb_csr builds) -- a plain sum: index_add_ has no divisor, whatever the scene's size.
__global__ void __launch_bounds__(128)
k_dyn_dnri_recv_sum(const float* __restrict__ X, const int64_t* __restrict__ order, const int64_t* __restrict__ rowptr,
                    float* __restrict__ out, int h) {
    const int64_t n = blockIdx.x;
    const int64_t beg = rowptr[n], end = rowptr[n + 1];
    for (int c = threadIdx.x * 4; c < h; c += 128 * 4) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t k = beg; k < end; ++k) s += ld4(X + (size_t)order[k] * h + c);
        st4(out + (size_t)n * h + c, s);
    }
}

// The decoder's aggregation (:656-661) over the caller's edge2node lists: out[n][:] = (sum over order[rowptr[n] ..
// rowptr[n + 1]) of M[e][:] / msg_div) / div[n] with msg_div the number of used edge types and div[n] the scene's num_vars - 1
// -- per OBJECT: scenes of one call differ in size (div == nullptr: the scalar agg_div for every object).
__global__ void __launch_bounds__(128)
k_dyn_dnri_aggregate(const float* __restrict__ M, const int64_t* __restrict__ order, const int64_t* __restrict__ rowptr,
                     float* __restrict__ out, int h, float msg_div, float agg_div, const float* __restrict__ div) {
    const int64_t n = blockIdx.x;
    const int64_t beg = rowptr[n], end = rowptr[n + 1];
    const float d = div != nullptr ? div[n] : agg_div;
    for (int c = threadIdx.x * 4; c < h; c += 128 * 4) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t k = beg; k < end; ++k) s += ld4(M + (size_t)order[k] * h + c) / msg_div;
        st4(out + (size_t)n * h + c, s / d);
    }
}

// out_fc3, the residual (:680-682) and, in the one-call step, the scatter to the un-compacted rows (:683-686) in one launch.
// A wave per row, butterfly sums (the arithmetic of k_s2s_dnri_out<2>).
//   cidx == nullptr (the staged decoder step): row = compacted object c; out[c] = x[c] + W3 o2[c] + b3.
//   cidx != nullptr (the step): row = flat object row of [B n_max]; c = cidx[row]; present rows get the prediction and
//     hidden[row] = new_h[c]; absent rows get zeros and keep their hidden state.  status[0] != 0 (a mask disagreed with its
//     n_present): NaN in every prediction row and in the hidden rows that would have been written.
__global__ void __launch_bounds__(256)
k_dyn_dnri_out(const float* __restrict__ o2, const float* __restrict__ w3, const float* __restrict__ b3, int hd,
               const float* __restrict__ x, float* __restrict__ out, int64_t n_rows, const int* __restrict__ cidx,
               const int* __restrict__ status, const float* __restrict__ new_h, float* __restrict__ hidden) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    int64_t c = row;
    const bool bad = status != nullptr && status[0] != 0;
    const float poison = __int_as_float(0x7fc00000);
    if (cidx != nullptr) {
        c = cidx[row];
        if (c < 0) {
            if (lane < 4) out[row * 4 + lane] = bad ? poison : 0.0f;
            return;
        }
        for (int k = 4 * lane; k < hd; k += 256) {
            f32x4 v = ld4(new_h + (size_t)c * hd + k);
            if (bad) v = f32x4{poison, poison, poison, poison};
            st4(hidden + (size_t)row * hd + k, v);
        }
    }
    float pred[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 4 * lane; k < hd; k += 256) {
        const f32x4 xv = ld4(o2 + (size_t)c * hd + k);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 wv = ld4(w3 + (size_t)t * hd + k);
            pred[t] += wv[0] * xv[0] + wv[1] * xv[1] + wv[2] * xv[2] + wv[3] * xv[3];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) pred[t] += __shfl_xor(pred[t], off);
    }
    if (lane != 0) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) out[row * 4 + t] = bad ? poison : x[c * 4 + t] + (pred[t] + b3[t]);
}

}  // namespace
