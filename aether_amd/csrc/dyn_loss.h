// dyn_loss.h -- what the evaluation half of calculate_loss of the variable-N models needs on top of the scene engine
// (dyn_step.h, dyn_dnri.h): nn/dynamicvars/aether_dynamicvars.py:152-207, dnri_dynamicvars.py:70-114.
//
// The sequence encoder (Encoder.forward, aether_dynamicvars.py:588-670 / dnri_dynamicvars.py:463-542) never writes its
// forward LSTM state back (tmp_state0 / tmp_state1 are built and dropped, :632-635 / :506-509) and its reverse pass never
// calls reverse_rnn (:657-662 / :531-536): every frame t gives h_t = LSTMcell(x_t, (0, 0)), prior = prior_fc_out(h_t),
// posterior = encoder_fc_out([h_t | 0]).  The frames are independent, so they run as scenes of ONE prior stage, and the LSTM
// step from the zero state is k_dyn_lstm_zero: no W_hh product, no h0 / c0 loads, no forget gate (it multiplies c0 = 0), no
// slot gather or scatter.  The teacher-forced decoding loop (:171-193 / :83-100) has no prior stage either: per step
// k_dyn_loss_graph puts the data set's graph into the numbering the decoder stage takes.
// Neither kernel takes a struct by value or reads a hidden kernel argument.
#pragma once
#include "dyn_step.h"

namespace {

// h1[e][u] = sig(o) tanh(sig(i) tanh(g)),  (i, g, o)[e][u] = W_ih[gate R + u][:] . x[e][:] + b_ih[gate R + u] + b_hh[gate R + u]
// (torch.nn.LSTM gate order i, f, g, o: gate rows 0, 2, 3).  A wave owns 16 rows x 16 units: three independent accumulators of
// v_mfma_f32_16x16x4_f32 (exact fp32 products and sums; two or more independent chains reach its issue rate), operands
// straight from global memory as one 16-byte fragment per lane and 16 columns of k -- lane (i, q) holds columns 16 a + 4 q
// + b of row i, the MFMA of b sums the columns {16 a + 4 q + b : q}; W_ih (3 R rows of h floats) stays in L2 for every row
// tile.  Grid: (ceil(n_rows / 64), R / 16), 4 waves each on their own 16 rows.  h % 16 == 0, R % 16 == 0.
// status (may be null): status[0] != 0 -- a frame's mask disagreed with its n_present -- writes NaN, which the heads carry
// into every logit.
__global__ void __launch_bounds__(256)
k_dyn_lstm_zero(const float* __restrict__ x, const float* __restrict__ w_ih, const float* __restrict__ b_ih,
                const float* __restrict__ b_hh, int h, int R, int64_t n_rows, const int* __restrict__ status,
                float* __restrict__ h1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (r0 >= n_rows) return;
    const int u0 = blockIdx.y * 16;
    const int64_t xr = r0 + i < n_rows ? r0 + i : n_rows - 1;          // rows past the end read the last row, and are not stored
    const float* xp = x + (size_t)xr * h + 4 * q;
    const float* wi = w_ih + (size_t)(u0 + i) * h + 4 * q;
    const float* wg = w_ih + (size_t)(2 * R + u0 + i) * h + 4 * q;
    const float* wo = w_ih + (size_t)(3 * R + u0 + i) * h + 4 * q;
    f32x4 ai = {0.f, 0.f, 0.f, 0.f}, ag = ai, ao = ai;
    for (int k = 0; k < h; k += 16) {
        const f32x4 xv = ld4(xp + k), vi = ld4(wi + k), vg = ld4(wg + k), vo = ld4(wo + k);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            ai = mfma16(xv[b], vi[b], ai);
            ag = mfma16(xv[b], vg[b], ag);
            ao = mfma16(xv[b], vo[b], ao);
        }
    }
    // accumulator register j of lane (i, q): row r0 + 4 q + j, unit u0 + i
    const int u = u0 + i;
    const float bi = b_ih[u] + b_hh[u], bg = b_ih[2 * R + u] + b_hh[2 * R + u], bo = b_ih[3 * R + u] + b_hh[3 * R + u];
    const bool bad = status != nullptr && status[0] != 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + 4 * q + j;
        if (r >= n_rows) continue;
        const float c = sigmoid1(ai[j] + bi) * tanh1(ag[j] + bg);
        const float v = sigmoid1(ao[j] + bo) * tanh1(c);
        h1[(size_t)r * R + u] = bad ? __int_as_float(0x7fc00000) : v;
    }
}

// One step of the decoding loop, one scene: the data set's graph of the step (numbering of the present objects) as the
// decoder stage takes it.  send / recv = the ids clamped into 0 .. n - 1 (the scene's first consecutive number is 0),
// order[j] = edge2node[j] clamped into 0 .. n_edges - 1 (refused on the host side of the module; clamped here), and, for the
// model with frames (ssend != null), ssend / srecv = the same ids -- rows of the UN-compacted ext_full, the reference's quirk
// (aether_dynamicvars.py:823) -- with ext_full[row] = [state | field of the present row or 0].  The first thread folds the
// scene's mismatch word (k_dynb_present) into status[0], which the decoder's last kernel reads: no kNN stage does it here.
__global__ void __launch_bounds__(256)
k_dyn_loss_graph(const int64_t* __restrict__ gsend, const int64_t* __restrict__ grecv, const int64_t* __restrict__ e2n, int n,
                 int64_t n_edges, int64_t n_e2n, int n_max, int64_t* __restrict__ send, int64_t* __restrict__ recv,
                 int64_t* __restrict__ order, int64_t* __restrict__ ssend, int64_t* __restrict__ srecv,
                 const float* __restrict__ state, const float* __restrict__ field_c, const int* __restrict__ cidx,
                 float* __restrict__ ext_full, int* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) status[0] = status[1];
    if (ssend != nullptr && t < (int64_t)n_max * 6) {
        const int64_t row = t / 6;
        const int col = (int)(t - row * 6);
        float v;
        if (col < 4) v = state[row * 4 + col];
        else { const int c = cidx[row]; v = c >= 0 ? field_c[(size_t)c * 2 + col - 4] : 0.0f; }
        ext_full[t] = v;
    }
    if (t < n_e2n) {
        const int64_t v = e2n[t];
        order[t] = v < 0 ? 0 : (v >= n_edges ? n_edges - 1 : v);
    }
    if (t >= n_edges) return;
    int64_t a = gsend[t], b = grecv[t];
    a = a < 0 ? 0 : (a >= n ? n - 1 : a);
    b = b < 0 ? 0 : (b >= n ? n - 1 : b);
    send[t] = a; recv[t] = b;
    if (ssend != nullptr) { ssend[t] = a; srecv[t] = b; }
}

}  // namespace
