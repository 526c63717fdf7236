// gnn_common.h -- what egnn.h and clof.h share word for word: the expf-based SiLU (NOT common.h's silu, which is other
// arithmetic), the weight-gradient job table and the second stage of the weight-gradient reduction.  Each model keeps
// its own first stage (k_egnn_wgrad_part on the vector ALU, k_clof_wgrad_part on the matrix cores).  And the state
// advance of their device rollouts (k_gnn_rollout_state).

#pragma once

namespace gnn {

__device__ __forceinline__ float sig(float a) { return 1.0f / (1.0f + expf(-a)); }
__device__ __forceinline__ float silu(float a) { return a * sig(a); }
__device__ __forceinline__ float dsilu(float a) { const float s = sig(a); return s * (1.0f + a * (1.0f - s)); }

// out[j][k] (row stride ldo) = sum_i G[i][j] act(A[i][k]), i over `rows`; A null: a column of ones (a bias); act: 1 = SiLU
// (k_clof_wgrad_part only; EGNN's jobs carry 0).  Two deterministic stages: row chunk c of every output tile ->
// part[c][...], then the chunks in order.
struct WgJob {
    const float *G, *A;
    float* out;
    int ldg, lda, ldo, J, K, act;
    int64_t rows;
    int tile0, poff;            // first tile of the job; offset of its J * K partials
};
constexpr int WGJ_MAX = 24;     // jobs of one weight-gradient launch
struct WgJobs { WgJob j[WGJ_MAX]; int n, n_tiles, n_out, n_ch; };

__global__ __launch_bounds__(256) void k_gnn_wgrad_sum(WgJobs T, const float* __restrict__ part) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= T.n_out) return;
    int q = 0;
    while (q + 1 < T.n && T.j[q + 1].poff <= idx) ++q;
    const WgJob& J = T.j[q];
    const int o = idx - J.poff, jj = o / J.K, kk = o % J.K;
    float s = 0.0f;
    for (int c = 0; c < T.n_ch; ++c) s += part[(int64_t)c * T.n_out + idx];
    J.out[(int64_t)jj * J.ldo + kk] = s;
}

// a^2 + b^2 + c^2 with every product and sum rounded (no fused multiply-add), as torch.sum(t ** 2, 1) rounds
__device__ __forceinline__ float sum_sq3(float a, float b, float c) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c));
}

// State advance of a device rollout (host_gnn_common.inc: gnn_rollout): from the positions x of the step about to run and
// x_prev of the step before (null at step 0, which takes vel0), the inputs of that step in the layouts the layer kernels
// read -- what the runner prepares per batch (experiments/lorentz/main.py:255-257, 267-269):
//   vel[n]  = (x[n] - x_prev[n]) / dt          h[n] = |vel[n]|   (`nodes`, in_node_nf = 1)
//   ea[e]   = [q_row q_col, |x_row - x_col|^2]  in the caller's edge order, row = recv[e], col = send[e]
// The charge product never changes: FIRST writes it, later steps leave it.  Thread i takes node i and edge i; every
// output element has one writer.  An index outside [0, n_nodes) (an edge list the graph view was not built from) reads
// nothing and leaves NaN.  The squares are summed as the runner's tensor ops round them (sum_sq3).
template <bool FIRST>
__global__ __launch_bounds__(256) void k_gnn_rollout_state(int64_t Nn, int64_t E, const float* __restrict__ x,
                                                           const float* __restrict__ x_prev, const float* __restrict__ vel0,
                                                           float dt, const float* __restrict__ charges,
                                                           const int64_t* __restrict__ recv, const int64_t* __restrict__ send,
                                                           float* __restrict__ vel, float* __restrict__ h,
                                                           float* __restrict__ ea) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < Nn) {
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = FIRST ? vel0[i * 3 + k] : (x[i * 3 + k] - x_prev[i * 3 + k]) / dt;
            vel[i * 3 + k] = v[k];
        }
        h[i] = sqrtf(sum_sq3(v[0], v[1], v[2]));
    }
    if (i < E) {
        const int64_t r = recv[i], c = send[i];
        const bool ok = r >= 0 && r < Nn && c >= 0 && c < Nn;
        float d2 = __builtin_nanf("");
        if (ok) {
            const float d0 = x[r * 3] - x[c * 3], d1 = x[r * 3 + 1] - x[c * 3 + 1], d2z = x[r * 3 + 2] - x[c * 3 + 2];
            d2 = sum_sq3(d0, d1, d2z);
        }
        if (FIRST) ea[i * 2] = ok ? charges[r] * charges[c] : d2;
        ea[i * 2 + 1] = d2;
    }
}

}  // namespace gnn
