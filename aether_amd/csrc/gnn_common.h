// gnn_common.h -- what egnn.h and clof.h share word for word: the expf-based SiLU (NOT common.h's silu, which is other
// arithmetic), the weight-gradient job table and the second stage of the weight-gradient reduction.  Each model keeps
// its own first stage (k_egnn_wgrad_part on the vector ALU, k_clof_wgrad_part on the matrix cores).

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

}  // namespace gnn
