// Device kernels of the seq2seq Aether's Markov decoder (MarkovDecoder, nn/seq2seq/aether.py:413-503) that the shared
// pieces (k_s2s_node_prep / k_s2s_edge_prep, the job-table GEMMs, k_s2s_gumbel_select, k_s2s_out_globalize) cannot express.
#pragma once

namespace {

// lin2's bias in per-type blocks: dst[k h + c] = src[c Ku + k] (MLPEdgeFilter's output column c Ku + k is channel c of
// used type k, aether.py:482-484).  The weight rows need no copy: type k's h x h block is lin2_w + k h at row stride Ku h.
__global__ void __launch_bounds__(256)
k_s2s_markov_bias(const float* __restrict__ src, int ku, int h, float* __restrict__ dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ku * h) return;
    const int k = idx / h, c = idx - k * h;
    dst[idx] = src[c * ku + k];
}

// aug[n][:] += (sum over the node's in-edges of M[edge][:]) / in-degree: the receiver mean of the messages (torch_scatter
// mean, aether.py:487-489) added onto res1(rel_feat) (:492-493), which aug holds.  edge_w != nullptr (hard samples of the
// fused step): the row of an edge that no used type k0 <= k < K carries was never written and counts as zero, as the
// reference's product with a zero weight does (the edge still counts in the degree).  One workgroup per node, fixed order.
__global__ void __launch_bounds__(128)
k_s2s_markov_agg(const float* __restrict__ M, const int64_t* __restrict__ order, const int64_t* __restrict__ rowptr,
                 const float* __restrict__ edge_w, int K, int k0, float* __restrict__ aug, int h) {
    const int64_t n = blockIdx.x;
    const int64_t beg = rowptr[n], end = rowptr[n + 1];
    for (int c = threadIdx.x * 4; c < h; c += 128 * 4) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t k = beg; k < end; ++k) {
            const int64_t e = order[k];
            if (edge_w != nullptr) {
                bool used = false;
                for (int t = k0; t < K; ++t) used = used || edge_w[e * K + t] != 0.0f;
                if (!used) continue;
            }
            s += ld4(M + (size_t)e * h + c);
        }
        const float cnt = (float)(end - beg > 1 ? end - beg : 1);
        st4(aug + (size_t)n * h + c, ld4(aug + (size_t)n * h + c) + s / cnt);
    }
}

}  // namespace
