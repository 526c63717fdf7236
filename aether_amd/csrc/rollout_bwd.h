// rollout_bwd.h -- what joins the per-step backward kernels into a backward through a whole device rollout
// (aether_rollout_backward, host_rollout_train.inc).  Included after backward.h (sum32).
//
// Protocol (oracle/aether_oracle.py::rollout; the runner's per-batch prep, experiments/lorentz/main.py:243-247):
//   x_{t+1} = Aether(x_t, v_t, ea_t),  ea_t = [q_i q_j, |x_row - x_col|] from x_t,  v_{t+1} = (x_{t+1} - x_t) / dt.
// Step t's backward (aether_backward + aether_backward_inputs on that step's slice of the workspace) leaves
//   gx_t = dL/dx_t through the step, gv_t = dL/dv_t, gea_t = dL/dea_t [E][2] (caller's edge order).
// k_rollout_chain then forms, in ONE launch, the grad_out of the next-earlier step
//   X_t = g_t + gx_t + sum_e gea_t[e, 1] d|x_row - x_col|/dx_t + gv_t / dt - gv_{t+1} / dt
// (g_t: the caller's dL/dx_t; x_t feeds step t directly and through the distances, v_t = (x_t - x_{t-1}) / dt and
// v_{t+1} = (x_{t+1} - x_t) / dt), for t = 0 the results dL/dx_0 = gx_0 + distances - gv_1 / dt and dL/dv_0 = gv_0, and -- in
// further workgroups of the same launch -- adds the step's parameter gradients to the running sum.
//
// The distance term of a node is a sum over its in-edge list (receiver CSR: rowptr / send_s / perm) and its out-edge
// list (sender lists: srowptr / sperm) of the graph view: 32 lanes per node take consecutive list entries (coalesced
// reads of the index arrays), then a fixed butterfly -- no float atomics, same bits on every run.  Repeated edges are
// list entries of their own; a node without in- or out-edges has an empty list.  End points that coincide exactly
// (d = 0, self loops included) are UNDEFINED in the protocol (the distance has no derivative there); such an edge
// contributes nothing here.
#pragma once

namespace {

constexpr int RC_MAX_TENSORS = 47;          // pointers of an AetherParams
constexpr int RC_ADD_BLOCK = 1024;          // floats per workgroup of the parameter-gradient sum (256 threads x 4)

// Parameter gradients summed over the steps: dst[k][i] += src[off[k] + i].  One step is added per launch, step K - 1 first
// (it is written straight into dst), so the order of the sum -- and its bits -- are fixed.
struct RolloutParamAdd {
    float* dst[RC_MAX_TENSORS];
    int numel[RC_MAX_TENSORS];
    int off[RC_MAX_TENSORS];                // start of tensor k in src (floats, multiples of 4)
    int block0[RC_MAX_TENSORS + 1];         // first workgroup (after the node workgroups) of tensor k
    const float* src;
    int n;                                  // tensors; 0: nothing to add in this launch
};

template <int D>
__global__ void __launch_bounds__(256)
k_rollout_chain(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ gx,
                const float* __restrict__ gv, const float* __restrict__ gv_next, const float* __restrict__ gea,
                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ send_s, const int32_t* __restrict__ recv_s,
                const int32_t* __restrict__ perm, const int32_t* __restrict__ srowptr, const int32_t* __restrict__ sperm,
                float inv_dt, float* __restrict__ out_x, float* __restrict__ out_v, int64_t n_nodes, int node_blocks,
                RolloutParamAdd A) {
    if ((int)blockIdx.x >= node_blocks) {           // (workgroup-uniform) parameter-gradient sum
        const int b = (int)blockIdx.x - node_blocks;
        int k = 0;
        while (k + 1 < A.n && b >= A.block0[k + 1]) ++k;
        const int i0 = (b - A.block0[k]) * RC_ADD_BLOCK + threadIdx.x * 4;
        const float* src = A.src + A.off[k];
        float* dst = A.dst[k];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < A.numel[k]) dst[i0 + j] += src[i0 + j];
        return;
    }
    const int grp = threadIdx.x >> 5, t = threadIdx.x & 31;
    const int64_t n = (int64_t)blockIdx.x * 8 + grp;
    const bool ok = n < n_nodes;
    const int64_t nc = ok ? n : n_nodes - 1;
    float xn[D], acc[D];
#pragma unroll
    for (int b = 0; b < D; ++b) { xn[b] = x[nc * D + b]; acc[b] = 0.f; }
    // in-edges row -> n: d|x_row - x_n| / dx_n = -(x_row - x_n) / d
    for (int k = rowptr[nc] + t; k < rowptr[nc + 1]; k += 32) {
        const int64_t s = send_s[k];
        const float w = gea[2 * (int64_t)perm[k] + 1];
        float rel[D], d2 = 0.f;
#pragma unroll
        for (int b = 0; b < D; ++b) { rel[b] = x[s * D + b] - xn[b]; d2 += rel[b] * rel[b]; }
        const float d = sqrtf(d2);
        const float c = d > 0.f ? w / d : 0.f;
#pragma unroll
        for (int b = 0; b < D; ++b) acc[b] -= c * rel[b];
    }
    // out-edges n -> col: d|x_n - x_col| / dx_n = (x_n - x_col) / d
    for (int kk = srowptr[nc] + t; kk < srowptr[nc + 1]; kk += 32) {
        const int64_t k = sperm[kk];
        const int64_t r = recv_s[k];
        const float w = gea[2 * (int64_t)perm[k] + 1];
        float rel[D], d2 = 0.f;
#pragma unroll
        for (int b = 0; b < D; ++b) { rel[b] = xn[b] - x[r * D + b]; d2 += rel[b] * rel[b]; }
        const float d = sqrtf(d2);
        const float c = d > 0.f ? w / d : 0.f;
#pragma unroll
        for (int b = 0; b < D; ++b) acc[b] += c * rel[b];
    }
#pragma unroll
    for (int b = 0; b < D; ++b) acc[b] = sum32(acc[b]);
    if (!ok || t >= D) return;
    float res = 0.f;
#pragma unroll
    for (int b = 0; b < D; ++b)
        if (t == b) res = acc[b];
    const int64_t idx = n * D + t;
    res += gx[idx];
    if (gv_next != nullptr) res -= gv_next[idx] * inv_dt;
    if (g != nullptr) res += g[idx] + gv[idx] * inv_dt;           // t >= 1: x_t is a loss term and the end point of v_t
    if (out_x != nullptr) out_x[idx] = res;
    if (out_v != nullptr) out_v[idx] = gv[idx];                   // t = 0: dL/dv_0
}

}  // namespace
