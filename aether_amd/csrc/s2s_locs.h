// The seq2seq LoCS baseline (nn/seq2seq/locs.py): the fused step of s2s_step.h behind the PLAIN localizer
// (nn/utils/global_to_local.py:46-62) instead of the augmented one -- no field query, no virtual origin node, no force columns:
//   canonicalize_inputs            nn/utils/canonicalization.py:12-30    rel_feat [2D]: 2-D [0, 0, |v|, 0], 3-D [0_3 | R^T v]
//   create_edge_attr_pos_vel       canonicalization.py:78-108  (2-D)     3D + O = 7 features per edge
//   create_3d_edge_attr_pos_vel    canonicalization.py:175-202 (3-D)     3D + O = 12
//   Localizer._edge_pos_idx_fn     global_to_local.py:16-21              cart: columns 0 .., polar: columns D ..
// The edge row is [features | rel_feat[recv]], 5D + O = 11 / 18 wide (the augmented one: 24 / 39).  The features are the
// augmented ones of seq2seq.h without their trailing force columns, computed by the same device function (aug_edge) on a
// zero force, so the angle conventions -- angle_diff, wrap_angles(normalize=True), ZYX Euler angles -- live in one place.
// Only the two kernels in front of the step differ; everything behind them runs on the job tables with LocsDims' widths.
#pragma once
#include "s2s_step.h"

namespace {

template <int D> struct LocsDims {
    static constexpr int O = D * (D - 1) / 2, NF = 3 * D + O, RF = 2 * D, EA = NF + RF, EP = D + O;
};

// Node side of the plain local frames (in the place of k_s2s_node_prep): a thread per node builds the frame Rinv from the
// velocity, rel_feat, its zero-padded copies at the row strides the dense layers read (ldp: the prior's / the Markov
// decoder's res1; the first S2S_RFG columns of the recurrent decoder's wide gate row) and clears the per-type edge counters
// of the step.
template <int D>
__global__ void __launch_bounds__(256)
k_s2s_locs_node_prep(const float* __restrict__ inputs, float* __restrict__ rel_feat, float* __restrict__ Rinv,
                     float* __restrict__ relp, int ldp, float* __restrict__ wide, int ldwide, int* __restrict__ counts,
                     int64_t n_nodes) {
    using A = LocsDims<D>;
    constexpr int RFp = (A::RF + 15) / 16 * 16;
    if (blockIdx.x == 0 && threadIdx.x < 8 && counts != nullptr) counts[threadIdx.x] = 0;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_nodes) return;
    float xi[2 * D];
#pragma unroll
    for (int t = 0; t < 2 * D; ++t) xi[t] = inputs[n * 2 * D + t];
    float row[A::RF];
    float R[D][D];
    if constexpr (D == 2) {
        const float ang = atan2f(xi[3], xi[2]);
        const float c = cosf(ang), s = sinf(ang);
        R[0][0] = c; R[0][1] = -s; R[1][0] = s; R[1][1] = c;
        row[0] = 0.f; row[1] = 0.f; row[2] = sqrtf(xi[2] * xi[2] + xi[3] * xi[3]); row[3] = 0.f;
    } else {
        float rho, th, ph;
        spherical3(xi + 3, rho, th, ph);
        rot3(th, ph, R);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            row[a] = 0.f;
            row[3 + a] = R[0][a] * xi[3] + R[1][a] * xi[4] + R[2][a] * xi[5];
        }
    }
#pragma unroll
    for (int t = 0; t < A::RF; ++t) rel_feat[n * A::RF + t] = row[t];
#pragma unroll
    for (int t = 0; t < RFp; ++t) relp[n * ldp + t] = t < A::RF ? row[t < A::RF ? t : 0] : 0.0f;
    if (wide != nullptr) {                            // S2S_RFG columns: a whole 32-wide k block for the split GEMM
#pragma unroll
        for (int t = 0; t < S2S_RFG; ++t) wide[n * ldwide + t] = t < A::RF ? row[t < A::RF ? t : 0] : 0.0f;
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) Rinv[n * D * D + a * D + b] = R[a][b];
}

// Edge side (in the place of k_s2s_edge_prep): edge_attr [E][5D + O] as the filter GEMM reads it, its zero-padded copy
// [E][EAp] for the decoder's present-message / lin1 layer, edge_pos [E][D + O] for either position representation.
// x: the step's inputs [n_nodes][2D] themselves (there is no extended state).  A thread per edge, rows staged in LDS and
// written out coalesced, as k_s2s_edge_prep.
template <int D>
__global__ void __launch_bounds__(256)
k_s2s_locs_edge_prep(const float* __restrict__ x, const int64_t* __restrict__ send, const int64_t* __restrict__ recv,
                     const float* __restrict__ rel_feat, int polar, float* __restrict__ edge_attr, float* __restrict__ eap,
                     float* __restrict__ edge_pos, int64_t n_edges) {
    using A = LocsDims<D>;
    constexpr int EAp = (A::EA + 31) / 32 * 32;
    constexpr int LDR = A::EA + 1 + (A::EA & 1);                      // odd row stride: conflict-free column writes
    __shared__ float rows[256 * LDR];
    __shared__ float prow[256 * (A::EP + 1)];
    const int64_t e0 = (int64_t)blockIdx.x * 256;
    const int64_t e = e0 + threadIdx.x;
    if (e < n_edges) {
        const int64_t j = send[e], i = recv[e];
        float xj[3 * D], xi[3 * D], o[AugDims<D>::NF];
#pragma unroll
        for (int t = 0; t < 2 * D; ++t) { xj[t] = x[j * 2 * D + t]; xi[t] = x[i * 2 * D + t]; }
#pragma unroll
        for (int t = 2 * D; t < 3 * D; ++t) { xj[t] = 0.0f; xi[t] = 0.0f; }
        aug_edge<D>(xj, xi, o);                                      // its first 3D + O columns are the plain localizer's
        float* out = rows + threadIdx.x * LDR;
#pragma unroll
        for (int t = 0; t < A::NF; ++t) out[t] = o[t];
#pragma unroll
        for (int t = 0; t < A::RF; ++t) out[A::NF + t] = rel_feat[i * A::RF + t];
        const int p0 = polar ? D : 0;                                // global_to_local.py:16-21
#pragma unroll
        for (int t = 0; t < A::EP; ++t) prow[threadIdx.x * (A::EP + 1) + t] = o[p0 + t];
    }
    __syncthreads();
    const int64_t left = n_edges - e0;
    const int cnt = (int)(left < 256 ? left : 256);
    for (int idx = threadIdx.x; idx < cnt * A::EA; idx += 256) {
        const int r = idx / A::EA, c = idx - r * A::EA;
        edge_attr[e0 * A::EA + idx] = rows[r * LDR + c];
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

}  // namespace
