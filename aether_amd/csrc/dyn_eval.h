// Forward-prediction metric of the inD runner (experiments/ind/evaluate.py:29-80) for B scenes at once.
// The reference walks the objects of ONE scene in Python, with several .item() calls per object; here a track
// (scene, object) is one wave:
//   k_de_track : finds the track's first predicted step and their number, and writes the track's contributions to the
//                horizons 0 .. num-1 (total, position, velocity error and count) as one row of scratch, zero beyond num
//   k_de_reduce: adds the rows column by column, track after track, in fp64 and ADDS the column sums to the caller's
//                accumulators; one more thread folds the per-track flags into the bad count and the longest horizon
// No atomics: the sum of a column has one fixed order.
#pragma once
#include "common.h"

namespace {

constexpr int DE_WAVES = 4;

template <typename T>
__device__ inline T de_wave_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline int de_wave_min(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ inline int de_wave_max(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// preds, truth [B][S][N][F]; masks, burn [B][S + 1][N]; keep [B][N] or null; rows [B * N][4][S] (fp64); flags [B * N][2]
// (int32: 1 if the predicted steps are not contiguous; num).
__global__ void __launch_bounds__(64 * DE_WAVES)
k_de_track(const float* __restrict__ preds, const float* __restrict__ truth, int F, const float* __restrict__ masks,
           const float* __restrict__ burn, const float* __restrict__ scale, const float* __restrict__ offset,
           const float* __restrict__ keep, int error_norm, int n_tracks, int N, int S, double* __restrict__ rows,
           int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int track = (int)blockIdx.x * DE_WAVES + ((int)threadIdx.x >> 6);
    if (track >= n_tracks) return;                                   // whole waves leave; no barrier below
    const int b = track / N, j = track - b * N;
    const float* m = masks + (size_t)b * (S + 1) * N + j;            // stride N over time
    const float* bm = burn + (size_t)b * (S + 1) * N + j;
    double* row = rows + (size_t)track * 4 * S;
    // :52 a burn-in entry anywhere (frame 0 included), :55-58 the data set's non_linear_masks
    bool has_burn = false;
    for (int s = lane; s <= S; s += 64) has_burn |= bm[(size_t)s * N] != 0.0f;
    bool live = __ballot(has_burn) != 0ull;
    if (keep != nullptr && keep[track] == 0.0f) live = false;
    // pred_mask = (masks - burn_in_masks)[1:]  (:29): first non-zero step, last one, how many, their sum (:69-76)
    int first = S, last = -1, nnz = 0;
    double total = 0.0;
    for (int s = lane; s < S; s += 64) {
        const float pm = m[(size_t)(s + 1) * N] - bm[(size_t)(s + 1) * N];
        if (pm != 0.0f) { first = min(first, s); last = max(last, s); ++nnz; }
        total += (double)pm;
    }
    first = de_wave_min(first); last = de_wave_max(last); nnz = de_wave_sum(nnz); total = de_wave_sum(total);
    // the length of the result is the longest pred_mask sum of ANY track, skipped ones included (:41)
    const int len = max(0, min((int)total, S));                      // .sum().int()
    int num = 0, bad = 0;
    if (live && nnz > 0) {
        num = min(len, S - first);
        bad = last - first + 1 != nnz ? 1 : 0;
    }
    if (lane == 0) { flags[2 * (size_t)track] = bad; flags[2 * (size_t)track + 1] = len; }
    double sc[4], of[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) { sc[f] = (double)scale[f]; of[f] = (double)offset[f]; }
    for (int h = lane; h < S; h += 64) {
        double e_all = 0.0, e_pos = 0.0, e_vel = 0.0, cnt = 0.0;
        if (h < num) {
            const int s = first + h;
            const double pm = (double)(m[(size_t)(s + 1) * N] - bm[(size_t)(s + 1) * N]);
            const float* p = preds + (((size_t)b * S + s) * N + j) * F;
            const float* g = truth + (((size_t)b * S + s) * N + j) * F;
            double d2[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double d = (sc[f] * (double)p[f] + of[f]) - (sc[f] * (double)g[f] + of[f]);
                d2[f] = d * d;
            }
            // multiplied by the mask, not selected by it (:60-68): inside a track with a gap the mask is 0 and a NaN
            // prediction there stays NaN, as in the reference
            e_all = (d2[0] + d2[1] + d2[2] + d2[3]) * 0.25 * pm;
            e_pos = (error_norm ? sqrt(d2[0] + d2[1]) : (d2[0] + d2[1]) * 0.5) * pm;
            e_vel = (error_norm ? sqrt(d2[2] + d2[3]) : (d2[2] + d2[3]) * 0.5) * pm;
            cnt = pm;
        }
        row[h] = e_all; row[(size_t)S + h] = e_pos; row[2 * (size_t)S + h] = e_vel; row[3 * (size_t)S + h] = cnt;
    }
}

// column c < 3 S: sums[c] += sum over tracks of rows[track][c];  3 S <= c < 4 S: counts[c - 3 S];  c == 4 S: stats.
__global__ void __launch_bounds__(256)
k_de_reduce(const double* __restrict__ rows, const int* __restrict__ flags, int n_tracks, int S,
            double* __restrict__ sums, double* __restrict__ counts, int64_t* __restrict__ stats) {
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c < 4 * S) {
        double acc = 0.0;
        for (int tr = 0; tr < n_tracks; ++tr) acc += rows[(size_t)tr * 4 * S + c];
        if (c < 3 * S) sums[c] += acc; else counts[c - 3 * S] += acc;
    } else if (c == 4 * S) {
        int64_t bad = 0, longest = 0;
        for (int tr = 0; tr < n_tracks; ++tr) {
            bad += flags[2 * (size_t)tr];
            longest = max(longest, (int64_t)flags[2 * (size_t)tr + 1]);
        }
        stats[0] += bad;
        stats[1] = max(stats[1], longest);
    }
}

}  // namespace
