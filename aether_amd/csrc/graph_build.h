// graph_build.h -- the graph view by a counting sort (aether_graph_build_counting, host_graph_build.inc).
//
// Receivers and senders are integers below n_nodes, so the two stable sorts of aether_graph_build are counting sorts:
//   k_gb_zero    clears the counters;
//   k_gb_count   one pass over the edges: range check, receiver and sender histograms (the value an edge's atomic
//                returns is its slot inside its receiver's / sender's list), crossing-edge difference array;
//   k_gb_scan    one workgroup: rowptr, srowptr (exclusive sums of the histograms) and cross (inclusive sum);
//   k_gb_place   perm[rowptr[r] + slot] = edge -- every in-edge list complete, in arrival order;
//   k_gb_recv    one wave per receiver: its list into ascending edge id (= the stable sort), recv_s, send_s, and the
//                sorted position of every edge into its sender's list;
//   k_gb_send    one wave per sender: its list into ascending sorted position; the tile table gsel on further waves.
// A list is ordered in LDS by counting, for every element, the smaller ones: the order of the result is a function of
// (key, value) alone, whatever order the atomics arrived in.  Integers only.  No kernel reads its grid or block size.
#pragma once
#include "fused_graph.h"

namespace {

constexpr int GB_CAP = 1024;              // longest in- or out-edge list ordered in LDS (config 5: 1,023); above: fallback
constexpr int GB_SCAN_THREADS = 1024;     // k_gb_scan: one workgroup, GB_SCAN_ITEMS counters per thread and round
constexpr int GB_SCAN_ITEMS = 4;
constexpr int64_t GB_SCAN_MAX = 1 << 20;  // counters (n_nodes + 1) one workgroup scans (config 5: 262,145); above: fallback

__global__ void __launch_bounds__(256)
k_gb_zero(int32_t* __restrict__ rowptr, int32_t* __restrict__ srowptr, int32_t* __restrict__ diff,
          int32_t* __restrict__ flag, int64_t n_nodes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n_nodes) { rowptr[i] = 0; srowptr[i] = 0; }
    if (i <= n_nodes + 1) diff[i] = 0;
    if (i < 4) flag[i] = 0;               // [0] bad index, [1] longest list
}

// An index outside [0, n_nodes) sets the flag and counts as node 0 (here and in the kernels below alike, so that every
// list is as long as its counter says and nothing is read or written out of range before the host has seen the flag).
// Crossing edges as in k_graph_cross.
__global__ void __launch_bounds__(256)
k_gb_count(const int64_t* __restrict__ send, const int64_t* __restrict__ recv, int64_t n_edges, int64_t n_nodes,
           int32_t* __restrict__ cnt_r, int32_t* __restrict__ cnt_s, int32_t* __restrict__ diff,
           int32_t* __restrict__ slot_r, int32_t* __restrict__ slot_s, int32_t* __restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_edges) return;
    int64_t s = send[k], r = recv[k];
    const bool bad_s = s < 0 || s >= n_nodes, bad_r = r < 0 || r >= n_nodes;
    if (bad_s || bad_r) {
        atomicOr(flag, 1);
    } else if (s != r) {
        const int64_t a = s < r ? s : r, b = s < r ? r : s;
        atomicAdd(diff + a + 1, 1);
        atomicAdd(diff + b + 1, -1);
    }
    if (bad_s) s = 0;
    if (bad_r) r = 0;
    slot_r[k] = atomicAdd(cnt_r + r, 1);
    slot_s[k] = atomicAdd(cnt_s + s, 1);
}

// rowptr / srowptr: counters in, exclusive sums out, in place; cross = inclusive sum of diff; diff then holds a copy of
// rowptr, next to cross and flag, so that everything the host reads comes back in one copy.  n = n_nodes + 1 counters.
__global__ void __launch_bounds__(GB_SCAN_THREADS)
k_gb_scan(int32_t* __restrict__ rowptr, int32_t* __restrict__ srowptr, int32_t* __restrict__ diff,
          int32_t* __restrict__ cross, int n, int32_t* __restrict__ flag) {
    __shared__ int wtot[3][GB_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry_a = 0, carry_b = 0, carry_d = 0, longest = 0;
    for (int base = 0; base < n; base += GB_SCAN_THREADS * GB_SCAN_ITEMS) {
        const int i0 = base + tid * GB_SCAN_ITEMS;
        int a[GB_SCAN_ITEMS], b[GB_SCAN_ITEMS], d[GB_SCAN_ITEMS];
        int sa = 0, sb = 0, sd = 0;
#pragma unroll
        for (int j = 0; j < GB_SCAN_ITEMS; ++j) {
            const bool ok = i0 + j < n;
            a[j] = ok ? rowptr[i0 + j] : 0;
            b[j] = ok ? srowptr[i0 + j] : 0;
            d[j] = ok ? diff[i0 + j] : 0;
            sa += a[j]; sb += b[j]; sd += d[j];
            longest = max(longest, max(a[j], b[j]));
        }
        int ia = sa, ib = sb, id = sd;        // inclusive over the lanes of the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int ta = __shfl_up(ia, o), tb = __shfl_up(ib, o), td = __shfl_up(id, o);
            if (lane >= o) { ia += ta; ib += tb; id += td; }
        }
        if (lane == 63) { wtot[0][wave] = ia; wtot[1][wave] = ib; wtot[2][wave] = id; }
        __syncthreads();
        int ra = carry_a + ia - sa, rb = carry_b + ib - sb, rd = carry_d + id - sd;    // sums in front of this thread
        for (int w = 0; w < GB_SCAN_THREADS / 64; ++w) {
            const int ta = wtot[0][w], tb = wtot[1][w], td = wtot[2][w];
            if (w < wave) { ra += ta; rb += tb; rd += td; }
            carry_a += ta; carry_b += tb; carry_d += td;
        }
#pragma unroll
        for (int j = 0; j < GB_SCAN_ITEMS; ++j) {
            if (i0 + j < n) {
                rd += d[j];
                rowptr[i0 + j] = ra; diff[i0 + j] = ra; srowptr[i0 + j] = rb; cross[i0 + j] = rd;
                ra += a[j]; rb += b[j];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) longest = max(longest, __shfl_xor(longest, o));
    if (lane == 0) atomicMax(flag + 1, longest);
}

__global__ void __launch_bounds__(256)
k_gb_place(const int64_t* __restrict__ recv, int64_t n_edges, int64_t n_nodes, const int32_t* __restrict__ rowptr,
           const int32_t* __restrict__ slot_r, int32_t* __restrict__ perm) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_edges) return;
    int64_t r = recv[k];
    if (r < 0 || r >= n_nodes) r = 0;
    perm[rowptr[r] + slot_r[k]] = (int32_t)k;
}

// One wave: the L <= GB_CAP distinct values src[0..L) in ascending order into out[0..L) (seg, out: LDS, GB_CAP ints each).
// The rank of a value is the number of smaller ones; a lane ranks up to four values per walk over the list.
__device__ inline void gb_sort_list(const int32_t* src, int L, int* seg, int* out, int lane) {
    for (int i = lane; i < L; i += 64) seg[i] = src[i];
    __syncthreads();
    if (L <= 64) {
        const int v = lane < L ? seg[lane] : 0;
        int rank = 0;
        for (int j = 0; j < L; ++j) rank += seg[j] < v ? 1 : 0;
        if (lane < L) out[rank] = v;
    } else {
        for (int i0 = 0; i0 < L; i0 += 256) {
            int v[4], rank[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + 64 * u + lane;
                v[u] = i < L ? seg[i] : 0;
                rank[u] = 0;
            }
            for (int j = 0; j < L; ++j) {
                const int x = seg[j];
#pragma unroll
                for (int u = 0; u < 4; ++u) rank[u] += x < v[u] ? 1 : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + 64 * u + lane < L) out[rank[u]] = v[u];
        }
    }
    __syncthreads();
}

// Workgroup (one wave) r: the in-edges of receiver r.  slot_s[edge]: the edge's slot in its sender's list (k_gb_count).
__global__ void __launch_bounds__(64)
k_gb_recv(const int64_t* __restrict__ send, int64_t n_nodes, const int32_t* __restrict__ rowptr,
          const int32_t* __restrict__ srowptr, const int32_t* __restrict__ slot_s, int32_t* __restrict__ perm,
          int32_t* __restrict__ recv_s, int32_t* __restrict__ send_s, int32_t* __restrict__ sperm) {
    __shared__ int seg[GB_CAP], out[GB_CAP];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int b = rowptr[r], L = rowptr[r + 1] - b;
    if (L <= 0 || L > GB_CAP) return;          // longer: the host falls back to aether_graph_build
    gb_sort_list(perm + b, L, seg, out, lane);
    for (int i = lane; i < L; i += 64) {
        const int e = out[i], pos = b + i;
        int64_t s = send[e];
        if (s < 0 || s >= n_nodes) s = 0;
        perm[pos] = e;
        recv_s[pos] = r;
        send_s[pos] = (int32_t)s;
        sperm[srowptr[s] + slot_s[e]] = pos;
    }
}

// Workgroups [0, n_nodes): the out-edges of one sender each (sorted positions, ascending).  The workgroups behind
// them: one tile of the streamed kernels' tile table each (fused_graph.h, graph_gtile).
__global__ void __launch_bounds__(64)
k_gb_send(int n_nodes, const int32_t* __restrict__ srowptr, int32_t* __restrict__ sperm,
          const int32_t* __restrict__ recv_s, int64_t n_edges, uint32_t* __restrict__ gsel) {
    __shared__ int seg[GB_CAP], out[GB_CAP];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_nodes) {
        graph_gtile(recv_s, n_edges, gsel, (int64_t)blockIdx.x - n_nodes, lane);
        return;
    }
    const int s = blockIdx.x;
    const int b = srowptr[s], L = srowptr[s + 1] - b;
    if (L <= 0 || L > GB_CAP) return;
    gb_sort_list(sperm + b, L, seg, out, lane);
    for (int i = lane; i < L; i += 64) sperm[b + i] = out[i];
}

}  // namespace
