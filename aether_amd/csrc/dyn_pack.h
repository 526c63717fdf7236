// Scene pack of the variable-N (inD) family: what the data set of the reference builds on the host
// per scene and per frame, for a whole batch of scenes in two launches:
//   node_inds                 experiments/ind/single_ind_data.py:82     (mask[step].nonzero()[:, -1])
//   graph_send / graph_recv   get_knn_graph_info, :186-211              (kNN graph of the frame's positions)
//   edge2node                 :213-215                                  ((tmp_inds == recv).nonzero()[:, 1].view(-1, k))
// k_dp_count: one workgroup per step counts the present objects of its (at most 256) scenes and scans them: every scene's
// offset into the step's concatenated arrays.  k_dp_build: one workgroup per (step, scene) compacts the present rows, runs
// the neighbour search of k_knn_select (knn_nearest: the edges aether_knn_edges lists) and sorts
// the scene's edge ids by receiver with a stable counting sort, all in LDS.  No atomics on anything a result depends on
// (the receiver histogram is an integer count), so the same input gives the same bytes.
#pragma once
#include "common.h"
#include "knn.h"

namespace {

constexpr int DP_MAX_SCENES = 256;
constexpr int DP_MAX_OBJECTS = 512;            // positions, masks, two counters per row and Nmax * k neighbour ids in LDS
constexpr int DP_THREADS = 256;

// counts[t][b] = present objects of scene b at step t (as found: 1 is reported to the host, which refuses it);
// node_off / edge_off[t][b]: where the scene's node_inds / edges start within step t's arrays.
__global__ void __launch_bounds__(DP_THREADS)
k_dp_count(const float* __restrict__ masks, int B, int N, int k, int* __restrict__ counts, int* __restrict__ node_off,
           int* __restrict__ edge_off) {
    __shared__ int nn[DP_MAX_SCENES], ne[DP_MAX_SCENES], part[DP_THREADS];
    const int t = blockIdx.x, b = threadIdx.x;
    int n = 0;
    if (b < B) {
        const float* m = masks + ((size_t)t * B + b) * N;
        for (int j = 0; j < N; ++j) n += m[j] != 0.0f ? 1 : 0;
        counts[(size_t)t * B + b] = n;
    }
    const int used = n >= 2 ? n : 0;
    nn[b] = used;
    ne[b] = used * min(k, used - 1);
    __syncthreads();
    block_exclusive_scan(nn, DP_MAX_SCENES, part, DP_THREADS);
    block_exclusive_scan(ne, DP_MAX_SCENES, part, DP_THREADS);
    if (b < B) {
        node_off[(size_t)t * B + b] = nn[b];
        edge_off[(size_t)t * B + b] = ne[b];
    }
}

// One workgroup per (step, scene).  x: [S][N][4] rows (position in the first two columns), masks [S][N], S = steps * B.
// node_inds [steps][node_stride], send / recv / e2n [steps][edge_stride].
__global__ void __launch_bounds__(DP_THREADS)
k_dp_build(const float* __restrict__ x, const float* __restrict__ masks, int B, int N, int k,
           const int* __restrict__ node_off, const int* __restrict__ edge_off, int64_t* __restrict__ node_inds,
           int64_t* __restrict__ send, int64_t* __restrict__ recv, int64_t* __restrict__ e2n, int64_t node_stride,
           int64_t edge_stride) {
    extern __shared__ float dp_lds[];
    float* px = dp_lds;                               // [N]
    float* py = px + N;                               // [N]
    float* pm = py + N;                               // [N]
    int* cidx = reinterpret_cast<int*>(pm + N);       // [N] compacted index of a present row
    int* start = cidx + N;                            // [N] in-edges per receiver, then their exclusive scan
    int* part = start + N;                            // [DP_THREADS]
    int* nbr = part + DP_THREADS;                     // [n][deg] neighbours in compacted numbering = recv of edge i * deg + p
    const int s = blockIdx.x, t = s / B, tid = threadIdx.x;
    for (int j = tid; j < N; j += DP_THREADS) {
        const float* row = x + ((size_t)s * N + j) * 4;
        px[j] = row[0]; py[j] = row[1];
        const float m = masks[(size_t)s * N + j];
        pm[j] = m;
        cidx[j] = m != 0.0f ? 1 : 0;
        start[j] = 0;
    }
    __syncthreads();
    const int n = block_exclusive_scan(cidx, N, part, DP_THREADS);
    if (n < 2) return;                                // nobody (or one object, which the host refuses): nothing to write
    const int deg = min(k, n - 1);
    const size_t nb = (size_t)t * node_stride + node_off[s], eb = (size_t)t * edge_stride + edge_off[s];
    for (int i = tid; i < N; i += DP_THREADS) {
        if (pm[i] == 0.0f) continue;
        node_inds[nb + cidx[i]] = i;
        int bi[KNN_MAX_K];
        knn_nearest(px, py, pm, N, i, bi);            // k_knn_select's search
        // a NaN position is nearer to nobody: fewer than deg neighbours found.  The edge keeps a valid receiver (the
        // object itself) so that nothing downstream indexes past the scene.
#pragma unroll
        for (int p = 0; p < KNN_MAX_K; ++p)
            if (p < deg) {
                const int r = bi[p] >= 0 ? cidx[bi[p]] : cidx[i];
                nbr[cidx[i] * deg + p] = r;
                atomicAdd(&start[r], 1);              // integer count in LDS: the order of the adds does not matter
            }
    }
    __syncthreads();
    block_exclusive_scan(start, n, part, DP_THREADS);
    const int E = n * deg;
    for (int e = tid; e < E; e += DP_THREADS) {
        send[eb + e] = e / deg;
        recv[eb + e] = nbr[e];
    }
    // stable counting sort by receiver: receiver r collects its in-edges in edge order (argsort(recv, stable=True))
    for (int r = tid; r < n; r += DP_THREADS) {
        int at = start[r];
        for (int e = 0; e < E; ++e)
            if (nbr[e] == r) e2n[eb + at++] = e;
    }
}

inline size_t dp_build_lds_bytes(int N, int k) { return ((size_t)5 * N + DP_THREADS + (size_t)N * k) * 4; }

}  // namespace
