// fused_graph.h -- the graph view's workgroup and tile records and the kernels that build them: k_fused / k_fused_bwd
// walk FusedWG, lorder / ledge / nrange and trec; the streamed edge kernels read gsel (graph_gtile; graph_build.h writes it too).
#pragma once
#include "fused_layout.h"

namespace {

// One workgroup's share of a group: it sees nodes [vb, ve) (whole graphs: every sender of its edges)
// and owns nodes [nb, ne) -- their in-edges, their node updates, their outputs.  Unsplit: own = visible.
// Split (two workgroups per group, when there are fewer groups than half the CUs): the partner owns
// the rest and the two exchange their P_s rows once per layer through global memory.
// A workgroup walks its m in-edges in a LOCAL order (lorder[eb + local] = offset into the receiver-sorted
// range): first the `na` edges whose sender it owns, then the edges from the partner's nodes, each run
// receiver-sorted (unsplit: na = m, the identity).  Tiles of the first run need nothing from the partner, so
// the forward starts with them while the partner's rows are in flight -- and the backward starts with the
// second run, whose sender-side sums the partner waits for.
// goff: the view's granule block (12-wave kernel, tagged-granule hand-off): its byte offset from the hand-off flags, 0 when
// the view has none; the same in every workgroup of a view.
struct FusedWG { int vb, ve, nb, ne, tile0, partner, na, eb, m, goff, pad2, pad3; };   // eb, m: first in-edge (sorted position) and in-edge count of [nb, ne)
struct FusedTile { int wg, t; };             // workgroup descriptor index, tile index within the workgroup

// Local edge order of every workgroup (one block per workgroup; m <= FUSED_MAX_EDGES <= blockDim.x) and the
// local index ranges of every own node's in-edges in the two runs: nrange[node] = {a_beg, a_end, b_beg, b_end}.
__global__ void __launch_bounds__(512)
k_graph_lorder(FusedWG* __restrict__ wgdesc, const int32_t* __restrict__ send_s, const int32_t* __restrict__ recv_s,
               const int32_t* __restrict__ perm, const int32_t* __restrict__ rowptr, int32_t* __restrict__ lorder,
               int4* __restrict__ ledge, int32_t* __restrict__ nrange) {
    __shared__ int wsum[2][8];
    __shared__ int cnt_a[FUSED_MAX_NODES + 1], cnt_b[FUSED_MAX_NODES + 1];
    const FusedWG wg = wgdesc[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int eb = rowptr[wg.nb], m = rowptr[wg.ne] - eb, n = wg.ne - wg.nb;
    const bool valid = tid < m;
    const bool split = wg.partner >= 0;
    const int snd = valid ? send_s[eb + tid] : -1;
    const bool own = valid && (!split || (snd >= wg.nb && snd < wg.ne));
    const bool oth = valid && !own;
    const unsigned long long bo = __ballot(own), bt = __ballot(oth);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (lane == 0) { wsum[0][wave] = __popcll(bo); wsum[1][wave] = __popcll(bt); }
    if (tid <= FUSED_MAX_NODES) { cnt_a[tid] = 0; cnt_b[tid] = 0; }
    __syncthreads();
    int base_o = 0, base_t = 0, na = 0;
    for (int w = 0; w < 8; ++w) {
        if (w < wave) { base_o += wsum[0][w]; base_t += wsum[1][w]; }
        na += wsum[0][w];
    }
    // ledge: the same order with everything the forward kernel's feature phase looks up per edge in one 16-byte record
    // {sorted position, sender, receiver, original edge}: one round trip instead of three dependent ones (k_fused, P2)
    if (valid) {
        const int pos = own ? base_o + __popcll(bo & below) : na + base_t + __popcll(bt & below);
        lorder[eb + pos] = tid;
        ledge[eb + pos] = make_int4(eb + tid, snd, recv_s[eb + tid], perm[eb + tid]);
    }
    if (tid == 0) wgdesc[blockIdx.x].na = na;
    // per-node run lengths (thread per own node, a handful of edges each), then a serial prefix
    if (tid < n) {
        int ca = 0, cb = 0;
        for (int k = rowptr[wg.nb + tid]; k < rowptr[wg.nb + tid + 1]; ++k) {
            const int sd = send_s[k];
            if (!split || (sd >= wg.nb && sd < wg.ne)) ++ca; else ++cb;
        }
        cnt_a[tid] = ca; cnt_b[tid] = cb;
    }
    __syncthreads();
    if (tid == 0) {
        int pa = 0, pb = na;
        for (int s = 0; s < n; ++s) {
            int32_t* o = nrange + 4 * (int64_t)(wg.nb + s);
            o[0] = pa; o[1] = pa + cnt_a[s]; o[2] = pb; o[3] = pb + cnt_b[s];
            pa += cnt_a[s]; pb += cnt_b[s];
        }
    }
}

// Per-tile structure of a workgroup's edge list in LOCAL order, built once with the graph: one record of
// FUSED_TREC dwords per tile, the same for all 64 lanes of the tile's wave (k_fused keeps it in scalar registers).
// A segment = consecutive rows with one receiver inside one run; its partial row is receiver + tile (+ n in the
// second run), at most 2 * 32 + 15 < 256.
//   dword 0      bit k: row k is the last row of its segment (padding rows end nothing)
//   dword 1      number of segments
//   dwords 2-5   partial row of segment s in byte s (segment order = row order), 0xFF behind the last segment
//   dwords 6, 7  zero
constexpr int FUSED_TREC = 8;
__global__ void __launch_bounds__(64)
k_graph_tiles(const FusedTile* __restrict__ tdesc, const FusedWG* __restrict__ wgdesc,
              const int32_t* __restrict__ recv_s, const int32_t* __restrict__ rowptr,
              const int32_t* __restrict__ lorder, uint32_t* __restrict__ trec) {
    const FusedTile T = tdesc[blockIdx.x];
    const FusedWG wg = wgdesc[T.wg];
    const int eb = rowptr[wg.nb], m = rowptr[wg.ne] - eb, n = wg.ne - wg.nb;
    const int na = wg.na;
    const int lane = threadIdx.x, i = lane & 15, q = lane >> 4;
    const int local = 16 * T.t + i;
    const bool valid = local < m;
    const int rcv = valid ? recv_s[eb + lorder[eb + local]] - wg.nb : -1;
    // row i ends its segment when the next row is padding, has another receiver or opens the second run
    const int next = __shfl_down(rcv, 1, 16);
    const bool ends = valid && (i == 15 || next != rcv || local + 1 == na);
    const unsigned emask = (unsigned)__ballot(q == 0 && ends) & 0xFFFFu;
    const int second = (wg.partner >= 0 && local >= na) ? n : 0;
    const int myrow = rcv + T.t + second;                 // (meaningful on rows that end a segment)
    // lane j < FUSED_TREC assembles dword j; the row lookups run on all lanes (shuffles)
    const int j = lane & (FUSED_TREC - 1);
    unsigned w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int seg = 4 * (j - 2) + b;                  // dwords 2-5: segments 0..15
        unsigned mm = emask;
        for (int t = 0; t < seg && mm != 0; ++t) mm &= mm - 1;
        const bool exists = seg >= 0 && seg < 16 && mm != 0;
        const int k = mm != 0 ? __ffs(mm) - 1 : 0;
        const int row = __shfl(myrow, k);
        w |= (exists ? (unsigned)row & 0xFFu : 0xFFu) << (8 * b);
    }
    if (j == 0) w = emask;
    if (j == 1) w = (unsigned)__popc(emask);
    if (j >= 6) w = 0;
    if (lane < FUSED_TREC) trec[(size_t)blockIdx.x * FUSED_TREC + lane] = w;
}

// The same structure for the whole receiver-sorted edge list (tile t = sorted positions 16t..16t+15),
// one word per lane, for the streamed edge kernels (streamed.h::tile_receiver_sums):
// bits 0-3 segment-matrix column; per result register r4: first row of segment 4q+r4 (4 bits), valid (1 bit).
__device__ inline void graph_gtile(const int32_t* __restrict__ recv_s, int64_t n_edges, uint32_t* __restrict__ gsel,
                                   int64_t tile, int lane) {
    const int i = lane & 15, q = lane >> 4;
    const int64_t k = tile * 16 + i;
    const bool valid = k < n_edges;
    const int rcv = valid ? recv_s[k] : -1;
    const int prev = __shfl_up(rcv, 1, 16);
    const unsigned smask = (unsigned)__ballot(q == 0 && i > 0 && rcv != prev) & 0xFFFFu;
    const unsigned vmask = (unsigned)__ballot(q == 0 && valid) & 0xFFFFu;
    unsigned w = 0;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        const int edge = 4 * s4 + q;
        const int seg_of_edge = __popc(smask & ((2u << edge) - 1u));
        if (((vmask >> edge) & 1u) && seg_of_edge == i) w |= 1u << s4;
    }
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
        const int seg = 4 * q + r4;
        unsigned mm = smask;
        int s0 = 0;
        bool exists = true;
        for (int t = 0; t < seg; ++t) {
            if (mm == 0) { exists = false; break; }
            s0 = __ffs(mm) - 1;
            mm &= mm - 1;
        }
        const unsigned ok = (exists && ((vmask >> s0) & 1u)) ? 16u : 0u;
        w |= ((unsigned)s0 | ok) << (4 + 5 * r4);
    }
    gsel[(size_t)tile * 64 + lane] = w;
}

__global__ void __launch_bounds__(64)
k_graph_gtiles(const int32_t* __restrict__ recv_s, int64_t n_edges, uint32_t* __restrict__ gsel) {
    graph_gtile(recv_s, n_edges, gsel, (int64_t)blockIdx.x, threadIdx.x);
}

}  // namespace
