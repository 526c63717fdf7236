// fused.h -- the whole Aether step for one *group* of small graphs in ONE launch.
//
// A group is a contiguous node range [nb, ne) whose in-edges all have senders inside the range
// (one or several whole graphs; built by aether_graph_build), with at most FUSED_MAX_NODES nodes
// and FUSED_MAX_EDGES edges.  One workgroup of NW waves owns the group from the field query to the
// output; nothing but the inputs, the weights and the D output floats per node touches HBM:
//   * every edge message tile (16 edges x 64) stays in the owning wave's registers across the four
//     layers (it is the next layer's MFMA B operand as it stands);
//   * node state (x, n, P_s, P_r) and the per-layer edge weights live in LDS (padded rows);
//   * the mean over in-edges needs no workgroup barrier inside a layer: the wave parks its tile in
//     16 private LDS rows and reads it back by columns -- lane L adds column L's 16 values in row
//     order (16 vector adds per tile) and stores the running sum after the last row of each receiver
//     segment; which rows end a segment, and where their sums go, is one record per tile built with
//     the graph (k_graph_tiles), held in scalar registers: the tests and branches run on the scalar
//     unit.  One partial row per (receiver, tile) goes to LDS and the node phase adds a node's
//     partial rows in tile order.  Fixed order everywhere: deterministic, no atomics.  (Until round 8
//     the sums were 16 fp32 MFMAs with the tile's 0/1 segment matrix: 512 cycles of vector-ALU time
//     per tile, most of it multiplying zeros; a masked DPP butterfly on the accumulator layout was
//     measured 2-4x slower than that in round 1, before the staging rows existed.)
//   * node-level GEMMs are split along their output rows over the waves; their weights come from L2
//     in MFMA fragment shape (each is used once per group and layer), all issued before the barrier
//     that ends the edge phase.
//   * waves per workgroup: 8, a wave owning up to ROUNDS edge tiles per layer (tile = NW * round + wave) -- or, for
//     inference on workgroups of 9-12 tiles and one node tile (every half of a split N = 17..20 graph), 12 with one
//     tile each (k_fused<D, 12, 1, false>): three waves per SIMD hide each other's LDS round trips and MFMA / SiLU
//     chains, where four of eight waves ran a second tile alone on their SIMD.  Same tiles, records, partial rows and
//     hand-off; the node phase's row blocks are dealt to the twelve waves (wf_h / wf_l below), the arithmetic is the
//     8-wave kernel's and the outputs are bit-identical.
// References: see common.h / streamed.h; the arithmetic per stage is identical to the streamed path.
// This file: FusedDebug, the stamp macros of the diagnostic build, the kernel.  LDS layout, weight images and constants
// blocks: fused_layout.h; the graph view's records and their kernels: fused_graph.h; the granule hand-off: fused_handoff.h.
#pragma once
#include "common.h"
#include "fused_layout.h"
#include "fused_graph.h"
#include "fused_handoff.h"

namespace {

// Optional global copies of the intermediates (same layout as the streamed path's workspace), so
// that the parity tests and (later) the backward can read them.
struct FusedDebug {
    float* nodeinfo; float* x[5]; float* e[4];
    float* n[4]; float* ps[3]; float* pr[3]; float* feat;     // saved for the backward
    int* flags;             // [workgroups] split mode: layer whose P_s rows this workgroup has published (lives in the
                            // graph buffer: zero when no launch is in flight, every launch re-arms what it consumed)
    int* errword;           // host-mapped word: set when a bounded wait on the partner workgroup gave up
    const float* wimg;      // split weight images (k_split_weights); used by the split-GEMM variants
    float* stamps;          // [groups][FUSED_STAMPS] diagnostic build only
    StepExtras step;        // rollout: derived edge attributes, next velocity
};
constexpr int FUSED_STAMPS = 512;

// In-kernel phase stamps: only in the diagnostic build (-DAETHER_FUSED_STAMPS).  Thread 0 of each
// workgroup records the 100 MHz wall clock (microseconds since entry) at phase boundaries; lane 0 of
// each wave records shader-clock cycles around the pieces of its layer-2 tiles.  The stamps go to a
// buffer nothing else reads.
#ifdef AETHER_FUSED_STAMPS
#define FUSED_STAMP(id)                                                                          \
    do {                                                                                         \
        if (tid == 0 && blockIdx.x < 4096)                                                       \
            dbg.stamps[blockIdx.x * FUSED_STAMPS + (id)] = (float)(wall_clock64() - t_entry) * 0.01f; \
    } while (0)
#define FUSED_WSTAMP(layer_, r_, k_)                                                              \
    do {                                                                                         \
        if ((layer_) == 2 && lane == 0 && blockIdx.x < 4096 && wave < 16)                        \
            dbg.stamps[blockIdx.x * FUSED_STAMPS + 64 + wave * 24 + (r_) * 8 + (k_)] =            \
                (float)(__builtin_amdgcn_s_memtime() - c_entry);                                 \
    } while (0)
// (k_ = 8, 9 with r_ = 0: begin and end of the early W_e e product, in the slots of the round the 12-wave kernels do not have)
// one more stamp per (wave, round), behind the 12 x 24 slots above: the partner's rows are there (front of the late add)
#define FUSED_WSTAMP_ROWS(layer_, r_)                                                             \
    do {                                                                                         \
        if ((layer_) == 2 && lane == 0 && blockIdx.x < 4096 && wave < 16)                        \
            dbg.stamps[blockIdx.x * FUSED_STAMPS + 352 + wave * 4 + (r_)] =                       \
                (float)(__builtin_amdgcn_s_memtime() - c_entry);                                 \
    } while (0)
// the field wave's pieces (wave 0, shader-clock cycles since entry), behind the slots above: 0 first vector load issued,
// 1 the block's vmcnt(0) passed, 2 last MFMA of the field net retired, 3 frame stored, 4 x0 stored.  `dep_`: a vector
// register the stamp waits for (the wave issues in order: the move stalls until the value is there).
// 12-wave kernels: 3 = the force stored (the frame is the frame wave's), 4 not written; FUSED_PSTAMP_W, wave `w_`: 5 the
// frame wave of node tile 0 has its inputs, 6 its frames stored; 7 x0 wave of row block 0 behind the P1 barrier, 8 its
// rows of x0 stored.
#define FUSED_PSTAMP_W(w_, k_, dep_)                                                              \
    do {                                                                                         \
        asm volatile("v_mov_b32 %0, %0" : "+v"(dep_));                                           \
        if (wave == (w_) && lane == 0 && blockIdx.x < 4096)                                      \
            dbg.stamps[blockIdx.x * FUSED_STAMPS + 400 + (k_)] =                                  \
                (float)(__builtin_amdgcn_s_memtime() - c_entry);                                 \
    } while (0)
#define FUSED_PSTAMP(k_, dep_) FUSED_PSTAMP_W(0, k_, dep_)
#else
#define FUSED_STAMP(id)
#define FUSED_WSTAMP(layer_, r_, k_)
#define FUSED_WSTAMP_ROWS(layer_, r_)
#define FUSED_PSTAMP(k_, dep_)
#define FUSED_PSTAMP_W(w_, k_, dep_)
#endif

template <int D, int NW, int ROUNDS, bool KEEP, bool GRAN = false>
__global__ void __launch_bounds__(NW * 64)
k_fused(AetherParams P, const float* __restrict__ x, const float* __restrict__ vel,
        const float* __restrict__ charges, const float* __restrict__ edge_attr_orig,
        const int32_t* __restrict__ perm, const int32_t* __restrict__ send_s,
        const int32_t* __restrict__ recv_s, const int32_t* __restrict__ rowptr,
        const FusedWG* __restrict__ wgdesc, const uint32_t* __restrict__ trec, const int4* __restrict__ ledge,
        const int32_t* __restrict__ nrange, FusedDebug dbg, float* __restrict__ out) {
    constexpr bool keep = KEEP;      // inference build carries none of the save-for-backward stores
    using NI = NodeInfo<D>;
    using L = FusedLds<NW, ROUNDS>;
    constexpr int THREADS = NW * 64;
    constexpr int FIN = 2 * D + 16;
    // NW == 12 (ROUNDS == 1, inference): twelve waves with one edge tile each, for workgroups of 9-12 tiles and one node
    // tile (n <= 16: the host dispatches it only then); the node phase's roles are spread over the twelve waves and
    // share one set of fragment registers (wf_h / wf_l below, DESIGN.md 4.1 "Wave roles in the node phase").
    static_assert(NW == 8 || NW == 12, "waves 0-7 run the node phase; NW == 12 adds four waves that run step 3 (DESIGN.md 4.1)");
    static_assert(NW == 8 || (ROUNDS == 1 && !KEEP), "the 12-wave kernel owns one tile per wave and saves nothing for the backward");
    // GRAN (12 waves, split views): the own P_s rows go to the partner as tagged granules (fused_handoff.h) instead of rows +
    // flag.  An instantiation holds ONE of the two protocols -- with both, the scalar registers of the unused one pushed
    // three dozen others into vector-register lanes, read back at the top of every layer (+1.0 us per step).  Both
    // workgroups of a pair run the same launch, so the two protocols never meet.
    static_assert(!GRAN || NW == 12, "granules are the 12-wave kernel's hand-off");
    // The kernels that run workgroups of 9-16 tiles -- the 12-wave kernels and the two-tile 8-wave kernels, compared bit for
    // bit -- share one rule for the first Linear of layers 2-4: g = W_e e from +0.0f accumulators, then g + (P_r + P_s),
    // or (g + P_r) + P_s on an edge whose sender the partner owns (front_gemm / late_add below).  g needs nothing but
    // the message tile, so the 12-wave kernels (EARLY) compute it under the previous layer's node phase, where the
    // matrix pipe is idle, and keep it in the tile's registers: e[0] is dead behind the product.
    constexpr bool LATE = NW == 12 || ROUNDS == 2;
    constexpr bool EARLY = NW == 12;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wA = smem + L::WA;
    float* wB = smem + L::WB;
    const float* cblk = smem + L::CBLK;
    float* xbuf = smem + L::XBUF;
    float* nbuf = smem + L::NBUF;
    float* psb = smem + L::PS;
    float* prb = smem + L::PR;
    float* ninfo = smem + L::NINFO;
    float* part = smem + L::PART;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const FusedWG wg = wgdesc[blockIdx.x];
    const int vb = wg.vb, nv = wg.ve - wg.vb;            // visible nodes (slots of ninfo / psb)
    const int nb = wg.nb, ne = wg.ne;                    // own nodes (slots of xbuf / nbuf / prb / part)
    const int n = ne - nb, off = nb - vb;
    const int eb = wg.eb, m = wg.m;                      // (= rowptr[nb], rowptr[ne] - rowptr[nb]: kept with the descriptor)
    const int n_tiles = (m + 15) >> 4;
    const int na = wg.na;                                // edges [0, na) of the local order have own senders
    // An LDS-typed word: plain ds_write / ds_read.  (Through a generic volatile pointer every access was a flat_ instruction
    // with sc0 sc1 and a full vmcnt(0) drain -- two of them here, in front of wave 0's first loads.)  volatile: the spin in
    // wait_partner_rows re-reads the word in every iteration.
    typedef __attribute__((address_space(3))) volatile int lds_word;
    lds_word* arrived = (lds_word*)(smem + L::ARRIVED);
    if (tid == 0) { arrived[0] = 0; arrived[1] = 0; }    // ordered before any use by the prologue's barriers
#ifdef AETHER_FUSED_STAMPS
    const unsigned long long t_entry = wall_clock64();
    const unsigned long long c_entry = __builtin_amdgcn_s_memtime();
#endif
    FUSED_STAMP(0);

    // ---------------------------------------------------------------- P0: layer-1 weights, requested only
    // (images of W1 and W2, constants block 1); they land in LDS during the prologue, behind the field net.
    // A layer's two weight images and its constants block are copied global -> LDS by LDS-DMA, one 1 KiB fragment per wave
    // instruction (lane-linear in both places), no registers, no VALU; layer 1's image A is half a slot.  Block l goes to
    // slot l & 1: the other slot holds the block that the running layer still reads.  The caller waits (vmcnt) before the
    // barrier that precedes the first read.
    auto dma_images = [&](int layer_) {
        const int na_frag = layer_ == 1 ? 8 : 16, nw_frag = na_frag + 16;     // 1 KiB fragments: 2 terms x 4 (x 2)
        const int total = nw_frag + FUSED_CBLK / 256;
        // Fragment index and both offsets in scalar registers, selects instead of branches (with the wave index as a lane
        // value this was a divergent loop of ~40 instructions and a dozen exec-mask branches per fragment, on every
        // wave's critical path).  Image B follows image A in global memory as W2 follows W_e in LDS.
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        __builtin_assume(wv >= 0 && wv < NW);
        const int g_img = fused_wimg_offset(layer_, 0), g_cb = fused_cblk_offset(layer_);
        const int l_cb = L::CBLK + (layer_ & 1) * FUSED_CBLK;
        constexpr int MAXF = (32 + FUSED_CBLK / 256 + NW - 1) / NW;
#pragma unroll
        for (int j = 0; j < MAXF; ++j) {
            const int f = wv + NW * j;
            if (f < total) {
                const int img = f < na_frag ? f * 256 : FUSED_WIMG + (f - na_frag) * 256;    // offset in [image A | image B]
                const int soff = f < nw_frag ? g_img + img : g_cb + (f - nw_frag) * 256;
                const int doff = f < nw_frag ? L::WA + img : l_cb + (f - nw_frag) * 256;
                __builtin_amdgcn_global_load_lds(dbg.wimg + soff + lane * 4, (__attribute__((address_space(3))) void*)(smem + doff), 16, 0, 0);
            }
        }
    };
    // 12 waves (EARLY): the tiles of layers 2-4 never read wA -- their W_e e product ran under the previous node phase -- so
    // wA is dead from the closing barrier of node phase l - 1 to the products of node phase l, and so is constants slot
    // (l + 1) & 1.  W_e(l + 1) and constants block l + 1 are therefore copied a whole edge phase ahead (dma_ahead: 19
    // fragments, dealt round-robin to `nslots` waves, this wave being number `slot` of them or none, slot < 0), and only
    // W2(l + 1) is left for the node phase (dma_w2: 16 fragments on the four waves that are idle in step 2).  Layer 1's
    // image A, which the tiles of layer 1 do read, goes to the P_s rows (L::W1A).
    // The copy instruction stands in an asm statement: as a builtin inside the layer loop's edge phase it is, to the
    // compiler's wait-count pass, an access that may return out of order with the LDS reads, and every counted lgkmcnt
    // wait of the tiles behind it becomes an lgkmcnt(0) (29 waits instead of 54 in the tile code, + 2.1 us per step).
    // Unseen, it only makes the compiler's counted vmcnt waits wait for more than they need: loads return in order.
    // The waits for the copy itself are written by hand where its fragments are first read.
    auto dma_frag = [&](int soff, int doff) {
        const float* src = dbg.wimg + soff + lane * 4;
        const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + doff);
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(src), "s"(dst) : "memory", "m0");
    };
    auto dma_ahead = [&](int layer_, int slot, int nslots) {
        const int g_img = fused_wimg_offset(layer_, 0), g_cb = fused_cblk_offset(layer_);
        const int l_cb = L::CBLK + (layer_ & 1) * FUSED_CBLK;
        constexpr int total = 16 + FUSED_CBLK / 256;
#pragma unroll
        for (int j = 0; j < (total + NW - 2) / (NW - 1); ++j) {
            const int f = slot + nslots * j;
            if (slot >= 0 && f < total) dma_frag(f < 16 ? g_img + f * 256 : g_cb + (f - 16) * 256, f < 16 ? L::WA + f * 256 : l_cb + (f - 16) * 256);
        }
    };
    auto dma_w2 = [&](int layer_, int slot) {
        const int g_img = fused_wimg_offset(layer_, 1);
        constexpr int nw2 = NW > FUSED_W2DMA_WAVE0 ? NW - FUSED_W2DMA_WAVE0 : 1;
        static_assert(16 % nw2 == 0, "every wave of step 2's idle ones issues the same number of fragments");
#pragma unroll
        for (int j = 0; j < 16 / nw2; ++j) {
            const int f = slot + nw2 * j;
            dma_frag(g_img + f * 256, L::WB + f * 256);
        }
    };
    if constexpr (EARLY) {
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        __builtin_assume(wv >= 0 && wv < NW);
        constexpr int total = 8 + 16 + FUSED_CBLK / 256;      // W1 (half an image), W2(1), constants block 1 -> slot 1
#pragma unroll
        for (int j = 0; j < (total + NW - 1) / NW; ++j) {
            const int f = wv + NW * j;
            if (f < total)
                dma_frag(f < 8 ? fused_wimg_offset(1, 0) + f * 256 : f < 24 ? fused_wimg_offset(1, 1) + (f - 8) * 256 : fused_cblk_offset(1) + (f - 24) * 256,
                         f < 8 ? L::W1A + f * 256 : f < 24 ? L::WB + (f - 8) * 256 : L::CBLK + FUSED_CBLK + (f - 24) * 256);
        }
        // W_e(2) -> wA, block 2 -> slot 0: neither has been written yet in this launch
        dma_ahead(2, wv, NW);
    } else {
        dma_images(1);
    }
    FUSED_STAMP(1);

    // ---------------------------------------------------------------- edge indices of P2, requested during P1
    // P2 needs, per lane, dependent rounds of global loads before it can read a node record: in rounds 1 - 4 (first half)
    // row pointers -> local order -> sender / receiver / original edge -> edge attributes, issued in P2 (1.8 us per workgroup).
    // Now the descriptor carries the row pointers, the graph one 16-byte record per edge in local order (ledge,
    // k_graph_lorder), and every wave asks for its records and attributes during P1 -- only two of the eight waves work
    // there (<= 32 visible nodes), behind their own inputs.
    constexpr int FR = ROUNDS < 2 ? ROUNDS : 2;              // rounds of the first feature pass (lane >> 4)
    // NW == 12 (PACKED): the features are built by one wave per SIMD -- waves 0-3, lanes 0-47, edge 48 wave + lane, that is
    // row lane & 15 of tile 3 wave + (lane >> 4) -- and go into the OWNING wave's rows of L::FEAT (tile t belongs to wave t).
    // With every wave building its own 16 edges on a quarter of its lanes, the three waves of a SIMD ran the same
    // ~200-instruction chain one after the other: a wave64 instruction holds the SIMD's vector issue for four cycles
    // whatever its exec mask.  t_e, sl, rl and nr_rec stay per owner.
    constexpr bool PACKED = NW == 12;
    constexpr bool FIMG = NW == 12;      // the field wave's weight operands come as the prepared field image (P1)
    // NW == 12 (FRAMES): the field wave runs the field net and stores the force alone.  R and cv = R^T v need the velocity
    // only: wave FUSED_FRAME_WAVE0 + t builds them for visible node tile t while the field net runs (P1's else branch);
    // cf = R^T f is D * D multiply-adds that each reader does on its register copy of the record (P2's receiver record,
    // the x0 waves), so the record's CF words are not written and no wave waits for another inside P1.  x0 is first read in
    // step 1 of layer 1's node phase: waves FUSED_X0_WAVE0 .. + 3 compute it behind the P1 barrier, next to the feature build.
    constexpr bool FRAMES = NW == 12;
    f32x4 x0_acc = f32x4{0.f, 0.f, 0.f, 0.f}, x0_ar = f32x4{0.f, 0.f, 0.f, 0.f};   // FRAMES: an x0 wave's two chunks of the field image
    const int f_local = PACKED ? fused_packed_edge(wave, lane) : 16 * (NW * (lane >> 4) + wave) + (lane & 15);
    const bool f_have = (PACKED ? wave < FUSED_PACK_WAVES && lane < FUSED_PACK_LANES : lane < 16 * FR) && f_local < m;   // this lane builds the features of edge f_local
    int4 f_e = make_int4(0, 0, 0, 0);                        // {sorted position, sender, receiver, original edge}
    f32x2 f_ea = {0.0f, 0.0f};                               // its two edge attributes (rollout: q_i, q_j)
    int4 t_e[ROUNDS];                                        // per (round, lane i): the tile's edge i
    // The segment records of the wave's tiles (k_graph_tiles) are the same for all lanes: tile index from the wave index in
    // a scalar register (as dma_images), so they arrive by scalar loads and stay in scalar registers.  Requested here, in
    // code every wave runs: behind a branch on the wave index the compiler would treat them as per-lane values.
    unsigned seg_ends[ROUNDS];                               // bit k: row k is the last row of its segment
    unsigned seg_rows[ROUNDS][4];                            // partial rows of the segments, one byte each, in segment order
    {
        const int wv = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int stile = NW * r + wv;
            const uint32_t* rec = trec + (size_t)(wg.tile0 + (stile < n_tiles ? stile : 0)) * FUSED_TREC;   // (a wave without that tile reads record tile0: inside the table also for a workgroup without tiles -- GraphLayout::max_tiles counts two more per node than are ever built)
            seg_ends[r] = stile < n_tiles ? __builtin_amdgcn_readfirstlane(rec[0]) : 0u;
#pragma unroll
            for (int w = 0; w < 4; ++w) seg_rows[r][w] = __builtin_amdgcn_readfirstlane(rec[2 + w]);
        }
    }
    // node-sum ownership (step 1 of the node phase): thread -> (node slot, 4 columns).  The node's nrange record is first
    // used in layer 1's node phase; it is requested here with the edge records (loaded behind the P2 barrier it was one
    // more full round trip in front of layer 1's tiles).
    const int aslot = (tid >> 4) & (FUSED_MAX_NODES - 1), ac4 = (tid & 15) * 4;
    int4 nr_rec;
    // Every load of the index stages is unconditional, on a clamped index, and the lanes (or workgroups) that have no such
    // edge or node select their constant AFTER the wait (index_select): a load in an exec-masked region gets a wait of its
    // own.  A workgroup without edges (or nodes) reads its own descriptor instead of a record: 16 valid bytes.
    const int4* own_desc = reinterpret_cast<const int4*>(wgdesc + blockIdx.x);
    const int4* le_base = m > 0 ? ledge + eb : own_desc;
    const int4* nr_base = n > 0 ? reinterpret_cast<const int4*>(nrange) + nb : own_desc;
    const float* ea_base = m > 0 ? edge_attr_orig : reinterpret_cast<const float*>(own_desc);
    const float* qattr = dbg.step.qattr;
    auto index_stage_a = [&]() {
        f_e = le_base[f_have ? f_local : 0];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int tile = NW * r + wave, local = 16 * tile + i;
            t_e[r] = le_base[local < m ? local : 0];
        }
        nr_rec = nr_base[aslot < n ? aslot : 0];
    };
    auto index_select = [&]() {
        if (!f_have) f_e = make_int4(0, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            t_e[r].x = m > 0 ? t_e[r].x : 0; t_e[r].y = m > 0 ? t_e[r].y : vb;
            t_e[r].z = m > 0 ? t_e[r].z : nb; t_e[r].w = m > 0 ? t_e[r].w : 0;
        }
    };
    // (returns its result: written through the capture, the two floats were kept in scratch memory -- 8 bytes per thread
    // stored and re-loaded, + 1 MB of WRITE_SIZE per launch in the first version)
    // Lanes without an edge hold a zero record (index_select) and load element 0; P2 reads f_ea only on lanes that have
    // the edge.  The two values come back as loaded (rollout: q_i and q_j, multiplied in P2): arithmetic on them here
    // would be a wait for them in the middle of the field net.
    auto index_stage_b = [&]() -> f32x2 {
        f32x2 v;
        if (qattr) {                       // main.py:243-246: q_i q_j (the distance is computed with the features)
            v[0] = qattr[f_e.y]; v[1] = qattr[f_e.z];
        } else {
            const float* ea = ea_base + 2 * (int64_t)f_e.w;
            v[0] = ea[0]; v[1] = ea[1];
        }
        return v;
    };

    // ---------------------------------------------------------------- P1: field net, frames, x0 on the matrix core
    // aether.py:108-134 (field), geometry.py:7-73 + aether.py:33-50 (frames), locs.py:214-218 (x0).
    // Wave t owns the visible nodes 16t .. 16t+15 as the 16 columns of its MFMA tiles; the three
    // Linear layers chain in accumulator layout, lanes q == 0 end up with the node's force and build
    // its frame, and x0 = res(rel_feat) is one more tile product: no workgroup barrier in between.
    // (NW == 12, FRAMES above: the field wave stops at the force; frames on waves 2, 3 in the else branch, x0 behind the barrier.)
    // The field wave's load block is: every pointer it needs out of the kernel arguments (scalar loads, one wait),
    // then every vector load (inputs, 2,080 field parameters, res weights, the external field, this wave's edge and
    // node records) back to back and unconditional, on clamped indices, then ONE vmcnt(0); lanes whose element does not exist select
    // their zero behind that wait.  (Left to the compiler the block held three scalar round trips and three vmcnt(0):
    // a conditional load becomes an exec-masked region with a wait of its own.)  The only loads behind the wait are
    // the edge attributes, whose address needs the edge record: they are issued behind the layer-1 MFMAs.
    // NW == 12 (FIMG): the parameters come as the field image that k_prepare_weights writes once per weight version --
    // 25 buffer loads of 16 bytes in place of 42 loads (D = 2; 28 of them 4-byte gathers), their address instructions and
    // the selects behind the wait; the same fp32 values reach the same MFMAs in the same order.
    {
        const int vtiles = (nv + 15) >> 4;
        if (wave < vtiles) {
            const float* p_ext;
            int node;                                          // visible slot
            bool live;
            int64_t g;
            float pz[D], vz[D], ef[D];
            float ch;
            // layer-1 operands: B = z[k][node], A = W0[16mb + i][k], k = 4s + q (FIN = 2D + 16 <= 24)
            float zc[6][3], a1[2][6];
            f32x4 w2f[2][2], w4f[2], acc1[2], acc2[2];
            f32x4 acc3 = f32x4{0.f, 0.f, 0.f, 0.f};
            // x0 operands: A = W_res[16mb + i][D + k], k = 4s + q < 2D (the first D inputs of rel_feat are zero)
            float ar[4][2];
            f32x4 acc0[4];
            f32x4 fimg[FIMG ? FUSED_FIMG_CHUNKS : 1];
            if constexpr (FIMG) {
                // The weight operands come as the field image (fused_layout.h, FI_*): 25 16-byte buffer loads on one lane
                // offset and immediate chunk offsets, every mask already a zero -- no parameter pointer, no address
                // arithmetic and no select behind the wait.  The descriptor covers the image alone.
                const auto fimg_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dbg.wimg) + fused_fimg_offset(), 0, FUSED_FIMG * 4, 0x00020000);
                p_ext = dbg.step.ext_field ? dbg.step.ext_field : x;      // (no external field: x again, not used)
                asm volatile("" :: "s"(fimg_rsrc), "s"(p_ext), "s"(x), "s"(vel), "s"(charges), "s"(le_base), "s"(nr_base),
                             "s"(ea_base), "s"(qattr));            // all in scalar registers before the first vector load
                node = 16 * wave + i;
                live = node < nv;
                g = vb + (live ? node : 0);
                FUSED_PSTAMP(0, f_e.x);
#pragma unroll
                for (int d = 0; d < D; ++d) { pz[d] = x[g * D + d]; vz[d] = vel[g * D + d]; ef[d] = p_ext[g * D + d]; }
                ch = charges[g];
#pragma unroll
                for (int c = 0; c < FUSED_FIMG_CHUNKS; ++c)
                    if (fused_fimg_field_chunk(c))                // (19 of the 25: the x0 operands are the x0 waves')
                        fimg[c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(fimg_rsrc, lane * 16, c * 1024, 0));
            } else {
                const float* p_emb = P.field_emb; const float* p_w0 = P.field_w0; const float* p_b0 = P.field_b0;
                const float* p_w2 = P.field_w2; const float* p_b2 = P.field_b2; const float* p_w4 = P.field_w4;
                const float* p_b4 = P.field_b4; const float* p_rb = P.l1_res_b; const float* p_rw = P.l1_res_w;
                p_ext = dbg.step.ext_field ? dbg.step.ext_field : x;      // (no external field: x again, not used)
                asm volatile("" :: "s"(p_emb), "s"(p_w0), "s"(p_b0), "s"(p_w2), "s"(p_b2), "s"(p_w4), "s"(p_b4), "s"(p_rb),
                             "s"(p_rw), "s"(p_ext), "s"(x), "s"(vel), "s"(charges), "s"(le_base), "s"(nr_base), "s"(ea_base),
                             "s"(qattr));                          // all in scalar registers before the first vector load
                node = 16 * wave + i;
                live = node < nv;
                g = vb + (live ? node : 0);
                FUSED_PSTAMP(0, f_e.x);
#pragma unroll
                for (int d = 0; d < D; ++d) { pz[d] = x[g * D + d]; vz[d] = vel[g * D + d]; ef[d] = p_ext[g * D + d]; }
                ch = charges[g];
#pragma unroll
                for (int s4 = 0; s4 < 6; ++s4) {
                    const int k = 4 * s4 + q;
                    const int ke = (k >= 2 * D && k < FIN) ? k - 2 * D : 0, kw = k < FIN ? k : 0;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        zc[s4][c] = (4 * s4 + 3 >= 2 * D && 4 * s4 < FIN) ? p_emb[c * 16 + ke] : 0.0f;
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) a1[mb][s4] = 4 * s4 < FIN ? p_w0[(16 * mb + i) * FIN + kw] : 0.0f;
                }
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    acc1[mb] = ld4(p_b0 + 16 * mb + 4 * q);
                    acc2[mb] = ld4(p_b2 + 16 * mb + 4 * q);
#pragma unroll
                    for (int a = 0; a < 2; ++a) w2f[mb][a] = ld4(p_w2 + (16 * mb + i) * 32 + 16 * a + 4 * q);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) w4f[a] = ld4(p_w4 + (i < D ? i : 0) * 32 + 16 * a + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc3[r] = r < D ? p_b4[4 * q + r < D ? 4 * q + r : 0] : 0.0f;
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    acc0[mb] = ld4(p_rb + 16 * mb + 4 * q);
#pragma unroll
                    for (int s4 = 0; s4 < 2; ++s4)
                        ar[mb][s4] = 4 * s4 < 2 * D ? p_rw[(16 * mb + i) * 3 * D + D + (4 * s4 + q < 2 * D ? 4 * s4 + q : 0)] : 0.0f;
                }
            }
            index_stage_a();                                  // behind this wave's own inputs (in-order returns: they do not wait for it)
            // The one wait of the block, in the form the compiler's wait-count pass sees (simm16 of vmcnt(0) alone): it places none
            // of its own in front of the MFMAs.
            // Nothing is scheduled across the wait (sched_barrier), and every loaded value is named right behind it (empty
            // statements), the ones used last first: the scheduler would otherwise sink the loads whose values the first
            // MFMAs do not need below the wait, and the wait-count pass would add waits of its own for them.
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __builtin_amdgcn_sched_barrier(0);
            FUSED_PSTAMP(1, f_e.x);
            auto landed = [](auto v) { asm volatile("" :: "v"(v)); };
            auto landed4 = [](const int4& v) { asm volatile("" :: "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); };
            landed4(f_e); landed4(nr_rec);
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) landed4(t_e[r]);
#pragma unroll
            for (int d = 0; d < D; ++d) { landed(pz[d]); landed(vz[d]); landed(ef[d]); }
            landed(ch);
            if constexpr (FIMG) {
#pragma unroll
                for (int c = 0; c < FUSED_FIMG_CHUNKS; ++c)
                    if (fused_fimg_field_chunk(c)) landed(fimg[c]);
                // the operands are the image's slots as they stand (FI_*): register names, no instruction
                auto slot = [&](int s) { return fimg[s >> 2][s & 3]; };
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    acc1[mb] = fimg[FI_ACC1 / 4 + mb]; acc2[mb] = fimg[FI_ACC2 / 4 + mb];
#pragma unroll
                    for (int a = 0; a < 2; ++a) w2f[mb][a] = fimg[FI_W2F / 4 + 2 * mb + a];
#pragma unroll
                    for (int s4 = 0; s4 < 6; ++s4) a1[mb][s4] = slot(FI_A1 + 6 * mb + s4);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) w4f[a] = fimg[FI_W4F / 4 + a];
                acc3 = fimg[FI_ACC3 / 4];
#pragma unroll
                for (int s4 = 0; s4 < 6; ++s4)
#pragma unroll
                    for (int c = 0; c < 3; ++c) zc[s4][c] = slot(FI_ZC + 3 * s4 + c);
                static_assert(FRAMES, "FI_ACC0 / FI_AR: the x0 waves' operands, loaded by them (P1's else branch)");
            } else {
#pragma unroll
                for (int s4 = 0; s4 < 6; ++s4) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (4 * s4 + 3 >= 2 * D && 4 * s4 < FIN) landed(zc[s4][c]);
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb)
                        if (4 * s4 < FIN) landed(a1[mb][s4]);
                }
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) { landed(acc1[mb]); landed(acc2[mb]); landed(w2f[mb][0]); landed(w2f[mb][1]); }
                landed(w4f[0]); landed(w4f[1]);
#pragma unroll
                for (int r = 0; r < D; ++r) landed(acc3[r]);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    landed(acc0[mb]);
#pragma unroll
                    for (int s4 = 0; s4 < 2; ++s4)
                        if (4 * s4 < 2 * D) landed(ar[mb][s4]);
                }
#pragma unroll
                for (int s4 = 0; s4 < 6; ++s4) {
                    const int k = 4 * s4 + q;
#pragma unroll
                    for (int c = 0; c < 3; ++c) zc[s4][c] = (k >= 2 * D && k < FIN) ? zc[s4][c] : 0.0f;
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) a1[mb][s4] = k < FIN ? a1[mb][s4] : 0.0f;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) w4f[a] = i < D ? w4f[a] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) acc3[r] = (4 * q + r < D) ? acc3[r] : 0.0f;
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int s4 = 0; s4 < 2; ++s4) ar[mb][s4] = 4 * s4 + q < 2 * D ? ar[mb][s4] : 0.0f;
            }
            index_select();
            long ci = (long)(ch + 1.0f);                        // charge_to_index: (q + 1).long(), aether.py:127-129
            ci = ci < 0 ? 0 : (ci > 2 ? 2 : ci);
#pragma unroll
            for (int s4 = 0; s4 < 6; ++s4) {
                const int k = 4 * s4 + q;
                float zk = ci == 0 ? zc[s4][0] : (ci == 1 ? zc[s4][1] : zc[s4][2]);
#pragma unroll
                for (int d = 0; d < D; ++d) { zk = k == d ? pz[d] : zk; zk = k == D + d ? vz[d] : zk; }
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) acc1[mb] = mfma16(a1[mb][s4], zk, acc1[mb]);
            }
            f32x4 hh[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) hh[mb] = silu4(acc1[mb]);
            // the edge record is opaque up to here: the attribute loads, whose addresses need it, stay behind the layer-1 MFMAs
            asm volatile("" : "+v"(f_e.y), "+v"(f_e.z), "+v"(f_e.w) : "v"(hh[0][0]));
            f_ea = index_stage_b();                                    // (the records are back by now; measured: asked for earlier, nothing gained)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) acc2[mb] = mfma16(w2f[mb][a][b], hh[a][b], acc2[mb]);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) hh[mb] = silu4(acc2[mb]);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc3 = mfma16(w4f[a][b], hh[a][b], acc3);
            FUSED_PSTAMP(2, acc3[0]);
            if constexpr (FRAMES) {
                // lanes q == 0: acc3[d] = force component d of node i -> the record's F words; the rest of the record is the
                // frame wave's, x0 the x0 waves'
                if (q == 0 && live) {
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        ninfo[node * 24 + NI::F + d] = dbg.step.ext_field ? ef[d] : acc3[d];       // (live: g = vb + node)
                }
                FUSED_PSTAMP(3, acc3[0]);
            } else {
                // lanes q == 0: acc3[d] = force component d of node i -> frame + NodeInfo record
                if (q == 0 && live) {
                    float f[D], R[D][D], cv[D], cf[D];
#pragma unroll
                    for (int d = 0; d < D; ++d)
                        f[d] = dbg.step.ext_field ? ef[d] : acc3[d];       // (live: g = vb + node)
                    node_frame<D>(vz, f, R, cv, cf);
                    float* ni = ninfo + node * 24;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        ni[NI::P + d] = pz[d]; ni[NI::V + d] = vz[d]; ni[NI::F + d] = f[d];
                        ni[NI::CV + d] = cv[d]; ni[NI::CF + d] = cf[d];
#pragma unroll
                        for (int e = 0; e < D; ++e) ni[NI::R + d * D + e] = R[d][e];
                    }
                    if (keep && node >= off && node < off + n) {
                        float* gni = dbg.nodeinfo + (int64_t)(vb + node) * NI::STRIDE;
#pragma unroll
                        for (int t = 0; t < NI::STRIDE; ++t) gni[t] = t < NI::CF + D ? ni[t] : 0.0f;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                FUSED_PSTAMP(3, acc3[0]);
                // x0 = W_res[:, D:] [cv | cf] + b (own nodes only; cv, cf are contiguous in the record)
#pragma unroll
                for (int s4 = 0; s4 < 2; ++s4) {
                    const int k = 4 * s4 + q;
                    const float rk = (live && k < 2 * D) ? ninfo[node * 24 + NI::CV + k] : 0.0f;
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) acc0[mb] = mfma16(ar[mb][s4], rk, acc0[mb]);
                }
                const int own = node - off;
                if (own >= 0 && own < n) {
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) {
                        st4(xbuf + own * LDW + 16 * mb + 4 * q, acc0[mb]);
                        if (keep) st4(dbg.x[0] + (int64_t)(nb + own) * H + 16 * mb + 4 * q, acc0[mb]);
                    }
                }
                FUSED_PSTAMP(4, acc0[3][0]);
            }
        } else {
            // FRAMES: the frame wave's inputs and an x0 wave's operands go out in front of the index loads: unconditional, on
            // clamped indices (a wave without that role loads node vb and row block wave & 3 and uses neither)
            const int ft = fused_frame_tile(wave), fnode = 16 * ft + i;
            const bool fwave = FRAMES && ft >= 0 && ft < vtiles;
            const bool flive = fwave && fnode < nv;
            float pz[D], vz[D];
            if constexpr (FRAMES) {
                const auto fimg_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dbg.wimg) + fused_fimg_offset(), 0, FUSED_FIMG * 4, 0x00020000);
                const int64_t g = vb + (flive ? fnode : 0);
#pragma unroll
                for (int d = 0; d < D; ++d) { pz[d] = x[g * D + d]; vz[d] = vel[g * D + d]; }
                const int mb = __builtin_amdgcn_readfirstlane(fused_x0_rowblock(wave)) & 3;
                x0_acc = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(fimg_rsrc, lane * 16, (FI_ACC0 / 4 + mb) * 1024, 0));
                x0_ar = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(fimg_rsrc, lane * 16, ((FI_AR + 2 * mb) >> 2) * 1024, 0));
            }
            index_stage_a();
            index_select();
            f_ea = index_stage_b();
            if constexpr (FRAMES) {
                // the inputs are read in an exec-masked region only: named here, the wait for them stands in front of it (the
                // first loads of the wave: the index loads stay in flight)
#pragma unroll
                for (int d = 0; d < D; ++d) asm volatile("" :: "v"(pz[d]), "v"(vz[d]));
                FUSED_PSTAMP_W(FUSED_FRAME_WAVE0, 5, vz[0]);
                // lanes 0-15 of a frame wave: P, V, R, CV of the node's record (F: the field wave; CF: not stored)
                if (flive && q == 0) {
                    float R[D][D], cv[D];
                    node_frame_vel<D>(vz, R, cv);
                    float* ni = ninfo + fnode * 24;
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        ni[NI::P + d] = pz[d]; ni[NI::V + d] = vz[d]; ni[NI::CV + d] = cv[d];
#pragma unroll
                        for (int e = 0; e < D; ++e) ni[NI::R + d * D + e] = R[d][e];
                    }
                }
                FUSED_PSTAMP_W(FUSED_FRAME_WAVE0, 6, vz[0]);
            }
            // rows of unused node slots are zero
            for (int idx = tid - 64 * vtiles; idx < (FUSED_MAX_NODES - n) * (H / 4); idx += THREADS - 64 * vtiles)
                st4(xbuf + (n + (idx >> 4)) * LDW + (idx & 15) * 4, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        // P0, second half: the layer-1 weights and constants are in LDS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's LDS-DMA fragments have landed
        lds_barrier();
    }
    FUSED_STAMP(2);

    // ---------------------------------------------------------------- x0 (12 waves), beside P2's feature build
    // x0 = W_res[:, D:] [cv | cf] + b (locs.py:214-218), own nodes only: wave FUSED_X0_WAVE0 + mb computes rows 16 mb .. + 15
    // for every visible node tile that holds own nodes -- the field wave's two MFMAs per accumulator in its k order, on
    // the same operands.  The rows are published by P2's barriers, three barriers before step 1 of layer 1 reads them.
    if constexpr (FRAMES) {
        // (loaded in P1's else branch, read in a branch on the wave index: named here so that the compiler's wait for
        // them stands behind the vmcnt(0) above and not in the layer loop, see f_ea below)
        asm volatile("" :: "v"(x0_acc), "v"(x0_ar));
        const int mb = __builtin_amdgcn_readfirstlane(fused_x0_rowblock(wave));
        if (mb >= 0 && mb < FUSED_X0_WAVES) {
            FUSED_PSTAMP_W(FUSED_X0_WAVE0, 7, x0_acc[0]);
            const float ar[2] = {(mb & 1) ? x0_ar[0] : x0_ar[2], (mb & 1) ? x0_ar[1] : x0_ar[3]};
            const int vtiles = (nv + 15) >> 4;
            for (int t = 0; t < vtiles; ++t) {
                const int lo = 16 * t > off ? 16 * t : off, hi = 16 * t + 16 < off + n ? 16 * t + 16 : off + n;
                if (lo >= hi) continue;                        // no own node in this tile
                const int node = 16 * t + i;
                const bool live = node < nv;
                const float* ni = ninfo + (live ? node : 0) * 24;
                float rec[2 * D];                                  // [cv | cf]
#pragma unroll
                for (int d = 0; d < D; ++d) rec[d] = ni[NI::CV + d];
                {
                    float Rl[D * D], fl[D];
#pragma unroll
                    for (int d = 0; d < D; ++d) fl[d] = ni[NI::F + d];
#pragma unroll
                    for (int d = 0; d < D * D; ++d) Rl[d] = ni[NI::R + d];
                    node_frame_force<D>(Rl, fl, rec + D);
                }
                f32x4 acc = x0_acc;
#pragma unroll
                for (int s4 = 0; s4 < 2; ++s4) {
                    const int k = 4 * s4 + q;
                    float rk = 0.0f;
#pragma unroll
                    for (int kk = 4 * s4; kk < 4 * s4 + 4 && kk < 2 * D; ++kk) rk = (live && k == kk) ? rec[kk] : rk;
                    acc = mfma16(ar[s4], rk, acc);
                }
                const int own = node - off;
                if (own >= 0 && own < n) st4(xbuf + own * LDW + 16 * mb + 4 * q, acc);
            }
            FUSED_PSTAMP_W(FUSED_X0_WAVE0, 8, x0_acc[0]);
        }
    }

    // ---------------------------------------------------------------- P2: edge features -> B operands
    // Wave w owns tiles {w, w+NW, ..}.  Per tile, 16 lanes each build the features of one edge into
    // the wave's scratch rows; then every lane reads its B fragments back.  Per-tile constants of
    // the graph structure (sender / receiver slot, receiver-segment index) are computed once here.
    int sl[ROUNDS], rl[ROUNDS];              // sender slot (visible numbering), receiver slot (own numbering)
    f32x4 e[ROUNDS][4];                      // message tiles, MFMA accumulator layout
    int ke[KEEP ? ROUNDS : 1];               // KEEP: receiver-sorted position of the lane's edge (row of the saved tensors)
    {
        float* scratch = smem + L::FEAT + wave * (L::FEAT_ROWS * LDF);
#pragma unroll
        for (int r0 = 0; r0 < ROUNDS; r0 += 2) {               // two rounds (32 scratch rows) per pass
            constexpr int PASS = 2;
            const int nr_pass = ROUNDS - r0 < PASS ? ROUNDS - r0 : PASS;
            if (PACKED ? wave < FUSED_PACK_WAVES && lane < FUSED_PACK_LANES : lane < 16 * nr_pass) {
                const int r = r0 + (lane >> 4), ii = lane & 15;
                const int local = PACKED ? f_local : 16 * (NW * r + wave) + ii;
                float o[FPAD];
                if (local < m) {
                    // position in the receiver-sorted edge list, sender, receiver (first pass: requested during P1)
                    const int4 le = r0 == 0 ? f_e : ledge[eb + local];
                    const int k = le.x, ks = le.y, kr = le.z;
                    const float* nj = ninfo + (ks - vb) * 24;
                    const float* nr = ninfo + (kr - vb) * 24;
                    float njl[NI::STRIDE], nrl[NI::STRIDE];
#pragma unroll
                    for (int t = 0; t < NI::STRIDE; ++t) { njl[t] = nj[t]; nrl[t] = nr[t]; }
                    // FRAMES: the record's CF words were not written (LDS keeps the previous launch's): cf = R^T f of the
                    // receiver from the copy; the sender's are not read
                    if constexpr (FRAMES) node_frame_force<D>(nrl + NI::R, nrl + NI::F, nrl + NI::CF);
                    float eal[2];
                    if (dbg.step.qattr) {          // main.py:243-246: [q_i q_j, sqrt(sum((x_i - x_j)^2))]
                        float d2 = 0.0f;
#pragma unroll
                        for (int d = 0; d < D; ++d) {
                            const float df = njl[NI::P + d] - nrl[NI::P + d];
                            d2 += df * df;
                        }
                        eal[0] = r0 == 0 ? f_ea[0] * f_ea[1] : dbg.step.qattr[ks] * dbg.step.qattr[kr];
                        eal[1] = sqrtf(d2);
                    } else if (r0 == 0) {
                        eal[0] = f_ea[0]; eal[1] = f_ea[1];
                    } else {
                        const float* ea = edge_attr_orig + 2 * (int64_t)le.w;
                        eal[0] = ea[0]; eal[1] = ea[1];
                    }
                    edge_features<D>(njl, nrl, eal, o);
                } else {
#pragma unroll
                    for (int t = 0; t < FPAD; ++t) o[t] = 0.0f;
                }
#pragma unroll
                for (int t = 0; t < FPAD; t += 4)
                    st4((PACKED ? smem + L::FEAT + local * LDF : scratch + lane * LDF) + t, f32x4{o[t], o[t + 1], o[t + 2], o[t + 3]});
            }
            // PACKED: the rows were written by another wave (row `local` of L::FEAT is row local & 15 of wave local >> 4).
            // Every wave of every workgroup arrives here, whether it built rows, owns a tile, or the group has no edge.
            if constexpr (PACKED) lds_barrier();
            else __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int rr = 0; rr < PASS; ++rr) {
                const int r = r0 + rr;
                if (r < ROUNDS) {
                    e[r][0] = ld4(scratch + (16 * rr + i) * LDF + 4 * q);   // features as bop[0..1]
                    e[r][1] = ld4(scratch + (16 * rr + i) * LDF + 16 + 4 * q);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this pass's features sit in registers ...
            __builtin_amdgcn_wave_barrier();                       // ... before the next pass overwrites the rows
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            e[r][2] = f32x4{0.f, 0.f, 0.f, 0.f};
            e[r][3] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int local = 16 * (NW * r + wave) + i;
            sl[r] = t_e[r].y - vb;                             // (requested during P1)
            rl[r] = t_e[r].z - nb;
            if constexpr (KEEP) {
                ke[r] = local < m ? t_e[r].x : -1;
                // the saved feature rows, from the B-operand registers: 16 rows x 64 contiguous bytes per store and all 64 lanes
                // (written by the lane that built the row they went out as eight 16-byte pieces per lane, half the wave idle)
                if (ke[r] >= 0) {
                    st4(dbg.feat + (int64_t)ke[r] * FPAD + 4 * q, e[r][0]);
                    st4(dbg.feat + (int64_t)ke[r] * FPAD + 16 + 4 * q, e[r][1]);
                }
            }
        }
        lds_barrier();       // feature scratch (aliases SCRATCH) is dead from here on
    }
    FUSED_STAMP(3);

    // node sums (step 1 of the node phase; aslot, ac4 above): the in-edge sum of a node arrives as per-(receiver, tile)
    // partial rows `part[node + tile]`.  Two runs of tiles per node (own senders / partner's senders, see FusedWG); the
    // second run's rows are offset by n.  The record arrived during P1 (index_stage_a).
    // The four tile bounds (each below 2 * 32 + 16 partial rows) travel through the layers as bytes of one register.
    unsigned arange = 0;
    float adeg = 1.0f;
    if constexpr (NW == 12) {
        // The edge attributes and the nrange record are read in exec-masked regions only (P2: lanes that build an edge;
        // below: threads that own a node slot).  On the path around such a region the compiler's wait-count pass carries
        // the loads as still in flight into the layer loop, and the first instruction there that reuses one of their
        // registers gets a vmcnt(0) -- behind part 1 of the node phase's prefetch, in every tile of every layer (1,800 of a
        // tile's 7,600 cycles in the first stamped build).  Naming the values here puts that wait in front of the loop,
        // where they have long landed.
        asm volatile("" :: "v"(f_ea[0]), "v"(f_ea[1]), "v"(nr_rec.x), "v"(nr_rec.y), "v"(nr_rec.z), "v"(nr_rec.w));
    }
    if (aslot < n) {
        const int4 nr = nr_rec;
        const int at0 = nr.x >> 4;
        const int at1 = nr.y > nr.x ? ((nr.y - 1) >> 4) + 1 : at0;
        const int bt0 = (nr.z >> 4) + n;
        const int bt1 = nr.w > nr.z ? ((nr.w - 1) >> 4) + 1 + n : bt0;
        arange = (unsigned)at0 | (unsigned)at1 << 8 | (unsigned)bt0 << 16 | (unsigned)bt1 << 24;
        const int deg = (nr.y - nr.x) + (nr.w - nr.z);
        adeg = (float)(deg > 1 ? deg : 1);
    }

    // next layer's W_s / W_r fragments (after layer 4: out_w0 / out_w3): fp16 x 2 pieces of the wave's row block, k blocks 0, 1
    f16x8 wsh[2], wsl[2], wrh[2], wrl[2];
    // NW == 12: ONE set of four hi and four lo fragments per wave for all its roles (registers are allocated statically,
    // whatever the wave's run-time role).  Waves 0-7: slots 0, 1 = W3 row block `wave`; slots 2, 3 = the next layer's
    // W_s (waves 0-3) or W_r (waves 4-7), row block wave & 3 (layer 4: out_w0 / out_w3).  Waves 8-11: slots 0-3 = the
    // four k blocks of W4 row block wave & 3.  w3* / w4* / ws* / wr* are not used then.
    f16x8 wf_h[4], wf_l[4];
    // the node phase's fragments come by buffer loads (issue_loads): descriptor of the whole image set, the lane's 16 bytes
    const auto wimg_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dbg.wimg), 0, FUSED_WIMG_SPLIT * 4, 0x00020000);
    const int lane16 = lane * 16;
#pragma unroll 1
    for (int layer = 1; layer <= 4; ++layer) {
        // ------------------------------------------------------------ edge tiles (locs.py:227-238)
        // No workgroup barrier in here.  A wave with K tiles runs them through one branch-free block
        // (front = first Linear + SiLU, back = second Linear + SiLU + per-receiver sums) so that the
        // compiler can overlap one tile's VALU / LDS tail with the next tile's MFMAs.
        const float* cb = cblk + (layer & 1) * FUSED_CBLK;   // this layer's constants (CB_*)
        // work split: step 2 has 16 (row block, node tile) units, step 3 has 8, step 4 has 16
        const int mb2 = wave & 7;                         // step 2: rows 16*mb2.. of the 128
        const int mb3 = wave & 3, tn3 = (wave >> 2) & 1;  // steps 3, 4: rows 16*mb3.. of node tile tn3
        const bool act3 = wave < 8;                       // steps 2 - 4 / out MLP: waves 0-7
        // One node tile (split mode, small groups): step 3 runs on waves 4-7, which own at most one edge tile per layer,
        // so a two-tile wave (0-3) never asks for the W4 fragments nor carries them through its last tile; in step 4 waves
        // 0-3 compute P_s and waves 4-7 P_r, all on tile 0.  Two node tiles: wave -> (mb3, tn3) in steps 3 and 4.
        const bool one_tile = NW == 12 ? true : n <= 16;
        const int tn4 = one_tile ? 0 : tn3;
        const int tn3s = tn4;
        const bool do3 = NW == 12 ? wave >= 8 : act3 && (one_tile ? wave >= 4 : 16 * tn3 < n);   // (NW == 12: mb3 = wave & 3, tn3 = 0)
        const bool do_s = act3 && (one_tile ? wave < 4 : true);
        const bool do_r = act3 && (one_tile ? wave >= 4 : true);
        // Every register load of the node phase is issued BEFORE the end of the wave's last edge tile, so that
        // the weight fragments a workgroup needs per layer (all 256 workgroups ask at the same moment) stream in under
        // the tile's MFMAs: W3 / W4 / next-layer W_s, W_r fragments.  Step 1 waits for them once; between that wait and
        // the end of step 4 nothing waits for global memory (biases: the constants block in LDS).
        f16x8 w3h[2], w3l[2], w4h[4], w4l[4];              // the wave's row block of W3 (k = 64) and of W4 (k = 128), split pieces
        // layer 4 has no next edge layer: wsv / wrv carry the out-MLP fragments (out_w0, out_w3) instead
        // part 1: W3; 2, 3: W4 halves; 4: W_s / W_r.  A wave spreads the parts over
        // its last tile (a burst of ~20 loads per wave blocks at issue until the L2 returns drain).
        // No part waits for an earlier one: every fragment is a buffer load whose address is the image set's descriptor, the
        // wave-uniform block offset in a scalar register and ONE lane-offset register shared by all of them.  (As
        // global loads from a pointer each fragment had a 64-bit address pair of its own, which the compiler allocated
        // in the destination registers of fragments still in flight -- a vmcnt(0) in front of every part.)
        auto frag = [&](int block_bytes, int kb) -> f16x8 {
            return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wimg_rsrc, lane16, block_bytes + kb * 1024, 0));
        };
        // term 0 / term 1 (hi / lo pieces) of row block mb of a <MBN, KBN> image: k blocks of 64 fragments, 1 KiB each
        auto load_frags = [&](int which, int mb, int MBN, int KBN, int kb0, int nkb, f16x8* wh, f16x8* wl) {
            // The three-tile KEEP kernel sits at the register ceiling: it keeps the loads through a pointer.  Their waits
            // are what lets a part's address pair live in registers of fragments that have landed; without them the
            // kernel spills 16 bytes instead of 12.
            if constexpr (ROUNDS == 3 && KEEP) {
                const f16x8* w = reinterpret_cast<const f16x8*>(dbg.wimg + fused_nimg_offset(layer, which)) +
                                 __builtin_amdgcn_readfirstlane(mb) * (KBN * 64);
#pragma unroll
                for (int kb = kb0; kb < kb0 + nkb; ++kb) {
                    wh[kb] = w[kb * 64 + lane];
                    wl[kb] = w[MBN * KBN * 64 + kb * 64 + lane];
                }
                return;
            }
            // (the layer's offset is opaque: hoisted out of the layer loop, the block offsets of all parts occupy scalar
            // registers through the tiles, and their spills vector registers)
            int lbytes = (layer - 1) * (FUSED_NIMG_LAYER * 4);
            asm volatile("" : "+s"(lbytes));
            const int blk = fused_nimg_offset(1, which) * 4 + lbytes + __builtin_amdgcn_readfirstlane(mb) * (KBN * 1024);
#pragma unroll
            for (int kb = kb0; kb < kb0 + nkb; ++kb) {
                wh[kb] = frag(blk, kb);
                wl[kb] = frag(blk + MBN * KBN * 1024, kb);
            }
        };
        auto issue_loads = [&](int part) {
            if constexpr (NW == 12) {
                // The wave's role picks the image and the row block by scalar selects -- no branch on the role around a
                // load; the fragments, their k order and the hi / lo pieces are those of load_frags.  Every wave issues
                // four fragments with part 1 (slots 0, 1) and four with part 3 (slots 2, 3); parts 2 and 4 are empty.
                const int wv = __builtin_amdgcn_readfirstlane(wave);
                int lbytes = (layer - 1) * (FUSED_NIMG_LAYER * 4);
                asm volatile("" : "+s"(lbytes));
                const bool w4 = wv >= 8;
                // slots 0, 1: W3 <8, 2> row block wv, or k blocks 0, 1 of W4 <4, 4> row block wv & 3 (lo pieces 16 KiB behind
                // the hi pieces in both images); slots 2, 3: k blocks 2, 3 of the same W4 row block, or W_s / W_r <4, 2>
                // row block wv & 3 (lo pieces 8 KiB behind)
                const int blk01 = lbytes + (w4 ? fused_nimg_offset(1, 1) * 4 + (wv & 3) * 4096 : fused_nimg_offset(1, 0) * 4 + wv * 2048);
                const int blk23 = w4 ? blk01 + 2048 : lbytes + (wv < 4 ? fused_nimg_offset(1, 2) : fused_nimg_offset(1, 3)) * 4 + (wv & 3) * 2048;
                const int lo23 = w4 ? 16 * 1024 : 8 * 1024;
                if (part == 1) {
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) {
                        wf_h[kb] = frag(blk01, kb);
                        wf_l[kb] = frag(blk01 + 16 * 1024, kb);
                    }
                }
                if (part == 3) {
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) {
                        wf_h[2 + kb] = frag(blk23, kb);
                        wf_l[2 + kb] = frag(blk23 + lo23, kb);
                    }
                }
            } else {
            // (round 4: fragments of the prepared fp16 x 2 images, fused_nimg_offset -- same bytes per weight as fp32)
            if (part == 1 && act3) load_frags(0, mb2, 8, 2, 0, 2, w3h, w3l);
            if ((part == 2 || part == 3) && do3) load_frags(1, mb3, 4, 4, 2 * (part - 2), 2, w4h, w4l);
            if (part == 4 && (layer < 4 ? true : act3)) {
                if (layer == 4 || do_s) load_frags(2, mb3, 4, 2, 0, 2, wsh, wsl);
                if (layer == 4 || do_r) load_frags(3, mb3, 4, 2, 0, 2, wrh, wrl);
            }
            }
        };
        // Split mode, layers 2-4: the partner workgroup's P_s rows are in flight when the edge phase starts.  The
        // workgroup walks the tiles whose senders it owns first (local order, FusedWG); ONE wave (recv_wave below) polls
        // the partner's flag or granules, copies the rows into LDS and sets an LDS word; a wave waits on that word only
        // in its first tile with a partner sender, and there only behind the tile's first Linear (late_add).  No
        // workgroup barrier, and nobody waits while there is work that does not need the rows.
        const bool xch = wg.partner >= 0 && layer > 1;
        // Layers 2-4 of a split view: an edge whose sender the partner owns (local position >= na) starts its accumulator
        // at P_r alone; its P_s row is added behind the product (late_add), so that the first Linear of a tile runs
        // under the wait for the partner's rows.  late_tile (wave-uniform): the tile holds such an edge.  A select, not a
        // product with 0: the row that such a lane reads here is the previous layer's and may hold anything.  Every
        // other edge -- all of them in an unsplit view -- starts at P_r + P_s.  One rule in every instantiation that adds late (see the tile loop).
        // In those (LATE) the start is not the product's accumulator any more: the product g runs from zeros -- in the 12-wave
        // kernels under the previous node phase -- and the start is added to it, g + (P_r + P_s) or (g + P_r) + P_s.
        auto front_gemm = [&](int r, f32x4 (&acc)[4], bool last, bool late_tile) {
            if (layer == 1) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = ld4(cb + CB_B1 + 16 * mb + 4 * q);
                f32x4 bop[2] = {e[r][0], e[r][1]};
                gemm_split<4, 1>(EARLY ? smem + L::W1A : wA, bop, acc, lane);      // (EARLY: layer 1's image A lies in the P_s rows)
            } else {
                f32x4 pr[4], st[4];          // st: what the product is added to, P_r + P_s or P_r alone
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    pr[mb] = ld4(prb + rl[r] * LDW + 16 * mb + 4 * q);
                    st[mb] = pr[mb] + ld4(psb + sl[r] * LDW + 16 * mb + 4 * q);
                }
                if (late_tile) {
                    const bool late = 16 * (NW * r + wave) + i >= na;
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                        for (int c = 0; c < 4; ++c) st[mb][c] = late ? pr[mb][c] : st[mb][c];
                }
                if constexpr (LATE) {
                    if constexpr (EARLY) {           // the tile holds g already (early_product, previous node phase)
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) acc[mb] = e[r][mb] + st[mb];
                    } else {
                        f32x4 g[4];
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) g[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
                        gemm_split<4, 2>(wA, e[r], g, lane);
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) acc[mb] = g[mb] + st[mb];
                    }
                } else {
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) acc[mb] = st[mb];
                    gemm_split<4, 2>(wA, e[r], acc, lane);
                }
            }
        };
        // ... and the partner senders' P_s rows, in front of the first SiLU (the caller has waited for them)
        auto late_add = [&](int r, f32x4 (&acc)[4]) {
            const bool late = 16 * (NW * r + wave) + i >= na;
            f32x4 ps[4];           // four reads in flight and one wait (read by read, a late tile paid four LDS round trips)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) ps[mb] = ld4(psb + sl[r] * LDW + 16 * mb + 4 * q);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ps[0]), "+v"(ps[1]), "+v"(ps[2]), "+v"(ps[3]));
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[mb][c] = late ? acc[mb][c] + ps[mb][c] : acc[mb][c];
        };
        auto receive_partner_rows = [&]() {
            if constexpr (GRAN) {             // no flag to poll, the rows' own tags say when they are there
                FUSED_WSTAMP(layer, 0, 6);
                gran_receive(gran_rsrc(dbg.flags, wg.goff, vb, nv), layer, nv, n, off, lane, psb, arrived, dbg.errword);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // rows are in LDS before the word says so
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) arrived[0] = layer;
                FUSED_WSTAMP(layer, 0, 7);
                return;
            }
            // second half of the hand-off (first half: end of the previous node phase), run by ONE wave: lane 0
            // polls the partner's flag (bounded: a wait that gives up reports through dbg.errword), then the wave
            // reads the partner's rows with sc1 (L1-bypassing) 16-byte buffer loads -- the only loads of those
            // bytes in this launch -- into LDS and publishes them to the other waves through an LDS word
            // (cdna_hip_programming.md Guideline 16: "the other waves load after ... an LDS word it then sets").
            if (lane == 0) {
                unsigned spins = 0;
                unsigned long long t_first = 0;
                while (__hip_atomic_load(dbg.flags + wg.partner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < layer - 1) {
                    __builtin_amdgcn_s_sleep(2);
                    // bounded by TIME (5 s of the 100 MHz wall clock), not by a spin count: when the device is shared
                    // (another process, another stream) the partner may legitimately be scheduled late -- a count of
                    // 2^22 polls gave up in a two-process rehearsal on one GPU
                    if ((++spins & 1023u) == 0) {
                        const unsigned long long now = wall_clock64();
                        if (t_first == 0) t_first = now;
                        if (now - t_first <= 500000000ull) continue;
                        // partner not resident: give up, never hang -- and say so:
                        // the host-mapped word for the next entry point / aether_check_async_error, and an LDS word that
                        // turns this workgroup's outputs into NaN (a launch that finished on stale rows must not look valid)
                        if (dbg.errword) __hip_atomic_store(dbg.errword, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        arrived[1] = 1;
                        break;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int np = nv - n;                              // partner rows = visible slots outside [off, off + n)
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(dbg.ps[layer - 2] + (int64_t)vb * H, 0, nv * H * 4, 0x00020000);
            FUSED_WSTAMP(layer, 0, 6);
            if constexpr (NW == 12) {
                // Seven of the twelve tiles wait for these rows (one round: nothing else to run meanwhile), so the copy is
                // on the edge phase's critical path.  Four loads in flight per lane and ONE wait per 256 pieces (16 rows)
                // instead of a load, a wait and a store per 64 pieces: the flagship's 10 rows took three dependent L2
                // round trips.  Every load is unconditional on a clamped piece (piece 0 exists: np >= 1); the same
                // loads of the same bytes, the same stores.
                for (int base = 0; base < np * 16; base += 256) {
                    u32x4 v[4];
                    int dst[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int idx = base + 64 * j + lane, idc = idx < np * 16 ? idx : 0;
                        int slot = idc >> 4;
                        if (slot >= off) slot += n;
                        const int c = (idc & 15) * 4;
                        v[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (slot * H + c) * 4, 0, 16);   // aux 16 = sc1
                        dst[j] = idx < np * 16 ? slot * LDW + c : -1;
                    }
                    // one wait that the compiler's wait-count pass sees, nothing scheduled across it, every loaded value
                    // named behind it (as the field wave's load block): left alone, the compiler sinks a load whose value
                    // only a predicated store reads into that store's exec-masked region, with a wait of its own
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_waitcnt(0x0F70);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) asm volatile("" :: "v"(v[j]));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4 f;
#pragma unroll
                        for (int r4 = 0; r4 < 4; ++r4) f[r4] = __uint_as_float(v[j][r4]);
                        if (dst[j] >= 0) st4(psb + dst[j], f);
                    }
                }
            } else
            for (int idx = lane; idx < np * 16; idx += 64) {
                int slot = idx >> 4;
                if (slot >= off) slot += n;
                const int c = (idx & 15) * 4;
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (slot * H + c) * 4, 0, 16);   // aux 16 = sc1
                f32x4 f;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) f[r4] = __uint_as_float(v[r4]);
                st4(psb + slot * LDW + c, f);
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // rows are in LDS before the word says so
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) arrived[0] = layer;
            FUSED_WSTAMP(layer, 0, 7);
        };
        auto wait_partner_rows = [&]() {
            while (__builtin_amdgcn_readfirstlane(arrived[0]) < layer) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
        };
        // 12 waves: g = W_e(layer + 1) e of the wave's tile, in place, under this layer's node phase (the image is in wA
        // since the post-edge barrier: dma_ahead).  gemm_split as the tile would run it: same k order, small terms first, same
        // operand scale.  A wave without a tile has nothing to multiply.
        auto early_product = [&]() {
            if (n_tiles > wave) {
                f32x4 g[4];
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) g[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
                gemm_split_paired<4, 2>(wA, e[0], g, lane);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) e[0][mb] = g[mb];
            }
        };
        auto front_act = [&](int r, f32x4 (&acc)[4], f32x4 (&h1)[4], bool last) {
            if (last) issue_loads(1);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) h1[mb] = silu4(acc[mb]);
        };
        auto back = [&](int r, const f32x4 (&h1)[4], bool last) {
            const int tile = NW * r + wave;
            f32x4 acc2[4];
            if (last) issue_loads(2);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc2[mb] = ld4(cb + CB_B2 + 16 * mb + 4 * q);
            gemm_split<4, 2>(wB, h1, acc2, lane);
            if (last) issue_loads(3);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) e[r][mb] = silu4(acc2[mb]);
            if constexpr (KEEP) {
                if (ke[r] >= 0 && dbg.e[layer - 1] != nullptr) {          // (layer 4 under AETHER_FLAG_BACKWARD_ONLY: not kept)
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb)
                        st4(dbg.e[layer - 1] + (int64_t)ke[r] * H + 16 * mb + 4 * q, e[r][mb]);
                }
            }
            // Per-receiver sums of the tile: park the tile in 16 LDS rows (one set per wave, private to it) and read it
            // back by columns -- lane L owns column L and adds its 16 values in row order, every segment from +0.0f, the
            // order and the roundings of the fmaf chain that a product with the 0/1 segment matrix would run.  After the
            // last row of a segment the sum goes to the segment's partial row.  Which rows end a segment and where the
            // sums go is the same for all lanes (seg_ends / seg_rows in scalar registers): the test and the
            // branch run on the scalar unit, and a restart is a move -- a non-finite message never reaches another
            // receiver's sum.
            float* wst = smem + L::WSTAGE + wave * (16 * LDST);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) st4(wst + i * LDST + 16 * mb + 4 * q, e[r][mb]);
            FUSED_WSTAMP(layer, r, 4);
            __builtin_amdgcn_wave_barrier();
            {
                float cv[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) cv[k] = wst[k * LDST + lane];
                float* pcol = part + lane;
                unsigned ends = seg_ends[r];
                // (opaque here: the sixteen bit tests stay one scalar compare each in front of their branch -- hoisted out
                // of the layer loop they become sixteen 64-bit lane masks per round, parked in vector-register lanes)
                asm volatile("" : "+s"(ends));
                unsigned long long lo = (unsigned long long)seg_rows[r][0] | ((unsigned long long)seg_rows[r][1] << 32);
                unsigned long long hi = (unsigned long long)seg_rows[r][2] | ((unsigned long long)seg_rows[r][3] << 32);
                float sum = 0.0f;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    sum += cv[k];
                    if ((ends >> k) & 1u) {
                        pcol[((unsigned)lo & 0xFFu) * LDW] = sum;
                        sum = 0.0f;
                        lo = (lo >> 8) | (hi << 56);
                        hi >>= 8;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (last) issue_loads(4);
        };
        {
            const int nvalid = n_tiles > wave ? (n_tiles - wave + NW - 1) / NW : 0;    // wave-uniform
            if constexpr (EARLY) {
                // W_e(layer + 1) -> wA and constants block layer + 1 -> slot (layer + 1) & 1, a layer ahead (layer 1: with the
                // prologue's DMA).  Safe without a second slot: every read of wA as W_e(layer) -- the products of node phase
                // layer - 1 -- precedes that phase's closing barrier, and so does the last read of the slot, which held block
                // layer - 1 (CB_B1N in step 4).  The receiving wave issues none: its sweep waits vmcnt(0) and would wait for
                // the copy; the other eleven share the 19 fragments whether or not the view is split.  This wave's fragments are
                // its oldest loads in flight: the node phase's prefetch, eight loads per wave, is issued behind them.
                // (in front of the prefetch of a wave without a tile, too)
                if (layer == 2 || layer == 3) {
                    const int recv_wave = GRAN && na >= 16 ? 0 : NW - 1;          // (see below)
                    const int wv = __builtin_amdgcn_readfirstlane(wave);
                    dma_ahead(layer + 1, wv == recv_wave ? -1 : wv - (wv > recv_wave ? 1 : 0), NW - 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (nvalid == 0) {
#pragma unroll
                for (int part = 1; part < 5; ++part) issue_loads(part);
            }
            // Who receives.  Flag protocol: the last wave -- it has the fewest tiles.  Granules: wave 0 when its tile is wholly
            // own-sender (na >= 16), in front of that tile: it needs no rows itself, so every wave that does -- the last
            // one included -- runs its first Linear under the sweep, and wave 0's late tile still ends before theirs.
            // Otherwise (hardly an own sender in the workgroup) the last wave as before.  The receiver is fixed before the
            // tile loop: it receives whether or not it owns a tile (N = 17: 9 tiles on 12 waves), the others wait for it.
            const int recv_wave = GRAN && na >= 16 ? 0 : NW - 1;
            if (xch && wave == recv_wave) receive_partner_rows();
            bool have_rows = !xch || wave == recv_wave;
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) {
                if (r < nvalid) {
                    const bool last = r == nvalid - 1;
                    // a partner sender in this tile (wave-uniform)
                    const bool partner_tile = xch && 16 * (NW * r + wave + 1) > na;
                    // The late add belongs to the workgroups of 9-16 tiles: the 12-wave kernels and the two-tile kernels,
                    // which are compared with them bit for bit.  The one-tile 8-wave kernels keep P_r + P_s in one
                    // rounding and the wait in front of the tile (HISTORY R17); three-tile kernels run unsplit views only.
                    const bool late_tile = LATE && partner_tile;
                    FUSED_WSTAMP(layer, r, 0);
                    if constexpr (!LATE) {
                        if (partner_tile && !have_rows) {
                            wait_partner_rows();
                            have_rows = true;
                        }
                    }
                    FUSED_WSTAMP(layer, r, 1);
                    f32x4 acc[4], h1[4];
                    front_gemm(r, acc, last, late_tile);
                    FUSED_WSTAMP(layer, r, 3);
                    if (late_tile) {
                        if (!have_rows) {      // first tile with a partner sender: the rows are needed from here on
                            wait_partner_rows();
                            have_rows = true;
                        }
                        FUSED_WSTAMP_ROWS(layer, r);
                        late_add(r, acc);
                    }
                    front_act(r, acc, h1, last);
                    FUSED_WSTAMP(layer, r, 2);
                    back(r, h1, last);
                    FUSED_WSTAMP(layer, r, 5);
                }
            }
        }
        FUSED_STAMP(4 + 8 * (layer - 1) + 2);
        // ------------------------------------------------------------ node phase (locs.py:240-241)
        // EARLY: this wave's fragments of W_e(layer + 1) and constants block layer + 1 (dma_ahead, top of the edge phase) have
        // landed: everything but the eight younger loads of the node phase's prefetch, which stay in flight (loads return
        // in order).
        if constexpr (EARLY) __builtin_amdgcn_s_waitcnt(0x0F78);       // vmcnt(8)
        lds_barrier();       // all partial rows are published; wB is idle (12 waves: wA holds W_e(layer + 1) whole already)
        FUSED_STAMP(4 + 8 * (layer - 1) + 3);
        // step 1: n = x_prev + (sum of the node's partial rows, in tile order) / max(deg, 1)
        if (tid < FUSED_MAX_NODES * 16) {
            f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
            const int at0 = arange & 0xFF, at1 = (arange >> 8) & 0xFF, bt0 = (arange >> 16) & 0xFF, bt1 = arange >> 24;
            for (int t = at0; t < at1; ++t) sum += ld4(part + (aslot + t) * LDW + ac4);
            for (int t = bt0; t < bt1; ++t) sum += ld4(part + (aslot + t) * LDW + ac4);
            const f32x4 nv = ld4(xbuf + aslot * LDW + ac4) + sum / adeg;
            st4(nbuf + aslot * LDW + ac4, nv);
            if constexpr (NW == 12) {
                // the one node tile's 16 rows (waves 0-3) also as step 2's B fragments, with the waves' range words
                if (wave < 4) {
                    pieces_store(smem + L::NPC, aslot, tid & 3, (tid & 15) >> 2, nv);
                    range_word_store(smem + L::PFLAG + wave, absmax4(0.0f, nv), lane);
                }
            }
            if (keep && aslot < n) st4(dbg.n[layer - 1] + (int64_t)(nb + aslot) * H + ac4, nv);
        }
        // The wave's W3 / W4 / W_s / W_r fragments have arrived: a wait the compiler's wait-count pass sees (simm16 of
        // vmcnt(0) alone), so that it places none of its own in steps 2-4 -- in particular none behind the LDS-DMA below.
        __builtin_amdgcn_s_waitcnt(0x0F70);
        // next layer's images and constants: in flight under steps 2-4, waited for before step 4's barrier (12 waves: W_e and
        // the constants came a layer ahead, W2 is issued in step 2)
        if constexpr (!EARLY) {
            if (layer < 4) dma_images(layer + 1);
        }
        lds_barrier();       // n complete
        FUSED_STAMP(4 + 8 * (layer - 1) + 7);
        if constexpr (EARLY) {
            // W2(layer + 1) -> wB, which the tiles of this layer read up to the post-edge barrier: issued by the waves that have
            // no row block in step 2, waited for in step 4 (granules) or in front of the closing barrier
            if (layer < 4 && wave >= FUSED_W2DMA_WAVE0) dma_w2(layer + 1, __builtin_amdgcn_readfirstlane(wave) - FUSED_W2DMA_WAVE0);
        }
        // step 2: u = SiLU(W3 n + b3): rows 16*mb2.. of u for both node tiles
        if (act3) {
            float* ubuf = smem + L::UBUF;
            const f32x4 bv = ld4(cb + CB_B3 + 16 * mb2 + 4 * q);
#pragma unroll
            for (int tn = 0; tn < (NW == 12 ? 1 : 2); ++tn) {
                if (16 * tn < n) {
                    if constexpr (NW == 12) {
                        // n comes split from step 1; u goes on to step 3 split, half mb2 >> 2 of its 128 units
                        const f16x8 wh2[2] = {wf_h[0], wf_h[1]}, wl2[2] = {wf_l[0], wf_l[1]};
                        const f32x4 uv = silu4(gemm_pieces_regs(wh2, wl2, smem + L::NPC, smem + L::PFLAG, nbuf + i * LDW + 4 * q, lane, bv));
                        st4(ubuf + i * LDU + 16 * mb2 + 4 * q, uv);
                        pieces_store(smem + L::UPC + (mb2 >> 2) * SPLIT_PIECES, i, q, mb2 & 3, uv);
                        range_word_store(smem + L::PFLAG + 4 + mb2, absmax4(0.0f, uv), lane);
                    } else {
                        f32x4 nv[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) nv[a] = ld4(nbuf + (16 * tn + i) * LDW + 16 * a + 4 * q);
                        const f32x4 acc = gemm_split_regs<2>(w3h, w3l, nv, bv);
                        st4(ubuf + (16 * tn + i) * LDU + 16 * mb2 + 4 * q, silu4(acc));
                    }
                }
            }
        }
        lds_barrier();       // u complete
        FUSED_STAMP(4 + 8 * (layer - 1) + 4);
        if constexpr (EARLY) {
            // waves 0-7 have nothing to do in step 3: their tile's product for the next layer runs here, next to the four
            // waves (8-11) of step 3, and never between a barrier and node-phase work that somebody waits for
            if (layer < 4 && fused_product_step(wave) == 3) {
                FUSED_WSTAMP(layer + 1, 0, 8);
                early_product();
                FUSED_WSTAMP(layer + 1, 0, 9);
            }
        }

        // step 3: x = n + W4 u + b4: rows 16*mb3.. of node tile tn3s (one node tile: on waves 4-7)
        if (do3) {
            const float* ubuf = smem + L::UBUF;
            f32x4 acc = ld4(cb + CB_B4 + 16 * mb3 + 4 * q);
#pragma unroll
            for (int hk = 0; hk < 2; ++hk) {                   // k halves of 64 (each with its own range check): fewer live registers
                if constexpr (NW == 12) {
                    const f16x8 wh2[2] = {wf_h[2 * hk], wf_h[2 * hk + 1]}, wl2[2] = {wf_l[2 * hk], wf_l[2 * hk + 1]};
                    acc = gemm_pieces_regs(wh2, wl2, smem + L::UPC + hk * SPLIT_PIECES, smem + L::PFLAG + 4 + 4 * hk,
                                           ubuf + i * LDU + 64 * hk + 4 * q, lane, acc);
                } else {
                    f32x4 uv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) uv[a] = ld4(ubuf + (16 * tn3s + i) * LDU + 16 * (4 * hk + a) + 4 * q);
                    const f16x8 wh2[2] = {w4h[2 * hk], w4h[2 * hk + 1]}, wl2[2] = {w4l[2 * hk], w4l[2 * hk + 1]};
                    acc = gemm_split_regs<2>(wh2, wl2, uv, acc);
                }
            }
            acc += ld4(nbuf + (16 * tn3s + i) * LDW + 16 * mb3 + 4 * q);
            st4(xbuf + (16 * tn3s + i) * LDW + 16 * mb3 + 4 * q, acc);
            if constexpr (NW == 12) {             // x split for step 4 / the out MLP (waves 8-11 here)
                pieces_store(smem + L::XPC, i, q, mb3, acc);
                range_word_store(smem + L::PFLAG + 12 + mb3, absmax4(0.0f, acc), lane);
            }
            if (keep && 16 * tn3s + i < n)
                st4(dbg.x[layer] + (int64_t)(nb + 16 * tn3s + i) * H + 16 * mb3 + 4 * q, acc);
        }
        lds_barrier();
        FUSED_STAMP(4 + 8 * (layer - 1) + 5);
        // step 4: next layer's node terms P_s = W_s x, P_r = W_r x + b1 (locs.py:233 split)
        if (layer < 4) {
            // granules: the LDS-DMA of the next layer's images and constants (issued in step 1) is waited for HERE, where it
            // has long landed, and not in front of the closing barrier: the granule stores below stay in flight across it
            // (12 waves: W2 alone, issued in step 2 by waves 8-11)
            if constexpr (GRAN) __builtin_amdgcn_s_waitcnt(0x0F70);
            if constexpr (EARLY) {
                // ... and waves 8-11, which ran step 3, have nothing to do in step 4
                if (fused_product_step(wave) == 4) {
                    FUSED_WSTAMP(layer + 1, 0, 8);
                    early_product();
                    FUSED_WSTAMP(layer + 1, 0, 9);
                }
            }
            if (16 * tn4 < n) {
                f32x4 xv[4];
                if constexpr (NW != 12) {         // (12 waves: x comes split from step 3)
#pragma unroll
                    for (int a = 0; a < 4; ++a) xv[a] = ld4(xbuf + (16 * tn4 + i) * LDW + 16 * a + 4 * q);
                }
                if (do_s) {
                    f32x4 accs;
                    if constexpr (NW == 12) {
                        const f16x8 wh2[2] = {wf_h[2], wf_h[3]}, wl2[2] = {wf_l[2], wf_l[3]};
                        accs = gemm_pieces_regs(wh2, wl2, smem + L::XPC, smem + L::PFLAG + 12, xbuf + i * LDW + 4 * q, lane,
                                                f32x4{0.f, 0.f, 0.f, 0.f});
                    } else {
                        accs = gemm_split_regs<2>(wsh, wsl, xv, f32x4{0.f, 0.f, 0.f, 0.f});
                    }
                    if (16 * tn4 + i < n) {      // sender rows live in the visible numbering
                        st4(psb + (off + 16 * tn4 + i) * LDW + 16 * mb3 + 4 * q, accs);
                        float* gps = dbg.ps[layer - 1] + (int64_t)(nb + 16 * tn4 + i) * H + 16 * mb3 + 4 * q;
                        if (GRAN && wg.partner >= 0) {
                            gran_publish(gran_rsrc(dbg.flags, wg.goff, vb, nv), off + 16 * tn4 + i, 16 * mb3 + 4 * q, layer, accs);
                        } else if (wg.partner >= 0) {       // write-through (sc1) payload: no release fence needed
                            // ONE 16-byte sc1 store per lane (aux 16): an 8-byte sc1 store is a fabric write of its
                            // own, 2.7 x the time per byte (MI355X_MICROARCH.md, visibility price list)
                            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
                                dbg.ps[layer - 1] + (int64_t)nb * H, 0, n * H * 4, 0x00020000);
                            u32x4 bits;
#pragma unroll
                            for (int r4 = 0; r4 < 4; ++r4) bits[r4] = __float_as_uint(accs[r4]);
                            __builtin_amdgcn_raw_buffer_store_b128(bits, rsrc, ((16 * tn4 + i) * H + 16 * mb3 + 4 * q) * 4, 0, 16);
                        } else if (keep) {
                            st4(gps, accs);
                        }
                    }
                }
                if (do_r) {
                    f32x4 accr;
                    if constexpr (NW == 12) {
                        const f16x8 wh2[2] = {wf_h[2], wf_h[3]}, wl2[2] = {wf_l[2], wf_l[3]};
                        accr = gemm_pieces_regs(wh2, wl2, smem + L::XPC, smem + L::PFLAG + 12, xbuf + i * LDW + 4 * q, lane,
                                                ld4(cb + CB_B1N + 16 * mb3 + 4 * q));
                    } else {
                        accr = gemm_split_regs<2>(wrh, wrl, xv, ld4(cb + CB_B1N + 16 * mb3 + 4 * q));
                    }
                    st4(prb + (16 * tn4 + i) * LDW + 16 * mb3 + 4 * q, accr);
                    if (keep && 16 * tn4 + i < n)
                        st4(dbg.pr[layer - 1] + (int64_t)(nb + 16 * tn4 + i) * H + 16 * mb3 + 4 * q, accr);
                }
            }
            // First half of the hand-off of the own P_s rows to the partner workgroup
            // (cdna_hip_programming.md Guideline 16, form R1 with write-through payload): every byte of
            // the payload was stored sc1 (16-byte buffer stores above); every wave drains its stores
            // before the barrier, then one lane raises the flag.  The partner picks the rows up after
            // the first GEMM of its next edge phase (receive_partner_rows), as this workgroup does with
            // the partner's: the flag's flight time hides behind those 64 MFMAs.
            // (granules: no drain, no flag -- the stores are on their way, the DMA was waited for above)
            if (!GRAN)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // hand-off stores; LDS-DMA images and constants
            lds_barrier();   // P_s / P_r and the staged weights are visible to the next edge tiles
            if (!GRAN && wg.partner >= 0 && tid == 0)
                __hip_atomic_store(dbg.flags + blockIdx.x, layer, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            FUSED_STAMP(4 + 8 * (layer - 1) + 6);
        }
    }
    if (wg.partner >= 0 && tid == 0)       // the partner's last flag value has been consumed: re-arm it
        __hip_atomic_store(dbg.flags + wg.partner, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (GRAN) {
        // ... and the granules this workgroup consumed: the partner's rows of all three slots, zeroed by the waves that have
        // no stage of the out MLP, under it.  Every one of them was seen with its tag (or the launch has reported an
        // error), so the partner's store of this launch is in memory before this one; the next launch starts behind it.
        if (wg.partner >= 0 && wave >= 8) gran_rearm(gran_rsrc(dbg.flags, wg.goff, vb, nv), nv, n, off, tid - 512, 256);
    }

    // ---------------------------------------------------------------- out MLP + globalise + residual
    // locs.py:160-168,193; local_to_global.py:12-13; aether.py:185
    {
        float* o1 = smem + L::OBUF1;
        float* o2 = smem + L::OBUF2;
        const int mb = wave & 3, tn = NW == 12 ? 0 : (wave >> 2) & 1;
        const bool act = wave < 8 && 16 * tn < n;
        // NW == 12 (one node tile): stage 1 on waves 0-3, which hold out_w0, stage 2 on waves 4-7, which hold out_w3
        const bool act1 = NW == 12 ? wave < 4 && n > 0 : act;
        const bool act2 = NW == 12 ? wave >= 4 && wave < 8 && n > 0 : act;
        const float* cb = cblk;                          // slot 0: block 4 (out_b0, out_b3, out_b6, out_w6)
        if (act1) {
            f32x4 acc;
            if constexpr (NW == 12) {
                const f16x8 wh2[2] = {wf_h[2], wf_h[3]}, wl2[2] = {wf_l[2], wf_l[3]};
                acc = gemm_pieces_regs(wh2, wl2, smem + L::XPC, smem + L::PFLAG + 12, xbuf + i * LDW + 4 * q, lane,
                                       ld4(cb + CB_B1N + 16 * mb + 4 * q));
            } else {
                f32x4 xv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) xv[a] = ld4(xbuf + (16 * tn + i) * LDW + 16 * a + 4 * q);
                acc = gemm_split_regs<2>(wsh, wsl, xv, ld4(cb + CB_B1N + 16 * mb + 4 * q));
            }
            f32x4 v = silu4(acc);
            if constexpr (KEEP) {
                if (dbg.step.drop1 != nullptr && 16 * tn + i < n)
                    v = v * ld4(dbg.step.drop1 + (int64_t)(nb + 16 * tn + i) * H + 16 * mb + 4 * q);
            }
            st4(o1 + (16 * tn + i) * LDW + 16 * mb + 4 * q, v);
            if constexpr (NW == 12) {             // o1 split for stage 2 (waves 0-3 here)
                pieces_store(smem + L::OPC, i, q, mb, v);
                range_word_store(smem + L::PFLAG + 16 + mb, absmax4(0.0f, v), lane);
            }
        }
        if constexpr (KEEP) {
            if (blockIdx.x == 0 && tid == 0 && dbg.step.dropword != nullptr) *dbg.step.dropword = dbg.step.drop1 != nullptr ? 1 : 0;
        }
        lds_barrier();
        if (act2) {
            f32x4 acc;
            if constexpr (NW == 12) {
                const f16x8 wh2[2] = {wf_h[2], wf_h[3]}, wl2[2] = {wf_l[2], wf_l[3]};
                acc = gemm_pieces_regs(wh2, wl2, smem + L::OPC, smem + L::PFLAG + 16, o1 + i * LDW + 4 * q, lane,
                                       ld4(cb + CB_OB3 + 16 * mb + 4 * q));
            } else {
                f32x4 xv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) xv[a] = ld4(o1 + (16 * tn + i) * LDW + 16 * a + 4 * q);
                acc = gemm_split_regs<2>(wrh, wrl, xv, ld4(cb + CB_OB3 + 16 * mb + 4 * q));
            }
            f32x4 v = silu4(acc);
            if constexpr (KEEP) {
                if (dbg.step.drop2 != nullptr && 16 * tn + i < n)
                    v = v * ld4(dbg.step.drop2 + (int64_t)(nb + 16 * tn + i) * H + 16 * mb + 4 * q);
            }
            st4(o2 + (16 * tn + i) * LDW + 16 * mb + 4 * q, v);
        }
        lds_barrier();
        if (wave < 2 && 16 * wave < n) {
            const int tn2 = wave;
            f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                // last Linear: rows >= D of the block are discarded
                const f32x4 w6v = ld4(cb + CB_OW6 + (i < D ? i : D - 1) * H + 16 * a + 4 * q);
                const f32x4 xv = ld4(o2 + (16 * tn2 + i) * LDW + 16 * a + 4 * q);
#pragma unroll
                for (int b = 0; b < 4; ++b) y = mfma16(w6v[b], xv[b], y);
            }
            const int node = 16 * tn2 + i;
            if (q == 0 && node < n) {
                float yl[D];
#pragma unroll
                for (int d = 0; d < D; ++d) yl[d] = y[d] + cb[CB_OB6 + d];
                const float* ni = ninfo + (off + node) * 24;
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    float s = 0.f;
#pragma unroll
                    for (int b = 0; b < D; ++b) s += ni[NI::R + a * D + b] * yl[b];
                    float xn = ni[NI::P + a] + s;
                    if (arrived[1]) xn = __builtin_nanf("");          // a hand-off wait gave up somewhere in this workgroup
                    out[(int64_t)(nb + node) * D + a] = xn;
                    if (dbg.step.vel_out)
                        dbg.step.vel_out[(int64_t)(nb + node) * D + a] = (xn - ni[NI::P + a]) / dbg.step.dt;
                }
            }
        }
    }
    FUSED_STAMP(40);
#ifdef AETHER_FUSED_STAMPS
    if (tid == 0 && blockIdx.x < 4096)      // total cycles, for the clock estimate
        dbg.stamps[blockIdx.x * FUSED_STAMPS + 41] = (float)(__builtin_amdgcn_s_memtime() - c_entry);
#endif
}

}  // namespace
