// fused_handoff.h -- the split-mode hand-off of P_s rows as tagged granules (k_fused<D, 12, 1, false, true>).
#pragma once
#include "common.h"

namespace {

// ---------------------------------------------------------------- hand-off as tagged granules (12-wave kernel)
// Split mode, k_fused<D, 12, 1, false, true>: the two workgroups of a group hand their P_s rows over as 8-byte granules
// {tag, fp32 bits} (cdna_hip_programming.md Guideline 16, form R2: "the data IS the flag") -- no flag, no drain of the
// stores, no order between them.  The granule of column c of node g for the hand-off behind layer l (tag l, row l - 1 of
// the node's three) lies at flags + goff + ((3 g + l - 1) * H + c) * 8 in the graph view: zero between launches, written
// once per launch, zeroed again by its reader.  Free functions, called from k_fused<D, 12, 1, false, true> only.
constexpr int GRAN_ROW = H * 8, GRAN_NODE = 3 * GRAN_ROW;      // bytes of one row of granules, of a node's three rows
typedef unsigned int gran_u32x4 __attribute__((ext_vector_type(4)));

// descriptor of the granules of a workgroup's visible nodes [vb, vb + nv) (rows in the numbering of ninfo / psb)
__device__ __forceinline__ auto gran_rsrc(int* flags, int goff, int vb, int nv) {
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(flags) + goff + (int64_t)vb * GRAN_NODE, 0, nv * GRAN_NODE,
                                             0x00020000);
}

// Producer (step 4 of layers 1-3): the lane's four columns c0 .. c0 + 3 of visible row `row` as four granules, two 16-byte
// sc1 stores (the 8-byte halves of such a store land whole: MI355X_MICROARCH.md, visibility).  Nothing waits for them and
// nothing signals them: the partner reads until it sees the tags.
template <class Rsrc>
__device__ __forceinline__ void gran_publish(Rsrc rsrc, int row, int c0, int layer, f32x4 val) {
    const unsigned tag = (unsigned)layer;
    const gran_u32x4 g01 = {tag, __float_as_uint(val[0]), tag, __float_as_uint(val[1])};
    const gran_u32x4 g23 = {tag, __float_as_uint(val[2]), tag, __float_as_uint(val[3])};
    const int voff = row * GRAN_NODE + c0 * 8, soff = (layer - 1) * GRAN_ROW;
    __builtin_amdgcn_raw_buffer_store_b128(g01, rsrc, voff, soff, 16);          // aux 16 = sc1
    __builtin_amdgcn_raw_buffer_store_b128(g23, rsrc, voff + 16, soff, 16);
}

// Consumer (start of the edge phase of layers 2-4), ONE wave: re-read the partner's rows -- the visible rows outside
// [off, off + n) -- of the hand-off behind layer - 1, every 16-byte piece {tag, value, tag, value}, NL pieces per lane, all
// in flight together, ONE wait per pass, until every tag says layer - 1; the pass that finds them all carries the values
// already, and they go to the rows of psb.  sc1 loads, the only loads of those bytes in the launch.  Bounded by TIME like
// the flag poll of the other protocol (5 s of the 100 MHz wall clock) with the same error path: the host-mapped word and
// arrived[1].  Five pieces per lane cover 10 partner rows (every split of N <= 20 but the most uneven); more rows, a
// second sweep.
template <class Rsrc, class LdsWord>
__device__ __forceinline__ void gran_receive(Rsrc rsrc, int layer, int nv, int n, int off, int lane, float* psb,
                                             LdsWord* arrived, int* errword) {
    constexpr int NL = 5;
    const int npieces = (nv - n) * (H / 2);
    const unsigned tag = (unsigned)(layer - 1);
    const int soff = (layer - 2) * GRAN_ROW;
    for (int base = 0; base < npieces; base += 64 * NL) {
        int src[NL];
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            // every load is unconditional on a clamped piece (piece 0 exists: there is a partner row)
            const int idx = base + 64 * j + lane, idc = idx < npieces ? idx : 0;
            int slot = idc >> 5;
            if (slot >= off) slot += n;
            src[j] = slot * GRAN_NODE + (idc & 31) * 16;
        }
        gran_u32x4 v[NL];
        unsigned spins = 0;
        unsigned long long t_first = 0;
        bool gave_up = false;
        for (;;) {
            asm volatile("" ::: "memory");                      // a pass loads again: nothing is carried over from the last one
#pragma unroll
            for (int j = 0; j < NL; ++j) v[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, src[j], soff, 16);   // aux 16 = sc1
            // one wait that the compiler's wait-count pass sees, nothing scheduled across it, every loaded value named behind it
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __builtin_amdgcn_sched_barrier(0);
            bool ok = true;
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                asm volatile("" : "+v"(v[j]));
                ok = ok && v[j][0] == tag && v[j][2] == tag;
            }
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 1023u) == 0) {
                const unsigned long long now = wall_clock64();
                if (t_first == 0) t_first = now;
                if (now - t_first <= 500000000ull) continue;
                // partner not resident: give up, never hang -- and say so (see the flag poll in k_fused)
                if (lane == 0) {
                    if (errword) __hip_atomic_store(errword, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    arrived[1] = 1;
                }
                gave_up = true;
                break;
            }
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            if (base + 64 * j + lane < npieces) {
                const int row = src[j] / GRAN_NODE, c = ((src[j] % GRAN_NODE) >> 4) * 2;
                *reinterpret_cast<f32x2*>(psb + row * LDW + c) = f32x2{__uint_as_float(v[j][1]), __uint_as_float(v[j][3])};
            }
        }
        if (gave_up) break;                                     // no second wait
    }
}

// Re-arm (after the layer-4 edge phase), `nthreads` threads of which this is thread t: zero the granules this workgroup
// consumed -- the partner's rows, all three of a node lie behind one another.  Every one of them was seen with its tag (or
// the launch has reported an error), so the partner's store of this launch is in memory before this one; the next launch
// starts behind it.
template <class Rsrc>
__device__ __forceinline__ void gran_rearm(Rsrc rsrc, int nv, int n, int off, int t, int nthreads) {
    constexpr int PIECES = GRAN_NODE / 16;
    const gran_u32x4 zero = {0u, 0u, 0u, 0u};
    for (int idx = t; idx < (nv - n) * PIECES; idx += nthreads) {
        int slot = idx / PIECES;
        const int piece = idx - slot * PIECES;
        if (slot >= off) slot += n;
        __builtin_amdgcn_raw_buffer_store_b128(zero, rsrc, slot * GRAN_NODE + piece * 16, 0, 16);   // aux 16 = sc1
    }
}

}  // namespace
