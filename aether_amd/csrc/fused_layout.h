// fused_layout.h -- k_fused's LDS layout, the weight images and constants blocks it reads, and their preparation
// (split_weights_block: one block of k_prepare_weights, aether_hip.hip).  fused_bwd.h reads the same images.
#pragma once
#include "common.h"

namespace {

constexpr int FUSED_MAX_NODES = 32;          // two 16-node MFMA tiles
constexpr int FUSED_MAX_EDGES = 384;         // 24 tiles (N=20 fully connected: 380 edges)
constexpr int FUSED_MAX_TILES = FUSED_MAX_EDGES / 16;
constexpr int LDU = 2 * H + 8;               // padded LDS row for the 128-wide update hidden
// 12-wave kernels: the layer-1 features of all (at most 12) tiles are built by one wave per SIMD -- waves 0-3, lanes 0-47 --
// each lane the edge below in the workgroup's local order: row lane & 15 of tile 3 wave + (lane >> 4), whose owner is
// wave `tile`.  4 x 48 = 192 edges = the 12 tiles.
constexpr int FUSED_PACK_WAVES = 4, FUSED_PACK_LANES = 48;
__device__ __host__ constexpr int fused_packed_edge(int wave, int lane) { return FUSED_PACK_LANES * wave + lane; }
static_assert(FUSED_PACK_WAVES * FUSED_PACK_LANES == 12 * 16 && FUSED_PACK_LANES % 16 == 0, "every row of the twelve tiles has one builder");
// 12-wave kernels, wave roles of the prologue behind the field waves (waves 0, 1: visible node tiles 0, 1):
//   * wave FUSED_FRAME_WAVE0 + t builds the frames of visible node tile t (R and cv need the velocity alone) while the
//     field wave of that tile runs the field net;
//   * behind the P1 barrier wave FUSED_X0_WAVE0 + mb computes rows 16 mb .. 16 mb + 15 of x0 for every visible node tile
//     that holds own nodes (four row blocks = the 64 rows), while waves 0-3 build the layer-1 features.
constexpr int FUSED_FRAME_WAVE0 = 2, FUSED_X0_WAVE0 = 4, FUSED_X0_WAVES = 4;
__device__ __host__ constexpr int fused_frame_tile(int wave) { return wave - FUSED_FRAME_WAVE0; }       // (a frame wave when 0 <= tile < vtiles)
__device__ __host__ constexpr int fused_x0_rowblock(int wave) { return wave - FUSED_X0_WAVE0; }        // (an x0 wave when 0 <= block < 4)
static_assert(FUSED_FRAME_WAVE0 >= FUSED_MAX_NODES / 16 && FUSED_FRAME_WAVE0 + FUSED_MAX_NODES / 16 <= 12 && FUSED_X0_WAVE0 + FUSED_X0_WAVES <= 12 &&
              FUSED_X0_WAVES * 16 == H, "frame waves behind the field waves, one x0 wave per 16 of the H rows");

// 12-wave kernels, node phase: the window in which a wave multiplies its tile by the next layer's W_e (early_product) --
// step 3's for the waves that have no row block there (0-7), step 4's for the four that run step 3 (8-11).  Those four
// have no row block in step 2 either: they issue the LDS-DMA of the next layer's W2 there.  (Products in step 1's window
// -- waves 4-11 beside the node sums -- or step 2's -- waves 8-11 -- cost 2 us per step: HISTORY R31.)
constexpr int FUSED_STEP3_WAVE0 = 8;
__device__ __host__ constexpr int fused_product_step(int wave) { return wave < FUSED_STEP3_WAVE0 ? 3 : 4; }
constexpr int FUSED_W2DMA_WAVE0 = FUSED_STEP3_WAVE0;

// The edge MLP's two 64 x 64 contractions run as three fp16 MFMA terms on operands split into two fp16 pieces (common.h,
// gemm_split); the weight images (2 x 8 KB each instead of 18 KB of padded fp32) fit every variant since the layer-1 features of the
// 17-24 tile one are built two rounds at a time.
constexpr int FUSED_WIMG = SPLIT_WIMG;                   // floats of a split image of a 64 x 64 matrix (16 KB)
// Per-layer constants block (plain fp32, written by k_prepare_weights next to the images, copied into LDS with them): every
// bias the kernel adds while layer l is in LDS, so that nothing between the node phase's barriers waits for global memory.
constexpr int FUSED_CBLK = 768;                          // floats per layer (3 KiB = three LDS-DMA fragments)
constexpr int CB_B1 = 0;                                 // [64]  bias of the tile's first Linear (layer 1: l1_msg_b0; layers 2-4: zeros)
constexpr int CB_B2 = 64;                                // [64]  b2
constexpr int CB_B3 = 128;                               // [128] b3
constexpr int CB_B4 = 256;                               // [64]  b4
constexpr int CB_B1N = 320;                              // [64]  layers 1-3: next layer's ln_msg_b0 (the P_r bias); layer 4: out_b0
constexpr int CB_OB3 = 384;                              // [64]  layer 4: out_b3
constexpr int CB_OB6 = 448;                              // [4]   layer 4: out_b6, zero padded
constexpr int CB_OW6 = 512;                              // [3][64] layer 4: out_w6 rows 0..D-1; everything else in a block is zero
template <int NW, int ROUNDS> struct FusedLds {          // offsets in floats
    static constexpr int WSZ = FUSED_WIMG;
    static constexpr int WA = 0;                                   // W_e  (layer 1: W1) split image
    static constexpr int WB = WA + WSZ;                            // W2
    static constexpr int CBLK = WB + WSZ;                          // [2][FUSED_CBLK] constants of layer l in slot l & 1
    static constexpr int XBUF = CBLK + 2 * FUSED_CBLK;             // [32][LDW]  x_{l-1} / x_l
    static constexpr int NBUF = XBUF + FUSED_MAX_NODES * LDW;      // [32][LDW]  n = x + mean
    static constexpr int PS = NBUF + FUSED_MAX_NODES * LDW;        // [32][LDW]  W_s x
    static constexpr int PR = PS + FUSED_MAX_NODES * LDW;          // [32][LDW]  W_r x + b1
    static constexpr int NINFO = PR + FUSED_MAX_NODES * LDW;       // [32][24]   NodeInfo records
    // one row per (receiver, tile).  A split workgroup walks its edges in two receiver-sorted runs (own senders,
    // then the partner's: see FusedWG), whose rows are kept apart by an offset of n: 2 * 32 + 16 rows for up to
    // 16 tiles; with 17-24 tiles (ROUNDS == 3) only unsplit workgroups are built: 32 + 24 rows.
    static constexpr int PART_ROWS = ROUNDS == 3 ? FUSED_MAX_NODES + FUSED_MAX_TILES : 2 * FUSED_MAX_NODES + 16;
    static constexpr int PART = NINFO + FUSED_MAX_NODES * 24;      // [PART_ROWS][LDW]  per-(receiver, tile) sums
    static constexpr int ARRIVED = PART + PART_ROWS * LDW;            // [4] ints: split mode, layer whose partner rows are in LDS
    static constexpr int SCRATCH = ARRIVED + 4;                    // aliased by the regions below
    static constexpr int FEAT_ROWS = 16 * (ROUNDS < 2 ? ROUNDS : 2);           // per wave: two rounds of features at a time
    static constexpr int SCRATCH_SIZE =
        NW * FEAT_ROWS * LDF > NW * 16 * LDST ? NW * FEAT_ROWS * LDF : NW * 16 * LDST;
    static constexpr int TOTAL = SCRATCH + SCRATCH_SIZE;
    static constexpr int FIELD_Z = SCRATCH;                            // [32][24]  p | v | emb
    static constexpr int FIELD_H1 = FIELD_Z + FUSED_MAX_NODES * 24;    // [32][32]
    static constexpr int FIELD_H2 = FIELD_H1 + FUSED_MAX_NODES * 32;   // [32][32]
    static constexpr int FIELD_F = FIELD_H2 + FUSED_MAX_NODES * 32;    // [32][4]
    static constexpr int FIELD_W = FIELD_F + FUSED_MAX_NODES * 4;      // field-net parameters (2,080 floats)
    static constexpr int FW0 = FIELD_W;                                // [32][22]
    static constexpr int FW2 = FW0 + 32 * 22;                          // [32][32]
    static constexpr int FW4 = FW2 + 32 * 32;                          // [3][32]
    static constexpr int FB = FW4 + 3 * 32;                            // b0[32] b2[32] b4[4]
    static constexpr int FEMB = FB + 68;                               // [3][16]
    static constexpr int FIELD_END = FEMB + 48;
    static constexpr int FEAT = SCRATCH;                               // [NW waves][FEAT_ROWS][LDF]
    static constexpr int WSTAGE = SCRATCH;                             // [NW waves][16][LDST] tile staging
    static constexpr int UBUF = SCRATCH;                               // [32][LDU]
    static constexpr int OBUF1 = SCRATCH;                              // [32][LDW]
    static constexpr int OBUF2 = SCRATCH + FUSED_MAX_NODES * LDW;      // [32][LDW]
    // 12 waves: the node phase's shared operands (n, u, x, the out MLP's o1) as fp16 pieces in the consumers' B-fragment
    // shape, written by the operand's producer next to the fp32 rows (common.h, pieces_store): u as two 64-unit halves.
    // Behind UBUF / OBUF2 in the part of SCRATCH that only the edge phase's tile staging uses: written and read between
    // the barrier that ends a layer's edge tiles and the one that starts the next layer's, where the staging rows are idle.
    static constexpr int NPC = SCRATCH + (LDU > 2 * LDW ? LDU : 2 * LDW) * FUSED_MAX_NODES;   // [hi | lo][2 k blocks][64 lanes] x 16 bytes
    static constexpr int UPC = NPC + SPLIT_PIECES;                     // [2 halves] of the same
    static constexpr int XPC = UPC + 2 * SPLIT_PIECES;
    static constexpr int OPC = XPC + SPLIT_PIECES;
    static constexpr int PFLAG = OPC + SPLIT_PIECES;                   // [5 operands][4 producing waves] range words (n, u half 0, u half 1, x, o1)
    // 12 waves: layer 1's image A (W1 padded to K = 32, half an image) lies in the P_s rows, which nobody touches before
    // step 4 of layer 1; wA holds W_e(2) from the prologue on.
    static constexpr int W1A = PS;
    static_assert(FUSED_WIMG / 2 <= FUSED_MAX_NODES * LDW && W1A % 256 == 0, "layer 1's image A fits the P_s rows, on a fragment boundary");
    static_assert(NW != 12 || (NPC >= OBUF2 + FUSED_MAX_NODES * LDW && NPC >= UBUF + FUSED_MAX_NODES * LDU && PFLAG + 5 * 4 <= TOTAL && NPC % 4 == 0), "operand pieces");
    static_assert(FIELD_END <= TOTAL, "field scratch");
    static_assert(UBUF + FUSED_MAX_NODES * LDU <= TOTAL, "ubuf");
    static_assert(OBUF2 + FUSED_MAX_NODES * LDW <= TOTAL, "obuf");
    static_assert(TOTAL * 4 <= 160 * 1024, "LDS budget");
};

// Split (2 x fp16) images of the edge-MLP weights in global memory, in the exact order the kernel keeps them in LDS
// (stage_split4): per layer l = 1..4 image A (layer 1: W1 padded to K = 32, FUSED_WIMG / 2 floats; layers 2-4: W_e)
// and image B (W2).  k_prepare_weights (aether_hip.hip) writes them once per weight version; k_fused copies them with LDS-DMA.
// Round 4: the node phase's weights as split images too (its GEMMs moved from the fp32 MFMA to the matrix pipe): per layer
// W3 [128][64] (stage_split4<8, 2>), W4 [64][128] (<4, 4>), and the NEXT layer's W_s, W_r (<4, 2> each; layer 4: out_w0, out_w3).
constexpr int FUSED_NIMG_W3 = 2 * 8 * 2 * 64 * 4, FUSED_NIMG_W4 = 2 * 4 * 4 * 64 * 4, FUSED_NIMG_WS = 2 * 4 * 2 * 64 * 4;
constexpr int FUSED_NIMG_LAYER = FUSED_NIMG_W3 + FUSED_NIMG_W4 + 2 * FUSED_NIMG_WS;
// Field image (12-wave kernels): what the field wave's MFMAs consume of the field net, W_res[:, D:] and their biases --
// fp32, in lane-fragment order (lane = 16 q + i), the k < FIN, i < D and 4q + r < D masks baked in as zeros -- so that the
// wave fetches them as FUSED_FIMG_CHUNKS 16-byte buffer loads per lane (chunk c, lane L: floats 256 c + 4 L ..) instead of
// 42 loads (D = 2), two thirds of them 4-byte gathers with per-lane addresses, and the mask selects behind the wait.  Slot s of a lane is float s & 3 of chunk s >> 2.
// Behind everything else in the set: no other offset moves.
constexpr int FI_ACC1 = 0;                               // [2 mb][4]     field_b0[16 mb + 4q + r]      (accumulator layout)
constexpr int FI_ACC2 = 8;                               // [2 mb][4]     field_b2
constexpr int FI_W2F = 16;                               // [2 mb][2 a][4] field_w2[16 mb + i][16 a + 4q + r]
constexpr int FI_W4F = 32;                               // [2 a][4]      field_w4[i][16 a + 4q + r], i < D
constexpr int FI_ACC3 = 40;                              // [4]           field_b4[4q + r], 4q + r < D
constexpr int FI_ACC0 = 44;                              // [4 mb][4]     l1_res_b[16 mb + 4q + r]
constexpr int FI_A1 = 60;                                // [2 mb][6 s]   field_w0[16 mb + i][4s + q], 4s + q < FIN
constexpr int FI_ZC = 72;                                // [6 s][3 c]    field_emb[c][4s + q - 2D], 2D <= 4s + q < FIN
constexpr int FI_AR = 90;                                // [4 mb][2 s]   l1_res_w[16 mb + i][D + 4s + q], 4s + q < 2D
constexpr int FI_END = 98;
constexpr int FUSED_FIMG_CHUNKS = (FI_END + 3) / 4;      // 25
// 12-wave kernels: x0 is computed behind the P1 barrier by the x0 waves (FUSED_X0_WAVE0 + mb), each of which loads the two
// chunks of its row block -- FI_ACC0 / 4 + mb and the chunk of slots FI_AR + 2 mb, FI_AR + 2 mb + 1 (elements 2, 3 of it for an
// even mb, 0, 1 for an odd one).  The field wave loads the chunks that hold a slot of the field net: 19 of the 25.
static_assert(FI_ACC0 % 4 == 0 && FI_AR % 4 == 2, "an x0 wave's operands: one whole chunk and half of another");
__device__ __host__ constexpr bool fused_fimg_x0_slot(int s) { return (s >= FI_ACC0 && s < FI_A1) || (s >= FI_AR && s < FI_END); }
__device__ __host__ constexpr bool fused_fimg_field_chunk(int c) {
    for (int r = 0; r < 4; ++r)
        if (4 * c + r < FI_END && !fused_fimg_x0_slot(4 * c + r)) return true;
    return false;
}
constexpr int FUSED_FIMG = FUSED_FIMG_CHUNKS * 256;      // floats (25 KiB)
constexpr int FUSED_WIMG_SPLIT = 8 * FUSED_WIMG + 4 * FUSED_NIMG_LAYER + 4 * FUSED_CBLK;   // the split images and constants blocks (layer 1's image A uses half of its slot)
constexpr int FUSED_WIMG_SET = FUSED_WIMG_SPLIT + FUSED_FIMG;   // floats reserved
// blocks of k_prepare_weights that write images (512 threads each): 8 edge images, 24 node images, the constants blocks,
// and one block per chunk of the field image (a thread writes one float: the launch is as long as its longest block, and
// every training step runs it)
constexpr int FUSED_SPLIT_BLOCKS = 8 + 4 * 6 + 1 + FUSED_FIMG_CHUNKS;
__device__ __host__ constexpr int fused_fimg_offset() { return FUSED_WIMG_SPLIT; }
__device__ __host__ constexpr int fused_wimg_offset(int layer, int which) { return ((layer - 1) * 2 + which) * FUSED_WIMG; }
// which: 0 W3, 1 W4, 2 W_s (next layer / out_w0), 3 W_r (next layer / out_w3)
__device__ __host__ constexpr int fused_nimg_offset(int layer, int which) {
    return 8 * FUSED_WIMG + (layer - 1) * FUSED_NIMG_LAYER +
           (which == 0 ? 0 : which == 1 ? FUSED_NIMG_W3 : which == 2 ? FUSED_NIMG_W3 + FUSED_NIMG_W4 : FUSED_NIMG_W3 + FUSED_NIMG_W4 + FUSED_NIMG_WS);
}
__device__ __host__ constexpr int fused_cblk_offset(int layer) { return 8 * FUSED_WIMG + 4 * FUSED_NIMG_LAYER + (layer - 1) * FUSED_CBLK; }

// Float c of layer's constants block (layout: CB_* above).
__device__ __forceinline__ float fused_cblk_value(const AetherParams& P, int nd, int layer, int c) {
    if (c < CB_B2) return layer == 1 ? P.l1_msg_b0[c] : 0.0f;
    if (c < CB_B3) return (layer == 1 ? P.l1_msg_b2 : P.ln_msg_b2[layer - 2])[c - CB_B2];
    if (c < CB_B4) return (layer == 1 ? P.l1_upd_b0 : P.ln_upd_b0[layer - 2])[c - CB_B3];
    if (c < CB_B1N) return (layer == 1 ? P.l1_upd_b2 : P.ln_upd_b2[layer - 2])[c - CB_B4];
    if (c < CB_OB3) return (layer < 4 ? P.ln_msg_b0[layer - 1] : P.out_b0)[c - CB_B1N];
    if (layer < 4) return 0.0f;
    if (c < CB_OB6) return P.out_b3[c - CB_OB3];
    if (c < CB_OB6 + 4) return c - CB_OB6 < nd ? P.out_b6[c - CB_OB6] : 0.0f;
    if (c >= CB_OW6 && c < CB_OW6 + nd * H) return P.out_w6[c - CB_OW6];
    return 0.0f;
}

// Slot `slot` of lane 16 q + i of the field image (layout: FI_* above).  Reads the tensors the 8-wave kernels' field wave
// reads, at the same indices and under the same conditions; a masked element is +0.0f and is not read.
__device__ __forceinline__ float fused_fimg_value(const AetherParams& P, int nd, int slot, int i, int q) {
    const int fin = 2 * nd + 16;
    if (slot < FI_ACC2) return P.field_b0[16 * (slot >> 2) + 4 * q + (slot & 3)];
    if (slot < FI_W2F) return P.field_b2[16 * ((slot - FI_ACC2) >> 2) + 4 * q + (slot & 3)];
    if (slot < FI_W4F) {
        const int s = slot - FI_W2F, mb = s >> 3, a = (s >> 2) & 1;
        return P.field_w2[(16 * mb + i) * 32 + 16 * a + 4 * q + (s & 3)];
    }
    if (slot < FI_ACC3) {
        const int s = slot - FI_W4F;
        return i < nd ? P.field_w4[i * 32 + 16 * (s >> 2) + 4 * q + (s & 3)] : 0.0f;
    }
    if (slot < FI_ACC0) return 4 * q + (slot - FI_ACC3) < nd ? P.field_b4[4 * q + (slot - FI_ACC3)] : 0.0f;
    if (slot < FI_A1) return P.l1_res_b[16 * ((slot - FI_ACC0) >> 2) + 4 * q + (slot & 3)];
    if (slot < FI_ZC) {
        const int s = slot - FI_A1, mb = s / 6, k = 4 * (s % 6) + q;
        return k < fin ? P.field_w0[(16 * mb + i) * fin + k] : 0.0f;
    }
    if (slot < FI_AR) {
        const int s = slot - FI_ZC, c = s % 3, k = 4 * (s / 3) + q;
        return (k >= 2 * nd && k < fin) ? P.field_emb[c * 16 + k - 2 * nd] : 0.0f;
    }
    if (slot < FI_END) {
        const int s = slot - FI_AR, mb = s >> 1, k = 4 * (s & 1) + q;
        return k < 2 * nd ? P.l1_res_w[(16 * mb + i) * 3 * nd + nd + k] : 0.0f;
    }
    return 0.0f;
}

__device__ __forceinline__ void split_weights_block(const AetherParams& P, int f1, int nd, float* __restrict__ wimg, int block, int tid) {
    if (block >= FUSED_SPLIT_BLOCKS - FUSED_FIMG_CHUNKS) {   // the field image: chunk c = 256 floats, float 4 lane + r is slot 4 c + r
        const int c = block - (FUSED_SPLIT_BLOCKS - FUSED_FIMG_CHUNKS), lane = tid >> 2;
        if (tid < 256) wimg[fused_fimg_offset() + 256 * c + tid] = fused_fimg_value(P, nd, 4 * c + (tid & 3), lane & 15, lane >> 4);
        return;
    }
    if (block == FUSED_SPLIT_BLOCKS - FUSED_FIMG_CHUNKS - 1) {   // the four constants blocks
        for (int idx = tid; idx < 4 * FUSED_CBLK; idx += 512)
            wimg[fused_cblk_offset(1) + idx] = fused_cblk_value(P, nd, idx / FUSED_CBLK + 1, idx % FUSED_CBLK);
        return;
    }
    if (block >= 8) {                                     // node-phase images: six blocks per layer
        const int nbk = block - 8, layer = nbk / 6 + 1, part = nbk % 6;
        if (part < 2) {                                   // W3 rows 64 part ..: 1,024 float4
            const float* w3 = layer == 1 ? P.l1_upd_w0 : P.ln_upd_w0[layer - 2];
            float* img = wimg + fused_nimg_offset(layer, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 512 * j, rr = 64 * part + (idx >> 4), cc = (idx & 15) * 4;
                stage_split4<8, 2>(img, rr, cc, ld4(w3 + (size_t)rr * H + cc));
            }
        } else if (part < 4) {                            // W4 [64][128], rows 32 (part - 2) ..
            const float* w4 = layer == 1 ? P.l1_upd_w2 : P.ln_upd_w2[layer - 2];
            float* img = wimg + fused_nimg_offset(layer, 1);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 512 * j, rr = 32 * (part - 2) + (idx >> 5), cc = (idx & 31) * 4;
                stage_split4<4, 4>(img, rr, cc, ld4(w4 + (size_t)rr * (2 * H) + cc));
            }
        } else {                                          // W_s / W_r of the next layer (layer 4: out_w0 / out_w3)
            const float* src = layer < 4 ? P.ln_msg_w0[layer - 1] + (part == 4 ? 0 : H) : (part == 4 ? P.out_w0 : P.out_w3);
            const int ld = layer < 4 ? 3 * H : H;
            float* img = wimg + fused_nimg_offset(layer, part - 2);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int idx = tid + 512 * j, rr = idx >> 4, cc = (idx & 15) * 4;
                stage_split4<4, 2>(img, rr, cc, ld4(src + (size_t)rr * ld + cc));
            }
        }
        return;
    }
    const int layer = block / 2 + 1, which = block & 1;
    float* img = wimg + fused_wimg_offset(layer, which);
    if (which == 0 && layer == 1) {                       // W1 [64][f1] -> K padded to 32: one float4 per thread
        const int r = tid >> 3, c0 = (tid & 7) * 4;
        f32x4 v;
#pragma unroll
        for (int b = 0; b < 4; ++b) v[b] = c0 + b < f1 ? P.l1_msg_w0[r * f1 + c0 + b] : 0.0f;
        stage_split4<4, 1>(img, r, c0, v);
        return;
    }
    const float* src;
    int ld;
    if (which == 0) { src = P.ln_msg_w0[layer - 2] + 2 * H; ld = 3 * H; }             // W_e = W1[:, 128:192]
    else { src = layer == 1 ? P.l1_msg_w2 : P.ln_msg_w2[layer - 2]; ld = H; }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = tid + 512 * j, rr = idx >> 4, cc = (idx & 15) * 4;
        stage_split4<4, 2>(img, rr, cc, ld4(src + (size_t)rr * ld + cc));
    }
}

}  // namespace
