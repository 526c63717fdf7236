/*
 * aether_hip.h -- C ABI of libaether_hip.so: the MI355X (gfx950) implementation of
 * the Aether state2state step.
 *
 * The reference has no FFI / plugin registry: the seam of this path is the Python
 * nn.Module surface.  The entry points below are what the
 * build's own nn.Module (aether_amd/nn/state2state/aether.py) binds through ctypes;
 * each one names the reference interface it replaces.  Plain pointers and sizes only:
 * every pointer is a DEVICE pointer (HIP) unless it says "host"; `stream` is a
 * hipStream_t passed as void*.  No call allocates, frees or synchronises except
 * aether_graph_build / aether_graph_build_counting (which synchronise `stream` to report bad
 * indices and to size the fused kernel's groups on the host).
 * All functions return 0 on success, a negative AETHER_E* code on error;
 * aether_last_error() returns a host string for the calling thread's last error.
 *
 * The Python binding (aether_amd/_lib.py) is generated from this file when it is imported: every integer #define, struct and
 * prototype below becomes its ctypes counterpart, and a new entry needs no Python table edit.  The reader is a few regular
 * expressions (aether_amd/_header.py), so the file stays inside the grammar of DESIGN.md section 1; a declaration outside it
 * is an error at import, not a skipped entry.
 */
#ifndef AETHER_HIP_H
#define AETHER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AETHER_OK 0
#define AETHER_EINVAL (-1)   /* bad argument (dims, null pointer, size)       */
#define AETHER_EINDEX (-2)   /* edge index outside [0, n_nodes)               */
#define AETHER_EHIP (-3)     /* a HIP runtime call or kernel launch failed    */
#define AETHER_ESPACE (-4)   /* workspace too small                           */

#define AETHER_HIDDEN 64     /* hidden width the kernels are built for (experiments/lorentz/main.py:42-43) */

/*
 * Parameter pointers, one per tensor of the reference state_dict
 * (nn/state2state/aether.py:143-160, nn/state2state/locs/locs.py:142-225; key list
 * in SURVEY.md 8b).  nn.Linear layout: weight[out][in] row-major, bias[out].
 * The same struct, pointing at gradient buffers, receives the parameter gradients.
 */
typedef struct AetherParams {
    /* field_net.* -- aether.py:108-121 */
    float* field_w0; float* field_b0;       /* [32][2D+16], [32] */
    float* field_w2; float* field_b2;       /* [32][32],    [32] */
    float* field_w4; float* field_b4;       /* [D][32],     [D]  */
    float* field_emb;                       /* [3][16]           */
    /* gnn.layer_1.* -- locs.py:170-178 (only_edge_attr=True) */
    float* l1_msg_w0; float* l1_msg_b0;     /* [64][7D+O+2], [64] */
    float* l1_msg_w2; float* l1_msg_b2;     /* [64][64],     [64] */
    float* l1_res_w;  float* l1_res_b;      /* [64][3D],     [64] */
    float* l1_upd_w0; float* l1_upd_b0;     /* [128][64],    [128] */
    float* l1_upd_w2; float* l1_upd_b2;     /* [64][128],    [64] */
    /* gnn.layer_{2,3,4}.* -- locs.py:179-181 */
    float* ln_msg_w0[3]; float* ln_msg_b0[3];   /* [64][192], [64] */
    float* ln_msg_w2[3]; float* ln_msg_b2[3];   /* [64][64],  [64] */
    float* ln_upd_w0[3]; float* ln_upd_b0[3];   /* [128][64], [128] */
    float* ln_upd_w2[3]; float* ln_upd_b2[3];   /* [64][128], [64] */
    /* gnn.out_mlp.{0,3,6} -- locs.py:160-168 */
    float* out_w0; float* out_b0;           /* [64][64], [64] */
    float* out_w3; float* out_b3;           /* [64][64], [64] */
    float* out_w6; float* out_b6;           /* [D][64],  [D]  */
} AetherParams;

/* Host-side summary of a built graph; filled by aether_graph_build, passed back to aether_forward. */
typedef struct AetherGraphInfo {
    int64_t n_nodes, n_edges;
    int32_t n_groups;          /* > 0: workgroups of the fused kernel (0: streamed path only)      */
    int32_t max_group_nodes;   /* most nodes / in-edges one workgroup owns (<= 32 / <= 384)         */
    int32_t max_group_edges;
    int32_t reserved;          /* bit 0: groups are split over two cooperating workgroups           */
} AetherGraphInfo;

/* aether_forward flags */
#define AETHER_FLAG_KEEP_INTERMEDIATES 1  /* also write nodeinfo, x0..x4, e1..e4 to the workspace */
#define AETHER_FLAG_FORCE_STREAMED 2      /* use the layer-by-layer kernels even for small graphs */
#define AETHER_FLAG_FORCE_FUSED 4         /* fail instead of falling back to the streamed kernels */
/* Accepted and ignored since 0.4: the fused kernel's inter-workgroup hand-off words now live in the `graph` buffer
 * (zeroed by aether_graph_build, re-armed by every launch that used them), so no call zeroes anything and a
 * workspace may be re-purposed freely.  Consequence: two launches that use the SAME graph buffer must not run
 * concurrently (different streams); build a second graph view for that. */
#define AETHER_FLAG_WORKSPACE_REUSED 8
/* The fused kernel multiplies its 64 x 64 layers (edge MLPs, node update, out MLP) as three fp16 matrix-core terms on
 * operands split into two fp16 pieces each, with exact power-of-two rescaling where a wave's activations leave fp16's
 * comfortable range (22 significand bits; parity 1e-5, measured 4e-8: csrc/common.h).  Weights must be below 65,504 in
 * magnitude (beyond: non-finite outputs).  The weights' pieces are prepared by a small kernel in front of every call
 * (workspace region).  Set this flag when `workspace` still holds the pieces written by an earlier call with the SAME
 * parameter values (inference loops, rollouts): that kernel is then skipped.  Never set it after the weights changed. */
#define AETHER_FLAG_WEIGHTS_PREPARED 16
/* With AETHER_FLAG_KEEP_INTERMEDIATES: keep only what aether_backward reads -- the last layer's messages e4 (12 MB at
 * N=20, batch=128; 8.6 GB for a 33.5 M-edge shard) are then not written (aether_debug_fetch("e4") is undefined). */
#define AETHER_FLAG_BACKWARD_ONLY 32
/* Training with dropout_prob > 0 (round 3).  The reference's only Dropout layers follow the two SiLUs of the out MLP
 * (nn/state2state/locs/locs.py:160-168).  The caller draws the masks: float[2][n_nodes][64] of SCALES (0 or 1 / (1 - p)),
 * written at byte offset aether_dropout_mask_offset(n_nodes, n_edges, num_dims) of the training workspace before
 * aether_forward(... AETHER_FLAG_KEEP_INTERMEDIATES | AETHER_FLAG_DROPOUT); aether_backward on the same workspace applies
 * the same masks (a word the forward leaves there says whether it used any).  The module fills them with torch's bernoulli_:
 * the same distribution as nn.Dropout, not its random stream. */
#define AETHER_FLAG_DROPOUT 64
size_t aether_dropout_mask_offset(int64_t n_nodes, int64_t n_edges, int num_dims);

/* Library / build identification (host string, static storage). */
const char* aether_version(void);
const char* aether_last_error(void);

/*
 * Graph preparation: receiver-sorted (CSR) view of an edge index.
 * Replaces what torch_scatter.scatter does implicitly on every call
 * (nn/state2state/locs/locs.py:236-238) with a one-time stable sort by receiver, so
 * that the per-layer mean is a deterministic segmented sum in edge order.
 *   send, recv : int64[E]   edges[0], edges[1] of Aether.forward (aether.py:169)
 *   graph      : device buffer of aether_graph_bytes(E, n_nodes) bytes, filled here
 * It also finds the contiguous node ranges that no edge leaves (whole graphs of a batch) and
 * packs them into groups for the single-launch fused kernel (small graphs only; `info`).
 * Synchronises `stream` (it reports bad indices and sizes the groups on the host); uses
 * temporary host memory.  Returns AETHER_EINDEX if any index is out of range.
 */
size_t aether_graph_bytes(int64_t n_edges, int64_t n_nodes);
/* 1 if (send, recv) is element for element the edge index `graph` was built from, 0 if not, < 0 on error.  One small
 * kernel + a stream synchronisation (a 4-byte flag in host-mapped memory): for callers that rebuild identical index
 * tensors every batch (experiments/lorentz/main.py:211-212) and want to reuse the view without sorting again. */
int aether_graph_matches(const int64_t* send, const int64_t* recv, int64_t n_edges, int64_t n_nodes, const void* graph,
                         void* stream);
int aether_graph_build(const int64_t* send, const int64_t* recv, int64_t n_edges,
                       int64_t n_nodes, void* graph, size_t graph_bytes, AetherGraphInfo* info,
                       void* stream);
/*
 * The same view -- same arguments, same buffer (aether_graph_bytes), same bytes in every region a kernel reads, same
 * `info`, same error codes -- without sorting: for callers whose edge index is new on every call, as the runner's is
 * (experiments/lorentz/main.py:211-212 rebuilds and re-uploads it every batch) and as every batch of kNN scenes is
 * (nn/dynamicvars/aether_dynamicvars.py:559-586).  Receivers and senders are integers below n_nodes: one pass counts
 * them (integer atomics), one workgroup scans the counters, every edge goes to its list, and each list is put into
 * ascending order in LDS, which is the order of the stable sort whatever order the atomics arrived in (csrc/graph_build.h).
 * Six launches in front of the host's group tables and two synchronisations of `stream`.  Falls back to aether_graph_build
 * -- and returns what it returns -- for an empty edge list, for more than 2^20 - 1 nodes, when a node has more than
 * 1,024 in- or out-edges, and under aether_set_option("graph_build", 0).
 */
int aether_graph_build_counting(const int64_t* send, const int64_t* recv, int64_t n_edges, int64_t n_nodes, void* graph,
                                size_t graph_bytes, AetherGraphInfo* info, void* stream);
/* Debug / test access: copies the sorted-position -> original-edge-id map (int32[E]). */
int aether_graph_perm(const void* graph, int64_t n_edges, int64_t n_nodes, int32_t* perm_out,
                      void* stream);

/* Bytes of scratch the forward (and, with keep_for_backward, the backward) needs. */
size_t aether_workspace_bytes(int64_t n_nodes, int64_t n_edges, int num_dims,
                              int keep_for_backward);

/*
 * Forward step: replaces Aether.forward (nn/state2state/aether.py:169-186):
 * field query -> local frames -> edge features -> 4 x (edge MLP, mean by receiver,
 * node update) -> out MLP -> rotate back -> x + pred.
 *   x, vel          : float[n_nodes][D]      positions, velocities
 *   charges         : float[n_nodes]         in {-1, 0, +1}  (aether.py:122-124)
 *   edge_attr_orig  : float[E][2]            [q_i q_j, |x_i - x_j|], ORIGINAL edge order
 *   graph           : from aether_graph_build for this (send, recv)
 *   out             : float[n_nodes][D]
 * `h` of the reference signature is unused by the reference and has no counterpart.
 * Small graphs (info->n_groups > 0) run as ONE kernel launch (csrc/fused.h); anything else runs
 * layer by layer (csrc/streamed.h).  Stream-ordered, re-entrant per (workspace, out) pair.
 */
int aether_forward(const AetherParams* params, int num_dims, int64_t n_nodes, int64_t n_edges,
                   const float* x, const float* vel, const float* charges,
                   const float* edge_attr_orig, const void* graph, const AetherGraphInfo* info,
                   void* workspace, size_t workspace_bytes, float* out, int flags, void* stream);

/*
 * Autoregressive rollout, all on the device: `steps` forward steps back to back,
 *   x_{t+1} = Aether(x_t, v_t),  v_{t+1} = (x_{t+1} - x_t) / dt,
 * with edge_attr_orig = [q_i q_j, |x_i - x_j|] derived inside the kernels from the current positions
 * (the runner's per-batch prep, experiments/lorentz/main.py:243-246) -- the protocol of the
 * "20-step rollout MSE" metric (oracle/aether_oracle.py::rollout restates it).  Replaces a
 * Python loop of model calls, gathers and concatenations (about 2/3 of the time of such a loop at
 * N=20, batch=128) by one kernel launch per step.
 *   x0, vel0   : float[n_nodes][D], state at t = 0 (not modified)
 *   trajectory : float[steps][n_nodes][D], positions x_1 .. x_steps
 *   workspace  : aether_workspace_bytes(n_nodes, n_edges, D, 0) bytes
 *   flags      : AETHER_FLAG_FORCE_* / AETHER_FLAG_WORKSPACE_REUSED as for aether_forward
 * Stream-ordered; capture it in a hipGraph to replay a whole rollout with one launch.
 */
int aether_rollout(const AetherParams* params, int num_dims, int64_t n_nodes, int64_t n_edges,
                   const float* x0, const float* vel0, const float* charges, const void* graph,
                   const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                   float* trajectory, int steps, float dt, int flags, void* stream);

/*
 * Backward step: gradients of a scalar loss w.r.t. every parameter, given grad_out = dL/d(out).
 * Replaces torch.autograd through Aether.forward (the runner's loss.backward(),
 * experiments/lorentz/main.py:289-291).  Inputs (x, vel, charges, edge attributes) are data and
 * receive no gradient, as in the runner (main.py:243-247 detaches them).
 *   The forward on the same `workspace` must have run with AETHER_FLAG_KEEP_INTERMEDIATES and a
 *   workspace of aether_workspace_bytes(..., keep_for_backward = 1) bytes.
 *   grads : AetherParams whose pointers address the gradient buffers (same shapes as params);
 *           every element is overwritten (not accumulated).
 * Deterministic (ordered partial sums, no atomics).  Stream-ordered.
 */
int aether_backward(const AetherParams* params, const AetherParams* grads, int num_dims, int64_t n_nodes,
                    int64_t n_edges, const float* x, const float* vel, const float* charges,
                    const void* graph, const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                    const float* grad_out, void* stream);

/*
 * Test hook: copy one named intermediate of the last aether_forward on `workspace`
 * (the fused path writes them only under AETHER_FLAG_KEEP_INTERMEDIATES)
 * into `dst` (device).  Names: "field"[n][D] "canon"[n][2D] (= rel_feat[:, D:]) "R"[n][D*D] "x0".."x4"[n][64]
 * "e1".."e4"[E][64] (receiver-sorted order; map back with aether_graph_perm).
 * Returns the number of floats written, or a negative error.
 */
int64_t aether_debug_fetch(const char* name, int num_dims, int64_t n_nodes, int64_t n_edges,
                           const void* workspace, float* dst, void* stream);

/*
 * Test hook of the fp16 split that every split GEMM of the library shares (csrc/common.h: split_scale_of, split8).
 * x = n_tiles tiles of [16 rows][64] floats (device).  One workgroup of 12 waves (three per SIMD) runs, per tile, the range
 * test and the 64 x 64 split GEMM against a fixed weight image, each wave beside the other waves' MFMAs, and writes
 *   hi, lo [n_tiles][16][64]  bit patterns of the fp16 pieces of s * x,   on, scale [n_tiles]  the decision and s,
 *   y [n_tiles][16][64]       the product.
 * Launches on the null stream.  Returns AETHER_OK or a negative error.
 */
int aether_debug_split(const float* x, int n_tiles, uint16_t* hi, uint16_t* lo, int* on, float* scale, float* y);

/*
 * Test hook: what the host chose for the dense-layer tables and the edge filter of the seq2seq steps since the last reset.
 * Kinds of a table's launch: 0 the fp32 job kernel (k_s2s_linear_jobs), 1 k_s2s_gemm_split<1> (64-row tiles), 2 <2> (128-row
 * tiles), 3 k_s2s_gemm_split_r1<1>, 4 k_s2s_gemm_split_r1<2>.  Per kind: launches, jobs, and the largest N, M, K, K2 of a job.
 * The first AETHER_S2S_LAUNCH_LOG launches are also kept one by one, in order: `N`, `M`, `K`, `K2` of the job with the largest
 * N * M (the one the tiling is chosen for), `min_n` the fewest rows of a job, `images` whether every job could run on the
 * split kernels (a prepared image for every weight, M a multiple of 128, K and K2 of 32), `tiles64` the sum of
 * ceil(N / 64) * ceil(M / 128) the switch is decided by, `wg128` the sum of ceil(N / 128) * (M / 128) the tile height is
 * decided by (0 unless the table went split), `wgs` the launch's workgroups.  filter_*: launches of k_s2s_filter_split with
 * splits == 1 and with more, and the largest splits.  Plain host integers, updated when a launch is issued: they mean nothing
 * for the replays of a captured graph, and are not synchronised between host threads.
 */
#define AETHER_S2S_LAUNCH_KINDS 5
#define AETHER_S2S_LAUNCH_LOG 96
typedef struct AetherS2SLaunchRecord {
    int32_t kind, jobs, images, M, K, K2, wgs, reserved;
    int64_t N, min_n, tiles64, wg128;
} AetherS2SLaunchRecord;
typedef struct AetherS2SLaunchStats {
    int64_t launches[AETHER_S2S_LAUNCH_KINDS], jobs[AETHER_S2S_LAUNCH_KINDS];
    int64_t max_n[AETHER_S2S_LAUNCH_KINDS], max_m[AETHER_S2S_LAUNCH_KINDS], max_k[AETHER_S2S_LAUNCH_KINDS],
        max_k2[AETHER_S2S_LAUNCH_KINDS];
    int64_t filter_one, filter_many, filter_max_splits;
    int64_t logged;                                    /* launches since the reset; min(logged, LOG) records are valid */
    AetherS2SLaunchRecord log[AETHER_S2S_LAUNCH_LOG];
} AetherS2SLaunchStats;
int aether_s2s_launch_stats(AetherS2SLaunchStats* stats);   /* copies the block out; AETHER_EINVAL for a null pointer */
void aether_s2s_launch_stats_reset(void);

/*
 * Test hook of the 12-wave fused kernels' layer-1 feature build (csrc/fused_layout.h: fused_packed_edge): the edge, in the
 * workgroup's local order, whose features lane `lane` of wave `wave` builds, or -1 for a (wave, lane) that builds none.
 * Edge f is row f & 15 of tile f >> 4, which wave f >> 4 owns.  Host only: needs no GPU.
 */
int aether_debug_fused_packed_edge(int wave, int lane);

/*
 * Test hook of the 12-wave fused kernels' wave roles behind the field waves (csrc/fused_layout.h), wave in 0 .. 11:
 *   what 0  the visible node tile whose frames the wave builds (fused_frame_tile), or -1;
 *   what 1  the 16-row block of x0 the wave computes behind the prologue's barrier (fused_x0_rowblock), or -1;
 *   what 3  the step of the node phase in whose window the wave multiplies its tile by the next layer's W_e
 *           (fused_product_step): 3 or 4;
 *   what 4  layout, not a role: bytes of layer 1's weight image A (wave 0) and of the P_s rows that hold it (wave 1).
 * Host only: needs no GPU.
 */
int aether_debug_fused_wave_role(int what, int wave);

/*
 * Dynamic-field variant of the state2state model: DynamicFieldAether.forward
 * (nn/state2state/dynamic_field_aether.py:79-100) = aether_dynamic_field (LatentFieldNetwork, :31-48:
 * attention-pooled graph summary + FiLM field net, hidden 32) followed by aether_forward_field, i.e.
 * aether_forward with the per-node field supplied instead of the built-in field net (params->field_* are
 * not read for the result but must point to readable memory of the documented sizes).
 *   graphs are consecutive blocks of nodes_per_graph nodes (x.reshape(-1, num_nodes, .), :38);
 *   field : float[n_nodes][D]
 */
typedef struct AetherDynFieldParams {
    const float* gate_w0; const float* gate_b0; const float* gate_w2; const float* gate_b2;   /* [32][2D],[32],[1][32],[1] */
    const float* nn_w0; const float* nn_b0; const float* nn_w2; const float* nn_b2;           /* [32][2D],[32],[32][32],[32] */
    const float* lin1_w; const float* lin1_b; const float* lin2_w; const float* lin2_b;       /* [32][2D+16],[32],[32][32],[32] */
    const float* lin3_w; const float* lin3_b;                                                 /* [D][32],[D] */
    const float* film1_w0; const float* film1_b0; const float* film1_w2; const float* film1_b2;
    const float* film1_w4; const float* film1_b4;                                             /* [32][32] x2, [64][32] */
    const float* film2_w0; const float* film2_b0; const float* film2_w2; const float* film2_b2;
    const float* film2_w4; const float* film2_b4;
    const float* emb;                                                                         /* [3][16] */
} AetherDynFieldParams;
int aether_dynamic_field(const AetherDynFieldParams* params, int num_dims, int64_t n_graphs, int nodes_per_graph,
                         const float* x, const float* vel, const float* charges, float* field, void* stream);
int aether_forward_field(const AetherParams* params, int num_dims, int64_t n_nodes, int64_t n_edges,
                         const float* x, const float* vel, const float* charges, const float* field,
                         const float* edge_attr_orig, const void* graph, const AetherGraphInfo* info,
                         void* workspace, size_t workspace_bytes, float* out, int flags, void* stream);
/*
 * aether_rollout for the dynamic-field model: every step runs aether_dynamic_field on the current state (into
 * field_scratch, float[n_nodes][D]) and then the step with that field; otherwise as aether_rollout.
 */
int aether_rollout_dynamic_field(const AetherParams* params, const AetherDynFieldParams* dyn_params, int num_dims,
                                 int64_t n_nodes, int64_t n_edges, int nodes_per_graph, const float* x0,
                                 const float* vel0, const float* charges, const void* graph,
                                 const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                                 float* field_scratch, float* trajectory, int steps, float dt, int flags, void* stream);
/*
 * Gradients with respect to the INPUTS of the step (round 3) -- the reference's forward is differentiable in x / vel
 * (nn/state2state/aether.py:169-186).  Call after aether_backward, on the same workspace (it reads what that call left:
 * dL/d(layer-1 edge features), dL/dn_1, dL/df and the out MLP's last input o2, from which y of x + R(v) y is formed) with
 * `out` = the forward's output (kept in the signature; no longer read) and the same grad_out:
 *   grad_x [n_nodes][D], grad_vel [n_nodes][D] (overwritten); grad_edge_attr [n_edges][2] in the caller's edge order, or
 *   NULL.  field_input_grad = NULL: the built-in field net (its input gradient is recomputed from dL/df).  For a step that
 *   ran through aether_forward_field: after aether_backward_field, float[n_nodes][2D] = dL/d[x | vel] THROUGH the external
 *   field, e.g. from aether_dynamic_field_backward_inputs below.  Positions and velocities enter through
 *   x + R(v) y, the field net's inputs, rel_feat = [0 | R^T v | R^T f] and the local-frame edge features (r, Euler angles
 *   of R_i^T R_j, distance, bearing, R_i^T v_j, R_i^T f_j); charges are an index (no gradient).
 */
int aether_backward_inputs(const AetherParams* params, int num_dims, int64_t n_nodes, int64_t n_edges, const float* x,
                           const float* vel, const float* charges, const void* graph, const AetherGraphInfo* info,
                           void* workspace, size_t workspace_bytes, const float* out, const float* grad_out, float* grad_x,
                           float* grad_vel, float* grad_edge_attr, const float* field_input_grad, void* stream);

/*
 * Training of the dynamic-field variant.  aether_backward_field = aether_backward for a step that ran through
 * aether_forward_field with AETHER_FLAG_KEEP_INTERMEDIATES: gradients of the GNN / res / out-MLP tensors into
 * `grads` (grads->field_* are not written) and dL/dfield into grad_field [n_nodes][D].
 * aether_dynamic_field_backward then differentiates LatentFieldNetwork (dynamic_field_aether.py:31-48: FiLM field
 * net, FiLM modulators, attention pooling): `grads` holds one output pointer per tensor of `params`;
 * workspace: aether_dynamic_field_backward_workspace_bytes(num_dims, n_graphs) bytes (one partial gradient row per
 * graph, added over the graphs in order: no atomics).
 */
int aether_backward_field(const AetherParams* params, const AetherParams* grads, int num_dims, int64_t n_nodes,
                          int64_t n_edges, const float* x, const float* vel, const float* charges,
                          const void* graph, const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                          const float* grad_out, float* grad_field, void* stream);
size_t aether_dynamic_field_backward_workspace_bytes(int num_dims, int64_t n_graphs);
int aether_dynamic_field_backward(const AetherDynFieldParams* params, const AetherDynFieldParams* grads, int num_dims,
                                  int64_t n_graphs, int nodes_per_graph, const float* x, const float* vel,
                                  const float* charges, const float* grad_field, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* The same, and grad_field_inputs [n_nodes][2D] (or NULL) = dL/d[x | vel] through the field: the FiLM net's first Linear and
 * the graph summary's nn / gate_nn (every node's row enters its graph's attention pooling).  Feed it to
 * aether_backward_inputs(field_input_grad). */
int aether_dynamic_field_backward_inputs(const AetherDynFieldParams* params, const AetherDynFieldParams* grads, int num_dims,
                                         int64_t n_graphs, int nodes_per_graph, const float* x, const float* vel,
                                         const float* charges, const float* grad_field, void* workspace,
                                         size_t workspace_bytes, float* grad_field_inputs, void* stream);

/*
 * Any hidden_size (round 4).  The reference builds Aether / DynamicFieldAether with whatever `--nf` says
 * (experiments/lorentz/main.py:42-43,143; nn/state2state/aether.py:143-158, nn/state2state/locs/locs.py:142-181): every
 * [64]-sized dimension of AetherParams above becomes [hidden], [128] becomes [2 hidden], [192] becomes [3 hidden].
 * The calls below are the calls above with the width as an argument:
 *   hidden == 64        : exactly the functions above (fused / streamed 64-wide kernels);
 *   hidden == 64 m > 64 : layer-by-layer on one generic split-operand (2 x fp16) MFMA GEMM kernel with fused epilogues (csrc/wide.h);
 *   other widths        : not accepted here -- zero-pad the parameters to the next multiple of 64 (padded channels stay
 *                         exactly zero through SiLU, the mean and the residuals; the Python module does this).
 * `field` (forward) / `grad_field` (backward) may be NULL (the built-in field net) or the external field of
 * aether_forward_field / aether_backward_field.  Workspaces are sized by aether_workspace_bytes_h; the dropout masks are
 * float[2][n_nodes][hidden] at aether_dropout_mask_offset_h.  aether_debug_fetch_h reads a KEEP_INTERMEDIATES workspace.
 */
size_t aether_workspace_bytes_h(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden, int keep_for_backward);
size_t aether_dropout_mask_offset_h(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden);
int aether_forward_h(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                     const float* x, const float* vel, const float* charges, const float* field,
                     const float* edge_attr_orig, const void* graph, const AetherGraphInfo* info,
                     void* workspace, size_t workspace_bytes, float* out, int flags, void* stream);
int aether_backward_h(const AetherParams* params, const AetherParams* grads, int num_dims, int hidden, int64_t n_nodes,
                      int64_t n_edges, const float* x, const float* vel, const float* charges, const void* graph,
                      const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* grad_out,
                      float* grad_field, void* stream);
int aether_backward_inputs_h(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                             const float* x, const float* vel, const float* charges, const void* graph,
                             const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* out,
                             const float* grad_out, float* grad_x, float* grad_vel, float* grad_edge_attr,
                             const float* field_input_grad, void* stream);
int aether_rollout_h(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges, const float* x0,
                     const float* vel0, const float* charges, const void* graph, const AetherGraphInfo* info,
                     void* workspace, size_t workspace_bytes, float* trajectory, int steps, float dt, int flags,
                     void* stream);
int aether_rollout_dynamic_field_h(const AetherParams* params, const AetherDynFieldParams* dyn_params, int num_dims,
                                   int hidden, int64_t n_nodes, int64_t n_edges, int nodes_per_graph, const float* x0,
                                   const float* vel0, const float* charges, const void* graph, const AetherGraphInfo* info,
                                   void* workspace, size_t workspace_bytes, float* field_scratch, float* trajectory,
                                   int steps, float dt, int flags, void* stream);
int64_t aether_debug_fetch_h(const char* name, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                             const void* workspace, float* dst, void* stream);

/*
 * Training through the device rollout: a k-step ("push-forward") loss and its backward through time.  Replaces a Python
 * loop of differentiable module calls with the runner's tensor ops in between (the per-batch prep and the
 * loss.backward() of experiments/lorentz/main.py:243-247,289-291, repeated per step and stitched together by autograd;
 * oracle/aether_oracle.py::rollout restates the protocol) by two library calls:
 *   x_{t+1} = Aether(x_t, v_t, ea_t),  ea_t = [q_i q_j, |x_i - x_j|] from x_t,  v_{t+1} = (x_{t+1} - x_t) / dt,  t = 0..steps-1.
 * The 64-wide engine only, on both its paths (fused and streamed); hidden > 64 returns AETHER_EINVAL.
 *
 * aether_rollout_train_forward -- experiments/lorentz/main.py:243-247 per step, oracle rollout: the arguments of
 *   aether_rollout_h; writes trajectory[steps][n_nodes][D] = x_1 .. x_steps and keeps, per step, what the backward reads
 *   (the AETHER_FLAG_KEEP_INTERMEDIATES | AETHER_FLAG_BACKWARD_ONLY layout, edge attributes derived in the kernels) and the
 *   step's input velocity in that step's own slice of `workspace`
 *   (aether_rollout_train_workspace_bytes(n_nodes, n_edges, num_dims, hidden, steps) bytes; 0 for sizes it refuses).
 *   flags: AETHER_FLAG_FORCE_STREAMED / AETHER_FLAG_FORCE_FUSED; no dropout masks.  Everything derived from the weights is
 *   prepared once per call.
 * aether_rollout_backward -- experiments/lorentz/main.py:289-291 through all steps, autograd through the oracle's rollout:
 *   given grad_trajectory[steps][n_nodes][D] = dL/dx_1 .. dL/dx_steps of the caller's loss, on the workspace and trajectory
 *   of the forward, writes
 *     grads    : AetherParams of destinations, OVERWRITTEN with dL/dtheta summed over the steps (step steps-1 first, a fixed
 *                order: the same bits on every run);
 *     grad_x0  : dL/dx_0 [n_nodes][D], grad_vel0 : dL/dv_0 [n_nodes][D]; either may be NULL.
 *   Per step: aether_backward, aether_backward_inputs and one chain launch that forms the next-earlier step's grad_out
 *   from g, gx, gv of this and the later step and the distance term of ea (a fixed-order sum over each node's in- and
 *   out-edge lists: no float atomics) and adds the step's parameter gradients (csrc/rollout_bwd.h).
 *   The call CONSUMES the workspace (a step's temporaries are laid over the later steps' kept intermediates, which it
 *   has finished with: the workspace grows per step by what a forward keeps, not by a whole training workspace): one
 *   aether_rollout_backward per aether_rollout_train_forward.
 *   Exactly coincident end points of an edge (distance 0, self loops included) are UNDEFINED: the distance has no
 *   derivative there.
 * Both are stream-ordered and capturable in a hipGraph: no synchronisation, no allocation.  Entry checks (null pointers,
 * info mismatch, steps < 1, dt == 0, a short workspace -> AETHER_ESPACE) run before anything is queued.
 */
size_t aether_rollout_train_workspace_bytes(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden, int steps);
int aether_rollout_train_forward(const AetherParams* params, int num_dims, int hidden, int64_t n_nodes, int64_t n_edges,
                                 const float* x0, const float* vel0, const float* charges, const void* graph,
                                 const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, float* trajectory,
                                 int steps, float dt, int flags, void* stream);
int aether_rollout_backward(const AetherParams* params, const AetherParams* grads, int num_dims, int hidden, int64_t n_nodes,
                            int64_t n_edges, const float* x0, const float* vel0, const float* charges, const void* graph,
                            const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* trajectory,
                            const float* grad_trajectory, float* grad_x0, float* grad_vel0, int steps, float dt, void* stream);
/*
 * The same for the dynamic-field model (nn/state2state/dynamic_field_aether.py:79-100 as the step): the protocol, the
 * contract and the checks of the two entries above, with the latent field recomputed from (x_t, v_t) every step as in
 * aether_rollout_dynamic_field -- the training forward writes the trajectory of that call, bit for bit.  Further checks:
 * dyn_params and every pointer inside dyn_grads non-null, 1..2048 nodes per graph, n_nodes a multiple of nodes_per_graph.
 *   forward, step t : aether_dynamic_field on (x_t, v_t), then the kept step with that field (one launch more than above).
 *   backward, step t: the step's backward with dL/dfield (aether_backward_field), the field net's backward on it
 *                     (recomputed from x_t, v_t: no field is kept per step) giving dL/d[x | v] through the field, the
 *                     input gradients with that term folded in (aether_backward_inputs(field_input_grad)), the chain
 *                     launch as above: one launch more per step, and one per call --
 *   dyn_grads       : OVERWRITTEN with the 27 field-net gradients summed over the steps.  The sum over the steps runs in
 *                     the per-graph partial rows (each entry owned by one thread, step steps-1 first), the sum over the
 *                     graphs once per call: no float atomics, the same bits on every run.
 *   grads           : as above; grads->field_* (the built-in field net, bypassed) are not written.
 * workspace: aether_rollout_dynamic_field_train_workspace_bytes(...) bytes = that of the entries above + one partial row
 * per graph + three per-node buffers (field, dL/dfield, dL/d[x | v]); 0 for sizes the entries refuse.
 */
size_t aether_rollout_dynamic_field_train_workspace_bytes(int64_t n_nodes, int64_t n_edges, int num_dims, int hidden,
                                                          int nodes_per_graph, int steps);
int aether_rollout_dynamic_field_train_forward(const AetherParams* params, const AetherDynFieldParams* dyn_params, int num_dims,
                                               int hidden, int64_t n_nodes, int64_t n_edges, int nodes_per_graph,
                                               const float* x0, const float* vel0, const float* charges, const void* graph,
                                               const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                                               float* trajectory, int steps, float dt, int flags, void* stream);
int aether_rollout_dynamic_field_backward(const AetherParams* params, const AetherDynFieldParams* dyn_params,
                                          const AetherParams* grads, const AetherDynFieldParams* dyn_grads, int num_dims,
                                          int hidden, int64_t n_nodes, int64_t n_edges, int nodes_per_graph, const float* x0,
                                          const float* vel0, const float* charges, const void* graph,
                                          const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                                          const float* trajectory, const float* grad_trajectory, float* grad_x0,
                                          float* grad_vel0, int steps, float dt, void* stream);

/*
 * seq2seq Aether, field query: replaces Aether.predict_field
 * (nn/seq2seq/aether.py:86-90) = FourierFeatureMapper (nn/nn/fourier_feature_mapper.py:7-21) followed by
 * field_net (aether.py:72-78).  Unlike the state2state field it sees positions only.
 *   B      : float[D][hidden/2]    buffer coordinate_embedding.B
 *   w0..b4 : field_net.{0,2,4}.{weight,bias}: [h][h],[h],[h][h],[h],[D][h],[D]
 *   x      : float[n_points][x_stride], the first D columns are the coordinates (x[..., :D], :87)
 *   field  : float[n_points][D]
 *   workspace : aether_s2s_field_workspace_bytes(n_points, hidden) bytes
 * Stream-ordered; four launches (features, three Linear layers on the matrix core).
 */
typedef struct AetherS2SFieldParams {
    const float* B;
    const float* w0; const float* b0;
    const float* w2; const float* b2;
    const float* w4; const float* b4;
} AetherS2SFieldParams;
size_t aether_s2s_field_workspace_bytes(int64_t n_points, int hidden);
int aether_s2s_field(const AetherS2SFieldParams* params, int num_dims, int hidden, int64_t n_points,
                     const float* x, int x_stride, void* workspace, size_t workspace_bytes, float* field,
                     void* stream);

/*
 * seq2seq Aether, augmented local frames: replaces AugmentedLocalizer.forward
 * (nn/utils/augmented_global_to_local.py:52-68; canonicalize_augmented_inputs and
 * create_augmented[_3d]_edge_attr_pos_vel, nn/utils/canonicalization.py:33-56,111-172) on a flattened
 * batch: nodes of all graphs in one array, edges as global node indices (no out-of-range check).
 *   x         : float[n_nodes][3D]           pos | vel | force
 *   send/recv : int64[n_edges]               edge j -> i, features in i's frame
 *   polar     : 1 = pos_representation 'polar', 0 = 'cart' (columns picked for edge_pos, :19-24)
 *   rel_feat  : float[n_nodes][7D+O]         canonical state | features of the edge from the virtual origin node
 *   Rinv      : float[n_nodes][D][D]         un-transposed frame, as the reference returns it
 *   edge_attr : float[n_edges][2(4D+O)+3D]   edge features | rel_feat[recv]      (24 | 39 columns)
 *   edge_pos  : float[n_edges][D+O]
 * O = D(D-1)/2.  Stream-ordered; two launches.
 */
int aether_s2s_localize(int num_dims, int64_t n_nodes, int64_t n_edges, const float* x,
                        const int64_t* send, const int64_t* recv, int polar, float* rel_feat,
                        float* Rinv, float* edge_attr, float* edge_pos, void* stream);

/*
 * seq2seq Aether, one step of the recurrent decoder (decoder half): replaces
 * RecurrentDecoder.forward (nn/seq2seq/aether.py:590-654) on a flattened batch -- messages from the
 * hidden states and from the present local-frame features per edge type, mean by receiver, GRU-style gate,
 * output MLP, rotate back (Globalizer, nn/utils/local_to_global.py:7-13), residual.
 *   params     : pointers to the reference module's tensors (nn.Linear layout weight[out][in]);
 *                index k of the arrays = edge type k (at most 4)
 *   inputs     : float[n_nodes][2D]  pos | vel          hidden_in : float[n_nodes][h]
 *   edge_w     : float[n_edges][K]   edge-type weights (one-hot or soft; `edges` of the reference)
 *   field      : float[n_nodes][D]   predicted field (aether_s2s_field)
 *   send, recv : int64[n_edges]      global node indices, messages j -> i
 *   order, rowptr : int64[n_edges], int64[n_nodes + 1]  edges grouped by receiver (stable), CSR offsets
 *   outputs    : float[n_nodes][2D]  hidden_out : float[n_nodes][h]  (may not alias hidden_in)
 *   workspace  : aether_s2s_decoder_workspace_bytes(D, h, n_nodes, n_edges) bytes
 * Dropout is 0 (the reference forces it to 0 outside training, aether.py:594).  Stream-ordered.
 */
typedef struct AetherS2SDecoderParams {
    const float* msg_fc1_w[4]; const float* msg_fc1_b[4];    /* [h][2h] (receiver | sender halves), [h] */
    const float* msg_fc2_w[4]; const float* msg_fc2_b[4];    /* [h][h], [h] */
    const float* hidden_r_w; const float* hidden_i_w; const float* hidden_h_w;      /* [h][h], no bias */
    const float* present_r_w; const float* present_r_b;
    const float* present_i_w; const float* present_i_b;
    const float* present_n_w; const float* present_n_b;      /* [h][h], [h] */
    const float* out0_w; const float* out0_b; const float* out3_w; const float* out3_b;   /* [h][h], [h] */
    const float* out6_w; const float* out6_b;                /* [2D][h], [2D] */
    const float* pmsg_fc1_w[4]; const float* pmsg_fc1_b[4];  /* [h][2(4D+O)+3D], [h] */
    const float* pmsg_fc2_w[4]; const float* pmsg_fc2_b[4];  /* [h][h], [h] */
    const float* input_r_w; const float* input_r_b;
    const float* input_i_w; const float* input_i_b;
    const float* input_n_w; const float* input_n_b;          /* [h][7D+O], [h] */
} AetherS2SDecoderParams;
size_t aether_s2s_decoder_workspace_bytes(int num_dims, int hidden, int64_t n_nodes, int64_t n_edges);
int aether_s2s_decoder_step(const AetherS2SDecoderParams* params, int num_dims, int hidden, int num_edge_types,
                            int skip_first, int64_t n_nodes, int64_t n_edges, const float* inputs,
                            const float* hidden_in, const float* edge_w, const float* field,
                            const int64_t* send, const int64_t* recv, const int64_t* order,
                            const int64_t* rowptr, void* workspace, size_t workspace_bytes, float* outputs,
                            float* hidden_out, void* stream);

/*
 * seq2seq Aether, one step of the encoder's prior (prior half): replaces
 * Encoder.single_step_forward (nn/seq2seq/aether.py:384-410) on a flattened batch -- local frames,
 * anisotropic edge filter (nn/nn/anisotropic_filter.py:34-40; the [E, R h] filter bank is never
 * materialised), edge2node / res1, mlp3, node2edge + skip, mlp4 (RefNRIMLP in eval mode: BatchNorm with
 * running statistics, nn/utils/model_utils.py:15-55), one LSTM step per edge, prior_fc_out.
 *   params  : the reference Encoder's tensors (nn.Linear / nn.LSTM layouts; gate order i, f, g, o)
 *   inputs  : float[n_nodes][2D]   field : float[n_nodes][D]   h0, c0 : float[n_edges][rnn_hidden]
 *   send, recv, order, rowptr : as for aether_s2s_decoder_step;  num_vars = objects per graph (edge2node
 *                               divides by num_vars - 1, aether.py:348)
 *   logits  : float[n_edges][K]    h1, c1 : float[n_edges][rnn_hidden]
 *   workspace : aether_s2s_prior_workspace_bytes(...) bytes
 * aether_s2s_gumbel_hard: gumbel_softmax(hard=True) of nn/utils/model_utils.py:58-118 with the uniform
 * draw U[n_edges][K] supplied by the caller (the reference draws it with torch.rand on the host).
 */
typedef struct AetherS2SPriorParams {
    const float* mlp3_w0; const float* mlp3_b0; const float* mlp3_w3; const float* mlp3_b3;       /* [h][h] */
    const float* mlp3_bn_w; const float* mlp3_bn_b; const float* mlp3_bn_mean; const float* mlp3_bn_var;
    const float* mlp4_w0; const float* mlp4_b0; const float* mlp4_w3; const float* mlp4_b3;       /* [h][3h], [h][h] */
    const float* mlp4_bn_w; const float* mlp4_bn_b; const float* mlp4_bn_mean; const float* mlp4_bn_var;
    const float* lstm_w_ih; const float* lstm_w_hh; const float* lstm_b_ih; const float* lstm_b_hh; /* [4R][h], [4R][R] */
    const float* prior_w[4]; const float* prior_b[4];                                            /* prior_fc_out */
    const float* res1_w; const float* res1_b;                                                    /* [h][7D+O] */
    const float* filt_w0; const float* filt_b0;                                                  /* [h][D+O] */
    const float* filt_w2; const float* filt_b2;                                                  /* [R h][h], R = 2(4D+O)+3D */
    const void* filt_image;   /* aether_s2s_filter_prepare(filt_w2, R, h, ..) of the CURRENT filt_w2 values, or NULL: the
                                 step then builds the image in its workspace on every call (reads all of filt_w2) */
} AetherS2SPriorParams;
/*
 * The filter GEMM (anisotropic_filter.py:34-40) runs on the matrix cores as three fp16 terms on operands split into two
 * fp16 pieces each, scaled by exact powers of two (22 significand bits: fp32-equivalent at the 1e-5 bar); its
 * weight operand is a re-ordered two-piece image of filt_w2 (4 bytes per weight + a 256-byte trailer holding max |filt_w2|,
 * from which the scale is derived).  Prepare it once per weight version (three small launches on `stream`):
 *   image : device buffer of aether_s2s_filter_image_bytes(n_features, hidden) bytes, 16-byte aligned
 */
size_t aether_s2s_filter_image_bytes(int n_features, int hidden);
int aether_s2s_filter_prepare(const float* filt_w2, int n_features, int hidden, void* image, size_t image_bytes,
                              void* stream);
size_t aether_s2s_prior_workspace_bytes(int num_dims, int hidden, int rnn_hidden, int prior_hidden,
                                        int64_t n_nodes, int64_t n_edges);
int aether_s2s_prior_step(const AetherS2SPriorParams* params, int num_dims, int hidden, int rnn_hidden,
                          int prior_layers, int prior_hidden, int num_edge_types, int polar, int num_vars,
                          int64_t n_nodes, int64_t n_edges, const float* inputs, const float* field,
                          const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                          const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                          float* logits, float* h1, float* c1, void* stream);
int aether_s2s_gumbel_hard(const float* logits, const float* uniform, float tau, int num_edge_types,
                           int64_t n_edges, float* edges, void* stream);
/*
 * The pieces of aether_s2s_prior_step on their own, for the full-sequence encoder (Encoder.forward,
 * nn/seq2seq/aether.py:350-382: the same per-time-step features, then a forward and a reverse LSTM over time and the two
 * heads prior_fc_out / encoder_fc_out):
 *   aether_s2s_encoder_features : everything up to mlp4 (:354-369) -> features float[n_edges][hidden]; workspace as for
 *                                 aether_s2s_prior_step (aether_s2s_prior_workspace_bytes with any rnn / prior sizes)
 *   aether_s2s_lstm_step        : one nn.LSTM cell step on n_rows rows (gate order i, f, g, o); gates: scratch
 *                                 float[n_rows][4 rnn_hidden]
 *   aether_s2s_mlp_head         : Linear (- ELU - Linear)* as prior_fc_out / encoder_fc_out build it (:286-300); w, b: HOST
 *                                 arrays of `layers` device pointers; scratch float[2][n_rows][hidden_size] when layers > 1
 */
int aether_s2s_encoder_features(const AetherS2SPriorParams* params, int num_dims, int hidden, int polar, int num_vars,
                                int64_t n_nodes, int64_t n_edges, const float* inputs, const float* field,
                                const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                                void* workspace, size_t workspace_bytes, float* features, void* stream);
int aether_s2s_lstm_step(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int in_size,
                         int rnn_hidden, int64_t n_rows, const float* x, const float* h0, const float* c0, float* gates,
                         float* h1, float* c1, void* stream);
int aether_s2s_mlp_head(const float* const* w, const float* const* b, int layers, int in_size, int hidden_size,
                        int out_size, int64_t n_rows, const float* x, float* scratch, float* out, void* stream);

/*
 * The whole autoregressive step in one call: field query -> prior step -> hard Gumbel sample -> decoder
 * step, nn/seq2seq/aether.py:176-185 (= predict_field :86-90, Encoder.single_step_forward :384-410, gumbel_softmax
 * :92-98, RecurrentDecoder.forward :590-654), ~31 launches instead of the ~75 of the four entry points above: dense
 * layers that are independent of each other share a launch, the gate pre-activations are K-concatenated products, the
 * local frames are built once for prior and decoder, and everything derived from the weights alone comes from a PLAN:
 *   aether_s2s_plan_build : filter image, padded input layers, BatchNorm affines, concatenated gate weights / summed gate
 *                           biases, summed LSTM biases, two-piece fp16 images of the dense layers (used from 2 K rows on; `field` may be
 *                           NULL when every step will be given ext_field, otherwise pass the field net the steps will use) -> plan (device, 256-byte aligned, aether_s2s_plan_bytes); rebuild after the weights change
 *   aether_s2s_step       : inputs [n_nodes][2D], decoder_hidden_in [n_nodes][hd], h0 / c0 [n_edges][rnn], uniform
 *                           [n_edges][K] (the U(0,1) draw of gumbel_softmax) -> outputs, decoder_hidden_out, h1, c1 and,
 *                           when edges_out is not NULL, the sampled edge types [n_edges][K].  ext_field != NULL replaces the
 *                           built-in field query by a given field [n_nodes][D] (the dynamic-field model); field params may
 *                           then be NULL.  Graph arrays as for aether_s2s_prior_step.
 *   aether_s2s_rollout    : the loop of predict_future (:166-185) on the device: burn_in_steps teacher-forced steps on
 *                           burn_in [burn_in_steps][n_nodes][2D] (predictions discarded), then `steps` autoregressive steps
 *                           from `inputs`; predictions [steps][n_nodes][2D], edges_out [steps][n_edges][K] or NULL; uniform
 *                           [burn_in_steps + steps][n_edges][K]; decoder_state [n_nodes][hd], h, c are read at entry and hold the final
 *                           state at exit.
 * Results equal the four separate calls up to the rounding of re-associated sums (gate biases are added once, as a sum).
 */
size_t aether_s2s_plan_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                             int prior_hidden, int num_edge_types);
int aether_s2s_plan_build(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                          const AetherS2SDecoderParams* decoder, int num_dims, int encoder_hidden, int decoder_hidden,
                          int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, void* plan,
                          size_t plan_bytes, void* stream);
size_t aether_s2s_step_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                       int num_edge_types, int64_t n_nodes, int64_t n_edges);
int aether_s2s_step(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior, const AetherS2SDecoderParams* decoder,
                    const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                    int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                    int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                    const float* inputs, const float* ext_field, const float* decoder_hidden_in, const float* h0,
                    const float* c0, const float* uniform, void* workspace, size_t workspace_bytes, float* outputs,
                    float* decoder_hidden_out, float* h1, float* c1, float* edges_out, void* stream);
int aether_s2s_rollout(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior, const AetherS2SDecoderParams* decoder,
                       const void* plan, int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                       int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau, int64_t n_nodes,
                       int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                       int burn_in_steps, const float* burn_in, int steps, const float* inputs, float* decoder_state, float* h,
                       float* c, const float* uniform, void* workspace, size_t workspace_bytes, float* predictions,
                       float* edges_out, void* stream);

/*
 * The charge-aware seq2seq Aether, AetherCharges of nn/seq2seq/ablations/aether_charges.py (the model the electrostatic runner
 * passes charges= to): the seq2seq Aether whose field query (:88-98), encoder (:368-432) and recurrent decoder (:615-680) also
 * see emb[c], a 16-wide nn.Embedding(2, 16) of every particle's charge sign (:86, charge_to_index :100-102).  The entries are
 * aether_s2s_plan_* / aether_s2s_step / aether_s2s_rollout with the same stages and launches per step; the parameter structs
 * are the plain model's with the widened tensors of the reference:
 *   field->w0 [he][he + 16]; prior->res1_w [he][7D + O + 16], prior->filt_w2 [(EA + 32) he][he], prior->filt_b2 [(EA + 32) he]
 *   (EA = 2 (4D + O) + 3D); decoder->pmsg_fc1_w[k] [hd][EA + 32], decoder->input_{r,i,n}_w [hd][7D + O + 16].
 * The embedding has two rows, so what it feeds is folded into tables when the plan is built (exact algebra, re-associated
 * fp32 sums): a Linear over [features | emb[c]] adds one of 2 bias rows per node (b + W_c emb[c]; the gates' rows carry the
 * sum of their biases), over [features | emb[c_recv] | emb[c_send]] one of 4 rows per edge; the 32 embedding features of the
 * anisotropic filter become four one-hot features (recv 0 / 1, send 0 / 1) whose weight blocks are sum_j emb[c][j] block_j,
 * so the filter GEMM runs on EA + 4 = 28 / 43 features, not 56 / 71.
 *   aether_s2s_charges_plan_build      : charge_embedding float[2][16] (charge_embedding.weight) and the structs above -> plan
 *                                        (device, 256-byte aligned, aether_s2s_charges_plan_bytes); rebuild after the weights change
 *   aether_s2s_charges_workspace_bytes : of a step / rollout (aether_s2s_step_workspace_bytes + index arrays and edge rows)
 *   aether_s2s_charges_step / _rollout : as aether_s2s_step / aether_s2s_rollout (replacing single_step_forward :104-113 with
 *                                        predict_field and Encoder.single_step_forward, and the loop of predict_future :169-208)
 *                                        with charge_index int32[n_nodes] = charge_to_index(charges), 0 or 1 per node.
 *                                        _step with ext_logits [n_edges][K] != NULL (then ext_field too) is the decoder on given
 *                                        logits, single_step_forward :104-113 as calculate_loss :147-149 calls it: the sample
 *                                        is taken from them, the prior is skipped, h0 / c0 / h1 / c1 may be NULL
 *   aether_s2s_charges_encoder_features: the per-time-step half of Encoder.forward (:371-389: local frames, filter on the folded
 *                                        image, res1 with its table, mlp3, mlp4) on a flattened batch of (time, graph) items with
 *                                        their field -> features [n_edges][he], the input of aether_s2s_lstm_step / _mlp_head;
 *                                        workspace as for a step
 *   aether_s2s_charges_field           : predict_field alone (:88-98) on n_points rows x [n_points][x_stride] with a charge
 *                                        index each -> field [n_points][D]; workspace aether_s2s_charges_field_workspace_bytes
 * A charge index outside {0, 1} reads no table out of bounds: that node's outputs are NaN (in a rollout the NaN spreads
 * through its graph, never to another graph) and the asynchronous error word is set -- the next aether_check_async_error
 * returns AETHER_EHIP -- as for the other inputs the library can only find inconsistent on the device.
 */
size_t aether_s2s_charges_plan_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                     int prior_hidden, int num_edge_types);
int aether_s2s_charges_plan_build(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                                  const AetherS2SDecoderParams* decoder, const float* charge_embedding, int num_dims,
                                  int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                  int num_edge_types, void* plan, size_t plan_bytes, void* stream);
size_t aether_s2s_charges_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                          int num_edge_types, int64_t n_nodes, int64_t n_edges);
int aether_s2s_charges_step(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                            const AetherS2SDecoderParams* decoder, const void* plan, int num_dims, int encoder_hidden,
                            int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                            int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges,
                            const int32_t* charge_index, const int64_t* send, const int64_t* recv, const int64_t* order,
                            const int64_t* rowptr, const float* inputs, const float* ext_field, const float* ext_logits,
                            const float* decoder_hidden_in, const float* h0, const float* c0, const float* uniform,
                            void* workspace, size_t workspace_bytes,
                            float* outputs, float* decoder_hidden_out, float* h1, float* c1, float* edges_out, void* stream);
int aether_s2s_charges_rollout(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                               const AetherS2SDecoderParams* decoder, const void* plan, int num_dims, int encoder_hidden,
                               int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                               int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges,
                               const int32_t* charge_index, const int64_t* send, const int64_t* recv, const int64_t* order,
                               const int64_t* rowptr, int burn_in_steps, const float* burn_in, int steps, const float* inputs,
                               float* decoder_state, float* h, float* c, const float* uniform, void* workspace,
                               size_t workspace_bytes, float* predictions, float* edges_out, void* stream);
int aether_s2s_charges_encoder_features(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                                        const AetherS2SDecoderParams* decoder, const void* plan, int num_dims, int encoder_hidden,
                                        int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                                        int polar, int num_vars, int64_t n_nodes, int64_t n_edges, const int32_t* charge_index,
                                        const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                                        const float* inputs, const float* field_values, void* workspace, size_t workspace_bytes,
                                        float* features, void* stream);
size_t aether_s2s_charges_field_workspace_bytes(int64_t n_points, int hidden);
int aether_s2s_charges_field(const AetherS2SFieldParams* field, const void* plan, int num_dims, int encoder_hidden,
                             int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                             int64_t n_points, const float* x, int x_stride, const int32_t* charge_index, void* workspace,
                             size_t workspace_bytes, float* field_out, void* stream);

/*
 * seq2seq Aether with decoder_type 'ref_mlp': one step of the Markov decoder (MarkovDecoder, nn/seq2seq/aether.py:413-503,
 * with MLPEdgeFilter of nn/nn/anisotropic_filter.py:43-71) on a flattened batch -- local frames of [inputs | field]
 * (AugmentedLocalizer, polar), edge MLP relu(lin2(relu(lin1(edge_attr)))) whose output column c Ku + k is channel c of used
 * type k (Ku = K - skip_first), messages sum_k out[e][c Ku + k] edge_w[e][k0 + k], receiver mean, + res1(rel_feat), output MLP,
 * rotate back, residual.  There is no hidden state (get_initial_hidden returns None, :456-457).
 *   params    : the reference module's tensors (nn.Linear layout weight[out][in])
 *   inputs    : float[n_nodes][2D]   edge_w : float[n_edges][K] (one-hot or soft)   field : float[n_nodes][D]
 *   send, recv, order, rowptr : as for aether_s2s_decoder_step
 *   outputs   : float[n_nodes][2D]
 *   workspace : aether_s2s_markov_decoder_workspace_bytes(D, h, n_nodes, n_edges) bytes
 * Each type's second layer runs on the edges whose weight for it is not zero; the [n_edges][h Ku] output is never formed.
 * Dropout is 0 (inference).  Stream-ordered.
 */
typedef struct AetherS2SMarkovParams {
    const float* lin1_w; const float* lin1_b;    /* edge_filter.lin1: [h][2(4D+O)+3D], [h] */
    const float* lin2_w; const float* lin2_b;    /* edge_filter.lin2: [h Ku][h], [h Ku] (row c Ku + k: channel c of type k) */
    const float* res1_w; const float* res1_b;    /* res1: [h][7D+O], [h] */
    const float* out0_w; const float* out0_b; const float* out3_w; const float* out3_b;   /* out_mlp.0 / .3: [h][h], [h] */
    const float* out6_w; const float* out6_b;    /* out_mlp.6: [2D][h], [2D] */
} AetherS2SMarkovParams;
size_t aether_s2s_markov_decoder_workspace_bytes(int num_dims, int hidden, int64_t n_nodes, int64_t n_edges);
int aether_s2s_markov_decoder_step(const AetherS2SMarkovParams* params, int num_dims, int hidden, int num_edge_types,
                                   int skip_first, int64_t n_nodes, int64_t n_edges, const float* inputs,
                                   const float* edge_w, const float* field, const int64_t* send, const int64_t* recv,
                                   const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                                   float* outputs, void* stream);
/*
 * The whole autoregressive step with the Markov decoder, as aether_s2s_plan_* / aether_s2s_step / aether_s2s_rollout for the
 * recurrent one (aether.py:176-185 with MarkovDecoder.forward :459-503): the same field query -> prior step -> hard Gumbel
 * sample (one shared implementation), then the Markov decoder on the sample's per-type edge lists -- each edge costs one
 * h x h product of its own type, scaled by its actual weight ((1 - y) + y) -- and no decoder state.  lin1 and res1 share the
 * launch of the prior's res1 layer.  The plan holds the prior's prepared weights and the Markov ones (padded lin1 / res1,
 * lin2's bias per type, fp16 x 2 images of lin2's per-type blocks and of out_mlp's hidden layers).
 *   workspace : aether_s2s_step_workspace_bytes(D, he, hd, R, prior_hidden, K, n_nodes, n_edges) bytes
 *   aether_s2s_markov_rollout: burn_in_steps steps on burn_in run the prior only (their predictions are discarded, so the
 *   decoder is skipped; their uniform rows are consumed all the same), then `steps` autoregressive steps; h, c as for
 *   aether_s2s_rollout.
 */
size_t aether_s2s_markov_plan_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                    int prior_hidden, int num_edge_types, int skip_first);
int aether_s2s_markov_plan_build(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                                 const AetherS2SMarkovParams* decoder, int num_dims, int encoder_hidden, int decoder_hidden,
                                 int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first,
                                 void* plan, size_t plan_bytes, void* stream);
int aether_s2s_markov_step(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                           const AetherS2SMarkovParams* decoder, const void* plan, int num_dims, int encoder_hidden,
                           int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                           int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges,
                           const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                           const float* inputs, const float* ext_field, const float* h0, const float* c0,
                           const float* uniform, void* workspace, size_t workspace_bytes, float* outputs, float* h1,
                           float* c1, float* edges_out, void* stream);
int aether_s2s_markov_rollout(const AetherS2SFieldParams* field, const AetherS2SPriorParams* prior,
                              const AetherS2SMarkovParams* decoder, const void* plan, int num_dims, int encoder_hidden,
                              int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                              int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges,
                              const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                              int burn_in_steps, const float* burn_in, int steps, const float* inputs, float* h, float* c,
                              const float* uniform, void* workspace, size_t workspace_bytes, float* predictions,
                              float* edges_out, void* stream);

/*
 * seq2seq dynamic-field variant: nn/seq2seq/dynamic_field_aether.py, the model
 * scripts/gravitational_field_3d_aether.sh trains (use_charges is never set by a runner: False).
 *
 * aether_s2s_graph_summary replaces GraphSummary.forward (nn/nn/graph_pool.py:50-71), run once per
 * sequence on the burn-in trajectories (dynamic_field_aether.py:214-218): particle embedding, a GRU over
 * time per object, [x | last hidden] + sinusoidal positional encoding (:10-28, eval mode: no dropout), and
 * torch_geometric's AttentionalAggregation over all (object, time) items of a graph
 * (softmax = exp(g - max) / (sum + 1e-16)).
 *   x       : float[batch][num_objects][timesteps][input_size]
 *   params  : nn.Linear / nn.GRU layouts (gates r, z, n); pe = buffer `pe.pe` [pe_len][input_size + hidden]
 *   summary : float[batch][hidden]
 * aether_s2s_film_modulation: the four FiLM modulators of FilmedNetwork (nn/nn/film.py:43-60) applied to the
 * summary: mod = gamma_1 | beta_1 | gamma_2 | beta_2, each [batch][mlp_hidden] (+ one scratch plane);
 * the summary is fixed for a sequence, so this also runs once.
 * aether_s2s_film_field replaces predict_field (dynamic_field_aether.py:117-134): Fourier features, then
 * linear_1 - FiLM - SiLU - linear_2 - FiLM - SiLU - linear_3 (nn/nn/filmed_network.py:27-35); point n belongs
 * to graph n / rows_per_graph.
 */
typedef struct AetherS2SGraphSummaryParams {
    const float* emb_w; const float* emb_b;                     /* particle_embedding [H][in], [H] */
    const float* gru_w_ih; const float* gru_w_hh;               /* rnn.weight_{ih,hh}_l0 [3H][H] */
    const float* gru_b_ih; const float* gru_b_hh;               /* [3H] */
    const float* pe;                                            /* [pe_len][in + H] */
    const float* gate_w0; const float* gate_b0; const float* gate_w2; const float* gate_b2;  /* [H][in+H], [H], [1][H], [1] */
    const float* nn_w0; const float* nn_b0; const float* nn_w2; const float* nn_b2;          /* [H][in+H], [H], [H][H], [H] */
} AetherS2SGraphSummaryParams;
size_t aether_s2s_graph_summary_workspace_bytes(int64_t batch, int num_objects, int timesteps, int input_size,
                                                int hidden);
int aether_s2s_graph_summary(const AetherS2SGraphSummaryParams* params, int64_t batch, int num_objects,
                             int timesteps, int input_size, int hidden, int pe_len, const float* x,
                             void* workspace, size_t workspace_bytes, float* summary, void* stream);

typedef struct AetherS2SFilmParams {
    const float* B;                                             /* coordinate_embedding.B [D][h/2] */
    const float* lin1_w; const float* lin1_b;                   /* [mh][h] */
    const float* lin2_w; const float* lin2_b;                   /* [mh][mh] */
    const float* lin3_w; const float* lin3_b;                   /* [D][mh] */
    /* film_{1,2}.{gamma,beta}.{0,2}: [mh][gh], [mh], [mh][mh], [mh]; index = 2 * (film - 1) + (beta ? 1 : 0) */
    const float* mod_w0[4]; const float* mod_b0[4]; const float* mod_w2[4]; const float* mod_b2[4];
} AetherS2SFilmParams;
size_t aether_s2s_film_modulation_bytes(int64_t batch, int mlp_hidden);
int aether_s2s_film_modulation(const AetherS2SFilmParams* params, int graph_hidden, int mlp_hidden, int64_t batch,
                               const float* summary, float* mod, size_t mod_bytes, void* stream);
size_t aether_s2s_film_field_workspace_bytes(int64_t n_points, int hidden, int mlp_hidden);
int aether_s2s_film_field(const AetherS2SFilmParams* params, int num_dims, int hidden, int mlp_hidden,
                          int64_t n_points, int64_t rows_per_graph, const float* x, int x_stride,
                          const float* mod, int64_t batch, void* workspace, size_t workspace_bytes,
                          float* field, void* stream);

/*
 * The fused step and the device rollout of the dynamic-field model: aether_s2s_plan_* / aether_s2s_step / aether_s2s_rollout
 * (and their Markov counterparts) with the FiLM field query as the step's built-in field source.  They replace the per-step
 * predict_field call (nn/seq2seq/dynamic_field_aether.py:117-134) and the loop of predict_future (:207-246): per step, the
 * Fourier features, linear_1 and linear_2 as jobs of the step's dense-layer launches with FiLM and SiLU in their epilogues
 * (linear_1 shares the launch of the decoder's first-layer products), linear_3 in the node kernel of the local frames.
 * One set of entries serves both decoders: exactly one of `decoder` (RecurrentDecoder) and `markov` (MarkovDecoder) is not
 * NULL.  Arguments are those of aether_s2s_step / aether_s2s_rollout, and:
 *   film        : the FiLM net's tensors; the modulators (mod_*) are not read: they are not part of the step
 *   mlp_hidden  : width of linear_1 / linear_2, a multiple of 16 (a multiple of 128: the plan holds their fp16 x 2 images)
 *   mod         : gamma_1 | beta_1 | gamma_2 | beta_2, each [batch][mlp_hidden], as aether_s2s_film_modulation wrote it for
 *                 this sequence's graph summary; mod_bytes >= aether_s2s_film_modulation_bytes(batch, mlp_hidden).  Not part
 *                 of the plan: passed per call, so a captured graph follows a buffer that is rewritten in place.
 *   batch, num_objects : node n belongs to graph n / num_objects; n_nodes must equal batch * num_objects
 *   aether_s2s_dynfield_plan_bytes        : 0 for sizes the step does not take or unless exactly one decoder is given (only
 *                                           whether `decoder` / `markov` are NULL is looked at); skip_first counts for the
 *                                           Markov decoder only
 *   aether_s2s_dynfield_plan_build        : as aether_s2s_plan_build / aether_s2s_markov_plan_build; rebuild after the weights
 *                                           of the encoder, the decoder, linear_1 / linear_2 or coordinate_embedding change
 *   aether_s2s_dynfield_step_workspace_bytes : aether_s2s_step_workspace_bytes with hidden rows of the field query
 *                                           max(encoder_hidden, mlp_hidden) wide
 *   aether_s2s_dynfield_step              : decoder_hidden_in / _out are NULL with the Markov decoder; ext_field != NULL replaces
 *                                           the built-in query; field_out (NULL or [n_nodes][D]) receives the field the
 *                                           built-in query computed
 *   aether_s2s_dynfield_rollout           : decoder_state is NULL with the Markov decoder, whose burn-in steps run the prior only;
 *                                           burn_in_field (NULL or [burn_in_steps][n_nodes][D]): the field of the burn-in
 *                                           frames from ONE aether_s2s_film_field call over all of them (they are known
 *                                           before the loop starts), instead of a query inside each burn-in step
 * AETHER_EINVAL: a NULL mod, n_nodes != batch * num_objects, mlp_hidden not a multiple of 16, both or neither decoder;
 * AETHER_ESPACE: mod_bytes or workspace_bytes too small.  Stream-ordered, no host synchronisation (capturable).
 */
size_t aether_s2s_dynfield_plan_bytes(const AetherS2SDecoderParams* decoder, const AetherS2SMarkovParams* markov, int num_dims,
                                      int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                      int prior_hidden, int num_edge_types, int skip_first, int mlp_hidden);
int aether_s2s_dynfield_plan_build(const AetherS2SFilmParams* film, const AetherS2SPriorParams* prior,
                                   const AetherS2SDecoderParams* decoder, const AetherS2SMarkovParams* markov, int num_dims,
                                   int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                   int num_edge_types, int skip_first, int mlp_hidden, void* plan, size_t plan_bytes,
                                   void* stream);
size_t aether_s2s_dynfield_step_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden,
                                                int prior_hidden, int num_edge_types, int mlp_hidden, int64_t n_nodes,
                                                int64_t n_edges);
int aether_s2s_dynfield_step(const AetherS2SFilmParams* film, const AetherS2SPriorParams* prior,
                             const AetherS2SDecoderParams* decoder, const AetherS2SMarkovParams* markov, const void* plan,
                             int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                             int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                             int64_t n_nodes, int64_t n_edges, int mlp_hidden, const float* mod, size_t mod_bytes, int64_t batch,
                             int num_objects, const int64_t* send, const int64_t* recv, const int64_t* order,
                             const int64_t* rowptr, const float* inputs, const float* ext_field, const float* decoder_hidden_in,
                             const float* h0, const float* c0, const float* uniform, void* workspace, size_t workspace_bytes,
                             float* outputs, float* decoder_hidden_out, float* h1, float* c1, float* edges_out, float* field_out,
                             void* stream);
int aether_s2s_dynfield_rollout(const AetherS2SFilmParams* film, const AetherS2SPriorParams* prior,
                                const AetherS2SDecoderParams* decoder, const AetherS2SMarkovParams* markov, const void* plan,
                                int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                                int64_t n_nodes, int64_t n_edges, int mlp_hidden, const float* mod, size_t mod_bytes,
                                int64_t batch, int num_objects, const int64_t* send, const int64_t* recv, const int64_t* order,
                                const int64_t* rowptr, int burn_in_steps, const float* burn_in, const float* burn_in_field,
                                int steps, const float* inputs, float* decoder_state, float* h, float* c, const float* uniform,
                                void* workspace, size_t workspace_bytes, float* predictions, float* edges_out, void* stream);

/*
 * The seq2seq LoCS baseline, LoCS of nn/seq2seq/locs.py (--model_type nn.seq2seq.locs.LoCS of the electrostatic and
 * gravitational runners): the seq2seq Aether without a field, on the plain Localizer (nn/utils/global_to_local.py:46-62;
 * canonicalize_inputs, create_edge_attr_pos_vel, create_3d_edge_attr_pos_vel of nn/utils/canonicalization.py:12-30, :78-108,
 * :175-202).  No virtual origin node, no force columns: rel_feat is 2D wide (2-D [0, 0, |v|, 0], 3-D [0_3 | R^T v]), an edge
 * has 3D + O features (O = D (D - 1) / 2) and its row [features | rel_feat[recv]] is 5D + O = 11 / 18 wide, where Aether's is
 * 24 / 39; the anisotropic filter GEMM, the step's dominant cost, runs on those 11 / 18 features.  The parameter structs are
 * the plain model's with the reference's tensor shapes:
 *   prior->res1_w [he][2D], prior->filt_w2 [(5D + O) he][he], prior->filt_b2 [(5D + O) he];
 *   decoder->pmsg_fc1_w[k] [hd][5D + O], decoder->input_{r,i,n}_w [hd][2D]      (RecurrentDecoder, locs.py:457-604)
 *   markov->lin1_w [hd][5D + O], markov->res1_w [hd][2D]                        (MarkovDecoder, locs.py:368-454)
 * Exactly one of decoder / markov is given (the other NULL), as for the aether_s2s_dynfield_* entries.  There is no field
 * query: nothing of it is in the plan or the workspace and none of its kernels is launched.  `polar` is
 * params['pos_representation'] == 'polar', which both the encoder's and the decoder's Localizer take (locs.py:279-282,
 * :416-419, :527-530; Localizer._edge_pos_idx_fn): it selects edge_pos, which only the encoder's filter reads.
 *   aether_s2s_locs_plan_bytes / _plan_build : prepared weights (device, 256-byte aligned); rebuild after the weights change
 *   aether_s2s_locs_workspace_bytes          : of a step / rollout / encoder_features call
 *   aether_s2s_locs_step                     : Encoder.single_step_forward (locs.py:341-365), the hard Gumbel sample and the
 *                                              decoder (LoCS.single_step_forward :69-77) as one call; arguments as
 *                                              aether_s2s_step without the field.  With ext_logits [n_edges][K] != NULL it is
 *                                              the decoder on given logits, as calculate_loss :101-102 calls it: the sample
 *                                              is taken from them, the prior is skipped, h0 / c0 / h1 / c1 may be NULL.
 *                                              decoder_hidden_in / _out are NULL with the Markov decoder; logits_out (or
 *                                              NULL) [n_edges][K]: the prior's logits the sample was taken from (not with
 *                                              ext_logits: AETHER_EINVAL)
 *   aether_s2s_locs_rollout                  : the loops of predict_future (:122-151) as aether_s2s_rollout; decoder_state
 *                                              is NULL with the Markov decoder, whose burn-in steps run the prior only
 *   aether_s2s_locs_encoder_features         : the per-time-step half of Encoder.forward (:309-326: local frames, filter,
 *                                              res1, mlp3, mlp4) on a flattened batch of (time, graph) items -> features
 *                                              [n_edges][he], the input of aether_s2s_lstm_step / aether_s2s_mlp_head
 * Sizes as for aether_s2s_step (AETHER_EINVAL otherwise; the size calls return 0); AETHER_EINVAL: both or neither decoder,
 * a NULL pointer; AETHER_ESPACE: plan or workspace too small.  Stream-ordered, no host synchronisation (capturable); nothing
 * outside the workspace and the outputs is written.
 */
size_t aether_s2s_locs_plan_bytes(const AetherS2SDecoderParams* decoder, const AetherS2SMarkovParams* markov, int num_dims,
                                  int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                  int num_edge_types, int skip_first);
int aether_s2s_locs_plan_build(const AetherS2SPriorParams* prior, const AetherS2SDecoderParams* decoder,
                               const AetherS2SMarkovParams* markov, int num_dims, int encoder_hidden, int decoder_hidden,
                               int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first, void* plan,
                               size_t plan_bytes, void* stream);
size_t aether_s2s_locs_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                       int num_edge_types, int64_t n_nodes, int64_t n_edges);
int aether_s2s_locs_step(const AetherS2SPriorParams* prior, const AetherS2SDecoderParams* decoder,
                         const AetherS2SMarkovParams* markov, const void* plan, int num_dims, int encoder_hidden,
                         int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first,
                         int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges, const int64_t* send,
                         const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                         const float* ext_logits, const float* decoder_hidden_in, const float* h0, const float* c0,
                         const float* uniform, void* workspace, size_t workspace_bytes, float* outputs, float* decoder_hidden_out,
                         float* h1, float* c1, float* edges_out, float* logits_out, void* stream);
int aether_s2s_locs_rollout(const AetherS2SPriorParams* prior, const AetherS2SDecoderParams* decoder,
                            const AetherS2SMarkovParams* markov, const void* plan, int num_dims, int encoder_hidden,
                            int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                            int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges,
                            const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                            int burn_in_steps, const float* burn_in, int steps, const float* inputs, float* decoder_state,
                            float* h, float* c, const float* uniform, void* workspace, size_t workspace_bytes, float* predictions,
                            float* edges_out, void* stream);
int aether_s2s_locs_encoder_features(const AetherS2SPriorParams* prior, const AetherS2SDecoderParams* decoder,
                                     const AetherS2SMarkovParams* markov, const void* plan, int num_dims, int encoder_hidden,
                                     int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                                     int skip_first, int polar, int num_vars, int64_t n_nodes, int64_t n_edges, const int64_t* send,
                                     const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                                     void* workspace, size_t workspace_bytes, float* features, void* stream);

/*
 * The seq2seq dNRI baseline, DNRI of nn/seq2seq/dnri.py (--model_type nn.seq2seq.dnri.DNRI of the electrostatic and
 * gravitational runners).  The model has no local frames: no localizer, no edge attributes, no hyper-network filter and no
 * rotation of the prediction; nothing of them is in the plan or the workspace and none of their kernels is launched.
 *   DNRI_Encoder.single_step_forward (dnri.py:403-424): mlp1 on the raw state [n_nodes][2D], node2edge ([x_send | x_recv],
 *     :334-342), mlp2, edge2node (in-edge sum / (num_vars - 1), :344-351), mlp3, node2edge | skip, mlp4, one LSTM step per edge,
 *     prior_fc_out.  Each mlp is a RefNRIMLP (nn/utils/model_utils.py): Linear, ELU, Linear, ELU, BatchNorm1d on its running
 *     statistics.
 *   DNRI_Decoder.forward (:479-534): messages tanh(msg_fc2[k](tanh(msg_fc1[k]([h_recv | h_send])))) * edges[.., k] / norm (norm:
 *     the number of used edge types), summed per receiver / (num_vars - 1); the GRU gate, whose input_r / _i / _n act on the raw
 *     inputs and which has no present-message terms; out_fc1 / 2 (ReLU), out_fc3; outputs = inputs + prediction.
 *   DNRI_MLP_Decoder.forward (decoder_type 'ref_mlp', :574-624): messages relu(msg_fc2[k](relu(msg_fc1[k]([x_recv | x_send])))) *
 *     edges[.., k] on the raw inputs, summed per receiver with no division; out_fc1 on [inputs | agg]; no state.
 * Exactly one of decoder / mlp is given (the other NULL).  The entries mirror aether_s2s_locs_* argument for argument; `polar`
 * is accepted for that reason and ignored (the model has no position representation).
 *   aether_s2s_dnri_plan_bytes / _plan_build : prepared weights (device, 256-byte aligned): BatchNorm affines, summed LSTM
 *                                              biases, the padded out_fc1 of the MLP decoder, fp16 x 2 images of the layers the
 *                                              split GEMM takes; rebuild after the weights change
 *   aether_s2s_dnri_workspace_bytes          : of a step / rollout / encoder_features call (smaller than LoCS's at the same
 *                                              sizes: no frame, edge-attribute, filter or present-message buffer)
 *   aether_s2s_dnri_step                     : DNRI_Encoder.single_step_forward, the hard Gumbel sample and the decoder
 *                                              (DNRI.single_step_forward :62-69) as one call.  With ext_logits [n_edges][K] !=
 *                                              NULL it is the decoder on given logits, as calculate_loss :87-91 calls it: the
 *                                              prior is skipped, h0 / c0 / h1 / c1 may be NULL.  decoder_hidden_in / _out are
 *                                              NULL with the MLP decoder; logits_out (or NULL) [n_edges][K]: the prior's logits
 *                                              the sample was taken from (not with ext_logits: AETHER_EINVAL)
 *   aether_s2s_dnri_rollout                  : the loops of predict_future (:111-136): burn_in_steps teacher-forced steps on
 *                                              burn_in [T0][n_nodes][2D] (the prior path is causal, so the step gives what the
 *                                              full-sequence encoder gives there), then `steps` steps from inputs; decoder_state
 *                                              (NULL with the MLP decoder, whose burn-in steps run the prior only), h, c are
 *                                              read first and written last; uniform [T0 + steps][n_edges][K]
 *   aether_s2s_dnri_encoder_features         : the per-time-step half of DNRI_Encoder.forward (:376-384, mlp1 .. mlp4) on a
 *                                              flattened batch of (time, graph) items -> features [n_edges][he], the input of
 *                                              aether_s2s_lstm_step / aether_s2s_mlp_head
 * Sizes: num_dims 2 or 3, encoder_hidden a multiple of 128, decoder_hidden of 32, rnn_hidden of 16, 1..4 prior layers
 * (prior_hidden a multiple of 16 when there are several), 1..4 edge types of which at least one is used (AETHER_EINVAL
 * otherwise; the size calls return 0).  AETHER_EINVAL: both or neither decoder, a NULL pointer; AETHER_ESPACE: plan or
 * workspace too small.  Everything is checked before anything is queued.  Stream-ordered, no host synchronisation
 * (capturable); nothing outside the workspace and the outputs is written.
 */
typedef struct AetherS2SDnriPriorParams {
    const float* mlp_w0[4]; const float* mlp_b0[4];      /* mlp1 .. mlp4, first Linear: [he][2D], [he][2he], [he][he], [he][3he] */
    const float* mlp_w3[4]; const float* mlp_b3[4];      /* second Linear: [he][he], [he] */
    const float* mlp_bn_w[4]; const float* mlp_bn_b[4]; const float* mlp_bn_mean[4]; const float* mlp_bn_var[4];   /* [he] */
    const float* lstm_w_ih; const float* lstm_w_hh; const float* lstm_b_ih; const float* lstm_b_hh; /* forward_rnn: [4R][he], [4R][R] */
    const float* prior_w[4]; const float* prior_b[4];    /* prior_fc_out */
} AetherS2SDnriPriorParams;
typedef struct AetherS2SDnriDecoderParams {
    const float* msg_fc1_w[4]; const float* msg_fc1_b[4];    /* [hd][2hd] (receiver | sender halves), [hd] */
    const float* msg_fc2_w[4]; const float* msg_fc2_b[4];    /* [hd][hd], [hd] */
    const float* hidden_r_w; const float* hidden_i_w; const float* hidden_h_w;      /* [hd][hd], no bias */
    const float* input_r_w; const float* input_r_b;
    const float* input_i_w; const float* input_i_b;
    const float* input_n_w; const float* input_n_b;          /* [hd][2D], [hd] */
    const float* out1_w; const float* out1_b; const float* out2_w; const float* out2_b;   /* out_fc1 / 2: [hd][hd], [hd] */
    const float* out3_w; const float* out3_b;                /* out_fc3: [2D][hd], [2D] */
} AetherS2SDnriDecoderParams;
typedef struct AetherS2SDnriMlpParams {
    const float* msg_fc1_w[4]; const float* msg_fc1_b[4];    /* [hd][4D] (receiver | sender halves), [hd] */
    const float* msg_fc2_w[4]; const float* msg_fc2_b[4];    /* [hd][hd], [hd] */
    const float* out1_w; const float* out1_b;                /* out_fc1: [hd][2D + hd] on [inputs | agg], [hd] */
    const float* out2_w; const float* out2_b;                /* out_fc2: [hd][hd], [hd] */
    const float* out3_w; const float* out3_b;                /* out_fc3: [2D][hd], [2D] */
} AetherS2SDnriMlpParams;
size_t aether_s2s_dnri_plan_bytes(const AetherS2SDnriDecoderParams* decoder, const AetherS2SDnriMlpParams* mlp, int num_dims,
                                  int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                  int num_edge_types, int skip_first);
int aether_s2s_dnri_plan_build(const AetherS2SDnriPriorParams* prior, const AetherS2SDnriDecoderParams* decoder,
                               const AetherS2SDnriMlpParams* mlp, int num_dims, int encoder_hidden, int decoder_hidden,
                               int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first, void* plan,
                               size_t plan_bytes, void* stream);
size_t aether_s2s_dnri_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                       int num_edge_types, int64_t n_nodes, int64_t n_edges);
int aether_s2s_dnri_step(const AetherS2SDnriPriorParams* prior, const AetherS2SDnriDecoderParams* decoder,
                         const AetherS2SDnriMlpParams* mlp, const void* plan, int num_dims, int encoder_hidden,
                         int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types, int skip_first,
                         int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges, const int64_t* send,
                         const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                         const float* ext_logits, const float* decoder_hidden_in, const float* h0, const float* c0,
                         const float* uniform, void* workspace, size_t workspace_bytes, float* outputs, float* decoder_hidden_out,
                         float* h1, float* c1, float* edges_out, float* logits_out, void* stream);
int aether_s2s_dnri_rollout(const AetherS2SDnriPriorParams* prior, const AetherS2SDnriDecoderParams* decoder,
                            const AetherS2SDnriMlpParams* mlp, const void* plan, int num_dims, int encoder_hidden,
                            int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                            int skip_first, int polar, int num_vars, float tau, int64_t n_nodes, int64_t n_edges,
                            const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                            int burn_in_steps, const float* burn_in, int steps, const float* inputs, float* decoder_state,
                            float* h, float* c, const float* uniform, void* workspace, size_t workspace_bytes, float* predictions,
                            float* edges_out, void* stream);
int aether_s2s_dnri_encoder_features(const AetherS2SDnriPriorParams* prior, const AetherS2SDnriDecoderParams* decoder,
                                     const AetherS2SDnriMlpParams* mlp, const void* plan, int num_dims, int encoder_hidden,
                                     int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden, int num_edge_types,
                                     int skip_first, int polar, int num_vars, int64_t n_nodes, int64_t n_edges, const int64_t* send,
                                     const int64_t* recv, const int64_t* order, const int64_t* rowptr, const float* inputs,
                                     void* workspace, size_t workspace_bytes, float* features, void* stream);

/*
 * The seq2seq ablation DNRIAether of nn/seq2seq/ablations/dnri_aether.py (--model_type nn.seq2seq.ablations.dnri_aether.
 * DNRIAether): dNRI whose encoder and decoders also read the field the model discovers, without local frames.  The field is
 * Aether's: predict_field (:81-85) = field_net(RFF(position)), AetherS2SFieldParams.  ext = [inputs | field] (3D columns) takes
 * the place of the raw state in mlp1's first Linear (:320, :416, :446), in input_r / _i / _n of DNRI_Decoder (:498-500, :564-569)
 * and in msg_fc1[k] / out_fc1 of DNRI_MLP_Decoder (:601, :608, :632-636, :669); both decoders return inputs + prediction on the
 * 2D-wide state (:580, :677).  The entries are aether_s2s_dnri_*'s with `field` in front and the arguments named below; the
 * three parameter structs are dNRI's with the wider first-layer tensors: mlp_w0[0] [he][3D], input_*_w [hd][3D], the MLP
 * decoder's msg_fc1_w[k] [hd][6D] and out1_w [hd][3D + hd].
 *   aether_s2s_dnri_aether_plan_bytes / _plan_build : dNRI's plan (out_fc1 padded from 3D + hd columns) and the fp16 x 2 images of
 *                                              field_net.0 / .2
 *   aether_s2s_dnri_aether_workspace_bytes   : dNRI's workspace and the field query's rows (RFF, two hidden layers, field, ext);
 *                                              nothing of a frame
 *   aether_s2s_dnri_aether_step              : predict_field, DNRI_Encoder.single_step_forward (:443-467), the hard Gumbel sample
 *                                              and the decoder (single_step_forward :87-94) as one call.  ext_field [n_nodes][D]
 *                                              != NULL: the field is handed in and no field launch is made (`field` may then be
 *                                              NULL); ext_logits as for dNRI (with both it is single_step_forward itself, as
 *                                              calculate_loss :119-122 calls it); field_out (or NULL) [n_nodes][D]: the field the
 *                                              step used
 *   aether_s2s_dnri_aether_rollout           : the loops of predict_future (:142-172).  burn_in_field (NULL or [burn_in_steps]
 *                                              [n_nodes][D]): the field of the burn-in frames, known before the loop (:148-149);
 *                                              the predicted steps query theirs from their own predictions (:161)
 *   aether_s2s_dnri_aether_encoder_features  : the per-time-step half of DNRI_Encoder.forward (:409-425) on a flattened batch of
 *                                              (time, graph) items; field_in (NULL: queried) [n_nodes][D] the field of those frames
 * Sizes, status codes and stream order as aether_s2s_dnri_*; AETHER_EINVAL also when `field` is NULL and a step has to query.
 */
size_t aether_s2s_dnri_aether_plan_bytes(const AetherS2SDnriDecoderParams* decoder, const AetherS2SDnriMlpParams* mlp, int num_dims,
                                         int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                         int num_edge_types, int skip_first);
int aether_s2s_dnri_aether_plan_build(const AetherS2SFieldParams* field, const AetherS2SDnriPriorParams* prior,
                                      const AetherS2SDnriDecoderParams* decoder, const AetherS2SDnriMlpParams* mlp, int num_dims,
                                      int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers, int prior_hidden,
                                      int num_edge_types, int skip_first, void* plan, size_t plan_bytes, void* stream);
size_t aether_s2s_dnri_aether_workspace_bytes(int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_hidden,
                                              int num_edge_types, int64_t n_nodes, int64_t n_edges);
int aether_s2s_dnri_aether_step(const AetherS2SFieldParams* field, const AetherS2SDnriPriorParams* prior,
                                const AetherS2SDnriDecoderParams* decoder, const AetherS2SDnriMlpParams* mlp, const void* plan,
                                int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                                int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order,
                                const int64_t* rowptr, const float* inputs, const float* ext_field, const float* ext_logits,
                                const float* decoder_hidden_in, const float* h0, const float* c0, const float* uniform,
                                void* workspace, size_t workspace_bytes, float* outputs, float* decoder_hidden_out, float* h1,
                                float* c1, float* edges_out, float* logits_out, float* field_out, void* stream);
int aether_s2s_dnri_aether_rollout(const AetherS2SFieldParams* field, const AetherS2SDnriPriorParams* prior,
                                   const AetherS2SDnriDecoderParams* decoder, const AetherS2SDnriMlpParams* mlp, const void* plan,
                                   int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                   int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars, float tau,
                                   int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv, const int64_t* order,
                                   const int64_t* rowptr, int burn_in_steps, const float* burn_in, const float* burn_in_field,
                                   int steps, const float* inputs, float* decoder_state, float* h, float* c, const float* uniform,
                                   void* workspace, size_t workspace_bytes, float* predictions, float* edges_out, void* stream);
int aether_s2s_dnri_aether_encoder_features(const AetherS2SFieldParams* field, const AetherS2SDnriPriorParams* prior,
                                            const AetherS2SDnriDecoderParams* decoder, const AetherS2SDnriMlpParams* mlp, const void* plan,
                                            int num_dims, int encoder_hidden, int decoder_hidden, int rnn_hidden, int prior_layers,
                                            int prior_hidden, int num_edge_types, int skip_first, int polar, int num_vars,
                                            int64_t n_nodes, int64_t n_edges, const int64_t* send, const int64_t* recv,
                                            const int64_t* order, const int64_t* rowptr, const float* inputs, const float* field_in,
                                            void* workspace, size_t workspace_bytes, float* features, void* stream);

/*
 * k-nearest-neighbour edge builder for variable-N scenes: replaces Encoder.knn_edges
 * (nn/dynamicvars/aether_dynamicvars.py:559-586; the same method in the other *_dynamicvars.py) and the send /
 * recv half of get_knn_graph_info (experiments/ind/single_ind_data.py:186-217).
 *   x        : float[n_scenes][n_objects][x_stride]   the first two columns are the 2-D position
 *   masks    : float[n_scenes][n_objects]             != 0: the object is present in the scene
 *   k        : neighbours per object (the reference: min(10, n_objects - 1)); 1 <= k <= 16
 *   send, recv : int64[capacity], capacity >= n_scenes * n_objects * k; the first totals[0] entries are
 *              written: scene by scene, object by object, nearest neighbour first, in the compacted
 *              numbering (present objects of all scenes counted consecutively).  As in the reference,
 *              `send` is the querying object and `recv` its neighbour.
 *   scene_edges, scene_nodes : int64[n_scenes]  edges / present objects per scene
 *   totals   : int64[2] = {edges, present objects}
 * Equal distances keep index order (torch.topk leaves that order unspecified).  Stream-ordered, no host
 * synchronisation; read totals[0] after the stream to size the result.
 */
size_t aether_knn_workspace_bytes(int64_t n_scenes, int n_objects, int k);
int aether_knn_edges(const float* x, int x_stride, const float* masks, int64_t n_scenes, int n_objects, int k,
                     int64_t* send, int64_t* recv, int64_t* scene_edges, int64_t* scene_nodes, int64_t* totals,
                     void* workspace, size_t workspace_bytes, void* stream);

/*
 * On-device data side: the simulators that generate the reference's datasets, batched over
 * simulations (fp64, as numpy).  The random draws (charges, initial state, field sources, observation noise)
 * stay with the caller's numpy generators, so a dataset is reproduced draw for draw.
 *
 * aether_sim_electrostatic replaces the integration of ElectrostaticFieldSim.sample_trajectory
 * (experiments/electrostatic/dataset/electrostatic_field_sim.py:108-163): Coulomb forces between all balls
 * (n_balls moving, then total_balls - n_balls static field sources), force capped at max_F, leap-frog.
 *   loc0, vel0 : double[n_sims][total_balls][dim]   initial state (:96-104; static velocities 0)
 *   charges    : double[n_sims][total_balls]        (:79-92)
 *   loc, vel   : double[n_sims][T/sample_freq - 1][total_balls][dim]   saved frames (:139-142; static rows constant)
 *   maxed_out  : int64[n_sims]   number of capped forces (the count the reference prints, :168)
 * aether_sim_gravitational replaces GravitationalFieldSim.sample_trajectory's loop
 * (experiments/gravitational/dataset/gravitational_field_sim.py:99-125): softened gravity, kick-drift-kick.
 *   pos0, vel0 : double[n_sims][total_balls][dim] (velocities in the centre-of-mass frame, :96); mass [n_sims][total_balls]
 *   pos, vel, force : double[n_sims][T/sample_freq][total_balls][dim]
 * total_balls <= 64, dim 2 or 3.  Stream-ordered.
 */
int aether_sim_electrostatic(const double* loc0, const double* vel0, const double* charges, int64_t n_sims,
                             int n_balls, int total_balls, int dim, int T, int sample_freq,
                             double interaction_strength, double delta_T, double max_F, double* loc, double* vel,
                             int64_t* maxed_out, void* stream);
/*
 * aether_sim_charged: the n-body simulators of the state2state runner's data sets
 * (experiments/lorentz/dataset/synthetic_sim.py: ChargedParticlesSim :221-300, GravitySim :375-460, DynamicSim
 * :536-622): 3-D Coulomb forces between n_balls moving charges, squared distances |a|^2 + |b|^2 - 2 a.b + 1e-6, plus
 * ext_mode 0: nothing ('charged'), 1: the constant force ext ('static': (0, 0, 0.098)), 2: the Lorentz force
 * q (v x ext) ('dynamic': ext = (0.5, 0.5, 0.5)), 3: a fixed charge at ext, ext_strength q (x - ext) / |x - ext|^3
 * (FixCharge :626-790: ext = (10, 10, 10), ext_strength 0.1).  pair != NULL (double[n_sims][n_balls][n_balls]): the pair
 * force is -interaction_strength * pair_ij (x_i - x_j) instead of Coulomb's and charges may be NULL (SpringSim :6-146).
 * Every force component is clipped to +-max_F; leap-frog.
 *   loc0, vel0 : double[n_sims][3][n_balls] (the reference's layout);  charges : double[n_sims][n_balls]
 *   ext        : HOST pointer to 3 doubles (read during the call; may be NULL for ext_mode 0)
 *   loc, vel   : double[n_sims][T/sample_freq - 1][3][n_balls]
 */
int aether_sim_charged(const double* loc0, const double* vel0, const double* charges, const double* pair, int64_t n_sims,
                       int n_balls, int T, int sample_freq, double interaction_strength, double delta_T, double max_F,
                       int ext_mode, const double* ext, double ext_strength, double* loc, double* vel, void* stream);
int aether_sim_gravitational(const double* pos0, const double* vel0, const double* mass, int64_t n_sims, int n_balls,
                             int total_balls, int dim, int T, int sample_freq, double interaction_strength,
                             double dt, double softening, double* pos, double* vel, double* force, void* stream);

/*
 * Variable-N models, one step of the decoder (second half): replaces Decoder.forward of
 * nn/dynamicvars/aether_dynamicvars.py:775-870 (2-D, one scene) on the objects present in the scene.
 * Differences from aether_s2s_decoder_step: rel_feat = the canonical state only (canonicalize_augmented_inputs,
 * 6 columns), messages from the present state through one AnisotropicEdgeFilter per edge type
 * (nn/nn/anisotropic_filter.py:34-40 with a ReLU hidden layer, in_size 15 = 9 edge features + 6 receiver columns)
 * followed by ReLU, hidden messages divided by the number of used edge types (:801-814), both aggregations are
 * sums over the caller's lists divided by agg_div (the reference: edge2node_inds rows, / (num_vars - 1), :816-819).
 *   inputs [n][4], field [n][2], hidden_in [n][h]: the present objects, compacted; edge_w [e][K]
 *   edge_state : float[m][6] rows [pos | vel | field] indexed by send / recv for the edge features; NULL = the
 *                compacted [inputs | field].  (The reference indexes the un-compacted array with compacted
 *                indices, :823 -- pass that array to reproduce it when objects are missing.)
 *   send, recv : int64[e] compacted object indices; agg_order int64[*], agg_rowptr int64[n + 1]: the edges summed
 *                into each object (the reference's edge2node_inds, flattened, with rowptr[i] = i * k)
 *   outputs [n][4], hidden_out [n][h];  h % 128 == 0
 */
typedef struct AetherDynDecoderParams {
    const float* msg_fc1_w[4]; const float* msg_fc1_b[4];    /* [h][2h] (receiver | sender halves), [h] */
    const float* msg_fc2_w[4]; const float* msg_fc2_b[4];    /* [h][h], [h] */
    const float* hidden_r_w; const float* hidden_i_w; const float* hidden_h_w;      /* [h][h], no bias */
    const float* input_r_w; const float* input_r_b;
    const float* input_i_w; const float* input_i_b;
    const float* input_n_w; const float* input_n_b;          /* [h][6], [h] */
    const float* present_r_w; const float* present_r_b;
    const float* present_i_w; const float* present_i_b;
    const float* present_n_w; const float* present_n_b;      /* [h][h], [h] */
    const float* out1_w; const float* out1_b; const float* out2_w; const float* out2_b;   /* out_fc1, out_fc2: [h][h] */
    const float* out3_w; const float* out3_b;                /* out_fc3: [4][h] */
    const float* filt_w0[4]; const float* filt_b0[4];        /* edge_filter.k.edge_filter.0: [h][3], [h] */
    const float* filt_w2[4]; const float* filt_b2[4];        /* edge_filter.k.edge_filter.2: [15 h][h], [15 h] */
    const void* filt_image[4];   /* aether_s2s_filter_prepare(filt_w2[k], 15, h, ..) of the current values, or NULL (built per call) */
} AetherDynDecoderParams;
size_t aether_dyn_decoder_workspace_bytes(int hidden, int64_t n_nodes, int64_t n_edges);
int aether_dyn_decoder_step(const AetherDynDecoderParams* params, int hidden, int num_edge_types, int skip_first,
                            int polar, int64_t n_nodes, int64_t n_edges, const float* inputs, const float* hidden_in,
                            const float* edge_w, const float* field, const float* edge_state, const int64_t* send,
                            const int64_t* recv, const int64_t* agg_order, const int64_t* agg_rowptr, float agg_div,
                            void* workspace, size_t workspace_bytes, float* outputs, float* hidden_out, void* stream);
/*
 * The same step for SEVERAL scenes at once -- what the reference cannot do (its variable-N models raise on batch > 1,
 * aether_dynamicvars.py:588-591): the present objects of all scenes are concatenated (n_nodes rows), `send` / `recv` /
 * `agg_order` are in that concatenated numbering (no edge crosses scenes), and the two per-scene quantities of the
 * single-scene call become arrays:
 *   agg_div_node : float[n_nodes], the divisor of each object's sums (the reference: its scene's num_vars - 1);
 *                  NULL = the scalar agg_div for everyone
 *   state_send, state_recv : int64[e] rows of `edge_state` the edge features read (NULL = send / recv).  The reference
 *                  indexes its scene's UN-compacted state with compacted indices (:823); with several scenes that is
 *                  scene_base_of_uncompacted_rows + compacted index within the scene, which differs from `send`.
 * aether_dyn_decoder_step is this function with both NULL.
 */
int aether_dyn_decoder_step_batched(const AetherDynDecoderParams* params, int hidden, int num_edge_types, int skip_first,
                                    int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                                    const float* hidden_in, const float* edge_w, const float* field,
                                    const float* edge_state, const int64_t* state_send, const int64_t* state_recv,
                                    const int64_t* send, const int64_t* recv, const int64_t* agg_order,
                                    const int64_t* agg_rowptr, float agg_div, const float* agg_div_node, void* workspace,
                                    size_t workspace_bytes, float* outputs, float* hidden_out, void* stream);

/*
 * Variable-N models, one step of the encoder's prior and the field query: with
 * aether_knn_edges, aether_dyn_decoder_step and aether_s2s_gumbel_hard the whole prediction step of
 * AetherDynamicVars.predict_future (nn/dynamicvars/aether_dynamicvars.py:245-273).
 *
 * aether_dyn_prior_step replaces Encoder.compute_feat_transform for one time step (:505-557) + the LSTM / prior
 * half of Encoder.single_step_forward (:688-696) on the present objects of a scene: canonical states, edge features
 * [9 | receiver's canonical state 6], anisotropic filter (ReLU hidden layer), SUM over the in-edges of an object +
 * mlp1(canonical state), mlp3, [x_send | x_recv | edge] -> mlp4 (RefNRIMLP in eval mode; bn pointers may all be
 * NULL: no_encoder_bn), one LSTM step per edge, prior_fc_out.
 *   inputs [n][4], field [n][2] : the present objects, compacted;  send, recv int64[e] (compacted; features of
 *   send -> recv in recv's frame, as aether_knn_edges lists them);  order, rowptr : edges grouped by recv (CSR)
 *   h0, c0 [e][R] : the LSTM state rows of these edges (the reference keeps one slot per fully connected pair and
 *   gathers / scatters them, :684-694: that indexing stays with the caller);  logits [e][K], h1, c1 [e][R]
 * aether_dyn_field replaces AetherDynamicVars.predict_field (:64-79) on the present objects: Fourier features of the
 * position (hidden/2 frequencies), angular_embedding Linear(2, hidden) of the unit velocity, field_net
 * Linear(2 hidden, hidden)-SiLU-Linear-SiLU-Linear(hidden, 2).   x [n][4] -> field [n][2]
 */
typedef struct AetherDynPriorParams {
    const float* mlp1_w0; const float* mlp1_b0; const float* mlp1_w3; const float* mlp1_b3;       /* [h][6], [h][h] */
    const float* mlp1_bn_w; const float* mlp1_bn_b; const float* mlp1_bn_mean; const float* mlp1_bn_var;
    const float* mlp3_w0; const float* mlp3_b0; const float* mlp3_w3; const float* mlp3_b3;       /* [h][h] */
    const float* mlp3_bn_w; const float* mlp3_bn_b; const float* mlp3_bn_mean; const float* mlp3_bn_var;
    const float* mlp4_w0; const float* mlp4_b0; const float* mlp4_w3; const float* mlp4_b3;       /* [h][3h], [h][h] */
    const float* mlp4_bn_w; const float* mlp4_bn_b; const float* mlp4_bn_mean; const float* mlp4_bn_var;
    const float* lstm_w_ih; const float* lstm_w_hh; const float* lstm_b_ih; const float* lstm_b_hh; /* [4R][h], [4R][R] */
    const float* prior_w[4]; const float* prior_b[4];                                            /* prior_fc_out */
    const float* filt_w0; const float* filt_b0;                                                  /* [h][3] */
    const float* filt_w2; const float* filt_b2;                                                  /* [15 h][h] */
    const void* filt_image;   /* aether_s2s_filter_prepare(filt_w2, 15, h, ..) of the current values, or NULL (built per call) */
} AetherDynPriorParams;
size_t aether_dyn_prior_workspace_bytes(int hidden, int rnn_hidden, int prior_hidden, int64_t n_nodes, int64_t n_edges);
int aether_dyn_prior_step(const AetherDynPriorParams* params, int hidden, int rnn_hidden, int prior_layers,
                          int prior_hidden, int num_edge_types, int polar, int64_t n_nodes, int64_t n_edges,
                          const float* inputs, const float* field, const float* h0, const float* c0,
                          const int64_t* send, const int64_t* recv, const int64_t* order, const int64_t* rowptr,
                          void* workspace, size_t workspace_bytes, float* logits, float* h1, float* c1, void* stream);
typedef struct AetherDynFieldQueryParams {
    const float* B;                                            /* coordinate_embedding.B [2][hidden/2] */
    const float* ang_w; const float* ang_b;                    /* angular_embedding [hidden][2], [hidden] */
    const float* w0; const float* b0; const float* w2; const float* b2; const float* w4; const float* b4;
                                                               /* field_net.{0,2,4}: [h][2h], [h][h], [2][h] */
} AetherDynFieldQueryParams;
size_t aether_dyn_field_workspace_bytes(int64_t n_points, int hidden);
int aether_dyn_field(const AetherDynFieldQueryParams* params, int hidden, int64_t n_points, const float* x,
                     void* workspace, size_t workspace_bytes, float* field, void* stream);

/*
 * One prediction step of the variable-N model as ONE call (round 3): the body of AetherDynamicVars.predict_future's loop
 * (nn/dynamicvars/aether_dynamicvars.py:245-273) for one scene -- field at the present objects (:64-79), the encoder's
 * own kNN graph + prior step with the per-pair LSTM slots gathered and scattered (:672-699), the hard Gumbel sample
 * (:133-141) and the decoder step (:775-870) -- with the index work between the stages (mask -> rows, receiver CSR of the
 * kNN graph, slot arithmetic, scatter of the results) in seven small kernels instead of ~60 framework launches.
 *   state [n_objects_max][4] : the scene's rows (observed objects: ground truth, the others: the last prediction, :264)
 *   mask  [n_objects_max]    : non-zero = present; n_present = their number, known to the caller (len(node_inds)).
 *                              A mask that disagrees makes the step's outputs NaN and the next call return AETHER_EHIP.
 *   node_inds int64[n_present] or NULL (= the mask's non-zero rows, ascending): rows of the present objects
 *   graph_send, graph_recv int64[n_edges], edge2node int64[n_present][in_degree] : the data set's graph_info of the step, in
 *                              the numbering of the present objects (single_ind_data.py:186-217);
 *                              n_edges = n_present * min(knn_k, n_present - 1), as the encoder's own graph has
 *   prior_h, prior_c [n_objects_max (n_objects_max - 1)][rnn_hidden] : one LSTM slot per ordered pair, UPDATED IN PLACE
 *   decoder_hidden [n_objects_max][decoder_hidden] : UPDATED IN PLACE at the present rows
 *   uniform [n_edges][K] : the U(0,1) draw of gumbel_softmax;  edge_types [n_edges][K] (one-hot, out) or NULL
 *   prediction [n_objects_max][4] : the decoder's output at the present rows, zero elsewhere (:866-868)
 * Every stage is the entry point documented above (same kernels, same order): results equal the staged calls bit for bit.
 */
typedef struct AetherDynStepConfig {
    int field_hidden, encoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, decoder_hidden;
    int skip_first, encoder_polar, decoder_polar, knn_k;
    float gumbel_tau;
} AetherDynStepConfig;
size_t aether_dyn_step_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int64_t n_present,
                                       int64_t n_edges);
int aether_dyn_step(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                    const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_objects_max,
                    int64_t n_present, int64_t n_edges, const float* state, const float* mask, const int64_t* node_inds,
                    const int64_t* graph_send, const int64_t* graph_recv, const int64_t* edge2node, int in_degree,
                    float* prior_h, float* prior_c, float* decoder_hidden, const float* uniform, float* prediction,
                    float* edge_types, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The prediction loop around aether_dyn_step (AetherDynamicVars.predict_future, :245-273) for one scene: for step t the
 * state is  observed * inputs[t] + (1 - observed) * (t == 0 ? inputs[0] : predictions[t - 1])  with observed =
 * burn_in_masks[t] (:264), then one aether_dyn_step.  Device arrays: inputs [n_steps + 1][n_objects_max][4] (row
 * n_steps is not read), masks, burn_in_masks [n_steps][n_objects_max] (at least), predictions [n_steps][n_objects_max][4];
 * prior_h / prior_c / decoder_hidden as in aether_dyn_step (initial state in, final state out).  HOST arrays of length
 * n_steps: n_present, n_edges (entries of the step's graph_send / graph_recv / uniform rows; as in aether_dyn_step it has
 * to equal n_present * min(knn_k, n_present - 1), the size of the encoder's own kNN graph), in_degree, and the per-step
 * device pointers node_inds (or NULL, or NULL entries), graph_send, graph_recv, edge2node, uniform.  Steps without present
 * objects yield zeros and leave the states alone (:841-843); a step with exactly one is refused (the reference fails there
 * too).  EVERY step is validated on the host before the first launch: a refused call has queued nothing and touched no
 * state.  No host synchronisation: the whole loop is queued on `stream` (52 launches per step).  A mask that disagrees
 * with n_present poisons that step's outputs AND the LSTM state rows it would have written with NaN (async error word).
 */
size_t aether_dyn_rollout_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int n_steps,
                                          const int64_t* n_present, const int64_t* n_edges);
int aether_dyn_rollout(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                       const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_objects_max,
                       int n_steps, const float* inputs, const float* masks, const float* burn_in_masks,
                       const int64_t* n_present, const int64_t* n_edges, const int64_t* const* node_inds,
                       const int64_t* const* graph_send, const int64_t* const* graph_recv, const int64_t* const* edge2node,
                       const int* in_degree, const float* const* uniform, float* prior_h, float* prior_c,
                       float* decoder_hidden, float* predictions, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same step and loop for B scenes per call (round 4; BASELINE config 4 is batch = 64; the reference's models raise on
 * batch > 1, aether_dynamicvars.py:588-591).  The present objects of all scenes are numbered consecutively, scene-major;
 * every stage runs once over all of them (same stage kernels as the single-scene call).  HOST arrays of length n_scenes:
 * n_present (0, or 2 .. n_objects_max per scene), n_edges (= n_present * min(knn_k, n_present - 1) per scene), in_degree
 * (1 .. 255).  Device arrays: state [B][n_max][4], mask [B][n_max], decoder_hidden [B][n_max][hd], prediction [B][n_max][4],
 * prior_h / prior_c [B * n_max (n_max - 1)][R] (scene b's slots from b * n_max (n_max - 1) on); node_inds (or NULL),
 * graph_send, graph_recv, edge2node, uniform: the scenes' arrays CONCATENATED in scene order, indices scene-local exactly
 * as the single-scene call takes them.  n_scenes <= 256.  A scene whose mask disagrees with its n_present poisons the
 * step's outputs with NaN (async error word).  aether_dyn_rollout_batched: every per-step tensor TIME-MAJOR -- inputs
 * [n_steps + 1][B][n_max][4], masks / burn_in_masks [n_steps][B][n_max], predictions [n_steps][B][n_max][4], host size arrays
 * [n_steps][B], per-step device pointers as in aether_dyn_rollout; everything is validated before the first launch.
 */
size_t aether_dyn_step_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max,
                                               const int64_t* n_present, const int64_t* n_edges, const int* in_degree);
int aether_dyn_step_batched(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                            const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_scenes,
                            int n_objects_max, const int64_t* n_present, const int64_t* n_edges, const int* in_degree,
                            const float* state, const float* mask, const int64_t* node_inds, const int64_t* graph_send,
                            const int64_t* graph_recv, const int64_t* edge2node, float* prior_h, float* prior_c,
                            float* decoder_hidden, const float* uniform, float* prediction, float* edge_types,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t aether_dyn_rollout_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max, int n_steps,
                                                  const int64_t* n_present, const int64_t* n_edges, const int* in_degree);
int aether_dyn_rollout_batched(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                               const AetherDynDecoderParams* decoder_params, const AetherDynStepConfig* config, int n_scenes,
                               int n_objects_max, int n_steps, const float* inputs, const float* masks,
                               const float* burn_in_masks, const int64_t* n_present, const int64_t* n_edges,
                               const int* in_degree, const int64_t* const* node_inds, const int64_t* const* graph_send,
                               const int64_t* const* graph_recv, const int64_t* const* edge2node, const float* const* uniform,
                               float* prior_h, float* prior_c, float* decoder_hidden, float* predictions, void* workspace,
                               size_t workspace_bytes, void* stream);

/*
 * The variable-N dNRI baseline (nn/dynamicvars/dnri_dynamicvars.py: DNRIDynamicVars, prediction path) on the same scene
 * engine.  The model has no field, no local frames, no edge attributes and no filter: none of their kernels is launched and
 * no buffer is sized for one.  The entries mirror the Aether ones argument for argument, minus the field parameters.
 *
 * aether_dyn_dnri_prior_step replaces DNRI_DynamicVars_Encoder.compute_feat_transform for one time step (:386-432) + the
 * LSTM / prior half of single_step_forward (:552-566) on the present objects, compacted: mlp1 on the raw 4 columns,
 * [x_send | x_recv] -> mlp2 (kept as the skip), index_add_ over the receiver (:374-377, a plain SUM), mlp3,
 * [x_send | x_recv | skip] -> mlp4 (RefNRIMLP in eval mode; the four bn pointers of a layer may be NULL: no_encoder_bn), one
 * LSTM step per edge, prior_fc_out.
 *   inputs [n][4];  send, recv int64[e]: the encoder's own kNN graph (aether_knn_edges: the query object is the sender),
 *   order, rowptr: its edges grouped by recv (CSR);  h0, c0 [e][R]: the LSTM state rows of the CALLER's edges, row e for edge
 *   e of the caller's graph (:554-559: the pairing is positional, so both graphs list n min(k, n - 1) edges; the slot
 *   arithmetic stays with the caller);  logits [e][K], h1, c1 [e][R].  `polar` is ignored (there is no frame).
 *
 * aether_dyn_dnri_decoder_step_batched replaces DNRI_DynamicVars_Decoder.forward (:618-688) on the present objects of one or
 * several scenes, concatenated: pre_msg = [h_recv | h_send], tanh(msg_fc2(tanh(msg_fc1))) z_k / (number of used types) per
 * used type, sum over the agg_order rows / agg_div_node (the scene's num_vars - 1; NULL: the scalar agg_div), the GRU-style
 * gate with input_r / _i / _n on the raw inputs, out_fc1-3 with ReLU and the residual.  decoder_dropout is 0 (the reference
 * drops in eval mode too, :653, :678-679: refused by the module, not reproduced).
 *   inputs [n][4], hidden_in [n][h], edge_w [e][K] with ONE-HOT rows (hard samples: every edge sits in one type's list);
 *   send, recv int64[e]; agg_order, agg_rowptr as aether_dyn_decoder_step_batched;  outputs [n][4], hidden_out [n][h].
 *   n >= 2 and e >= 1: a scene with one present object is not taken.  `polar` is ignored.
 */
typedef struct AetherDynDnriPriorParams {
    const float* mlp_w0[4]; const float* mlp_b0[4];      /* mlp1 .. mlp4, first Linear: [h][4], [h][2h], [h][h], [h][3h] */
    const float* mlp_w3[4]; const float* mlp_b3[4];      /* second Linear: [h][h], [h] */
    const float* mlp_bn_w[4]; const float* mlp_bn_b[4]; const float* mlp_bn_mean[4]; const float* mlp_bn_var[4];   /* [h] or NULL */
    const float* lstm_w_ih; const float* lstm_w_hh; const float* lstm_b_ih; const float* lstm_b_hh; /* forward_rnn: [4R][h], [4R][R] */
    const float* prior_w[4]; const float* prior_b[4];    /* prior_fc_out */
} AetherDynDnriPriorParams;
typedef struct AetherDynDnriDecoderParams {
    const float* msg_fc1_w[4]; const float* msg_fc1_b[4];    /* [h][2h] (receiver | sender halves), [h] */
    const float* msg_fc2_w[4]; const float* msg_fc2_b[4];    /* [h][h], [h] */
    const float* hidden_r_w; const float* hidden_i_w; const float* hidden_h_w;      /* [h][h], no bias */
    const float* input_r_w; const float* input_r_b;
    const float* input_i_w; const float* input_i_b;
    const float* input_n_w; const float* input_n_b;          /* [h][4], [h] */
    const float* out1_w; const float* out1_b; const float* out2_w; const float* out2_b;   /* out_fc1 / 2: [h][h], [h] */
    const float* out3_w; const float* out3_b;                /* out_fc3: [4][h], [4] */
} AetherDynDnriDecoderParams;
size_t aether_dyn_dnri_prior_workspace_bytes(int hidden, int rnn_hidden, int prior_hidden, int64_t n_nodes, int64_t n_edges);
int aether_dyn_dnri_prior_step(const AetherDynDnriPriorParams* params, int hidden, int rnn_hidden, int prior_layers,
                               int prior_hidden, int num_edge_types, int polar, int64_t n_nodes, int64_t n_edges,
                               const float* inputs, const float* h0, const float* c0, const int64_t* send, const int64_t* recv,
                               const int64_t* order, const int64_t* rowptr, void* workspace, size_t workspace_bytes,
                               float* logits, float* h1, float* c1, void* stream);
size_t aether_dyn_dnri_decoder_workspace_bytes(int hidden, int num_edge_types, int64_t n_nodes, int64_t n_edges);
int aether_dyn_dnri_decoder_step_batched(const AetherDynDnriDecoderParams* params, int hidden, int num_edge_types, int skip_first,
                                         int polar, int64_t n_nodes, int64_t n_edges, const float* inputs,
                                         const float* hidden_in, const float* edge_w, const int64_t* send, const int64_t* recv,
                                         const int64_t* agg_order, const int64_t* agg_rowptr, float agg_div,
                                         const float* agg_div_node, void* workspace, size_t workspace_bytes, float* outputs,
                                         float* hidden_out, void* stream);
/*
 * One prediction step (the body of DNRIDynamicVars.predict_future's loop, :165-174) and the whole loop (:152-175) for
 * 1 .. 256 scenes as ONE call each: aether_dyn_step_batched / aether_dyn_rollout_batched without the field stage, with the
 * same arrays, conventions and checks -- n_scenes = 1 is the single-scene call.  AetherDynStepConfig is reused; its
 * field_hidden, encoder_polar and decoder_polar members are ignored.  Per scene n_present is 0 or 2 .. n_objects_max and
 * n_edges = n_present * min(knn_k, n_present - 1); a scene with exactly one present object is refused by name, as the engine
 * refuses it for the Aether model (the reference's dNRI itself would run it with zero messages).  Every step of every scene is
 * validated on the host before anything is queued: a refused call has queued nothing and touched no state.  A mask that
 * disagrees with n_present poisons the step's outputs and the state rows it would have written with NaN, and the next call
 * returns AETHER_EHIP (async error word).  The stages are the two entries above (same kernels, same order): results equal
 * the staged calls bit for bit.  The workspace is smaller than aether_dyn_step_batched_workspace_bytes for the same sizes.
 */
size_t aether_dyn_dnri_step_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max,
                                                    const int64_t* n_present, const int64_t* n_edges, const int* in_degree);
int aether_dyn_dnri_step_batched(const AetherDynDnriPriorParams* prior_params, const AetherDynDnriDecoderParams* decoder_params,
                                 const AetherDynStepConfig* config, int n_scenes, int n_objects_max, const int64_t* n_present,
                                 const int64_t* n_edges, const int* in_degree, const float* state, const float* mask,
                                 const int64_t* node_inds, const int64_t* graph_send, const int64_t* graph_recv,
                                 const int64_t* edge2node, float* prior_h, float* prior_c, float* decoder_hidden,
                                 const float* uniform, float* prediction, float* edge_types, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t aether_dyn_dnri_rollout_batched_workspace_bytes(const AetherDynStepConfig* config, int n_scenes, int n_objects_max,
                                                       int n_steps, const int64_t* n_present, const int64_t* n_edges,
                                                       const int* in_degree);
int aether_dyn_dnri_rollout_batched(const AetherDynDnriPriorParams* prior_params, const AetherDynDnriDecoderParams* decoder_params,
                                    const AetherDynStepConfig* config, int n_scenes, int n_objects_max, int n_steps,
                                    const float* inputs, const float* masks, const float* burn_in_masks, const int64_t* n_present,
                                    const int64_t* n_edges, const int* in_degree, const int64_t* const* node_inds,
                                    const int64_t* const* graph_send, const int64_t* const* graph_recv,
                                    const int64_t* const* edge2node, const float* const* uniform, float* prior_h, float* prior_c,
                                    float* decoder_hidden, float* predictions, void* workspace, size_t workspace_bytes,
                                    void* stream);

/*
 * The evaluation half of calculate_loss of both variable-N models (aether_dynamicvars.py:152-207, dnri_dynamicvars.py:70-114),
 * as the inD runner calls it for its validation NLL / KL (is_train=False): two calls per sequence.
 *
 * aether_dyn_sequence_logits / aether_dyn_dnri_sequence_logits replace Encoder.forward (aether_dynamicvars.py:588-670,
 * dnri_dynamicvars.py:463-542) on the F = T - 1 frames of one sequence.  The reference never writes its forward LSTM state
 * back (tmp_state0 / tmp_state1 are built and dropped, :632-635 / :506-509) and its reverse pass never calls reverse_rnn
 * (:657-662 / :531-536), so for every frame t
 *     h_t = LSTMcell(compute_feat_transform(frame t), (0, 0)),  prior = prior_fc_out(h_t),  posterior = encoder_fc_out([h_t | 0])
 * and the frames are independent: they run as F scenes of ONE prior stage -- present rows, the field at them (Aether), the
 * encoder's own kNN graphs and their receiver CSR, the feature transform (the kernels of the prior step), one LSTM kernel from
 * the zero state (no W_hh product, no state loads, no slots) and the two heads, whose layers of equal depth share a launch; the
 * posterior head's first Linear reads the first R of its 2R weight columns in place.
 *   frames [F][n_objects_max][4], masks [F][n_objects_max]; HOST arrays n_present, n_edges [F] with n_edges[t] =
 *   n_present[t] * min(knn_k, n_present[t] - 1);  prior_logits, posterior_logits [sum_t n_edges[t]][K]: frames in time order,
 *   edges in the order of the encoder's kNN graph (aether_knn_edges) -- the layout calculate_loss slices by step (:181-188).
 *   posterior_params: encoder_fc_out, posterior_layers (1..4) Linear layers with ELU between, hidden size posterior_hidden
 *   (a multiple of 16; ignored with one layer); w[0] is [.][2 rnn_hidden].
 * F <= 256 per call; a longer sequence is split by the caller, and the result does not depend on the split.  Refused before
 * anything is queued (AETHER_EINVAL): null pointers, F outside 1..256, an n_edges that disagrees with n_present, and a frame
 * with fewer than two present objects (the reference's encoder drops such a frame from the logits while its loss loop does
 * not; the runner skips such sequences, experiments/ind/train_dynamicvars.py:166-174).  A mask that disagrees with n_present
 * makes every logit NaN and the next call return AETHER_EHIP (async error word).
 *
 * aether_dyn_loss_rollout / aether_dyn_dnri_loss_rollout are the body of calculate_loss's loop (:171-193 / :83-100) for one
 * sequence: for step t the state is inputs[t] when t == 0 or t is teacher-forced (teacher_forcing_steps: -1 = every step,
 * otherwise the steps t < teacher_forcing_steps; teacher_forcing=False is 0), else predictions[t - 1] -- an object that first
 * appears then enters with the all-zero row the reference feeds (:176, :866-868).  Per step: the present rows, the field at
 * them (Aether), the hard Gumbel sample of logits[sum_{s<t} n_edges[s] ...] with uniform[t], and the decoder step on the data
 * set's graph of the step, from a zero decoder state.  No prior stage, no LSTM slots, no kNN graph.
 *   inputs [n_steps (+ 1)][n_objects_max][4], masks [n_steps][n_objects_max]; HOST arrays n_present, n_edges, in_degree
 *   [n_steps] and per-step device pointers graph_send, graph_recv, edge2node, uniform as aether_dyn_rollout takes them;
 *   logits [sum_t n_edges[t]][K]: the slice the caller decodes with (posterior or prior);
 *   predictions [n_steps][n_objects_max][4], zero at absent rows;  edge_types [n_edges[n_steps - 1]][K]: the last step's
 *   one-hot sample, or NULL.
 * Everything is validated on the host before the first launch (the refusals above, plus the in_degree rule of
 * aether_dyn_step_batched): a refused call has queued nothing and written nothing.  No host synchronisation.  The decoder
 * stage is the one of aether_dyn_step (same kernels, same order), computing its own node frames.
 */
typedef struct AetherDynPosteriorParams {
    const float* w[4]; const float* b[4];                      /* encoder_fc_out: [.][2R] first, [K][.] last */
} AetherDynPosteriorParams;
size_t aether_dyn_sequence_logits_workspace_bytes(const AetherDynStepConfig* config, int posterior_layers, int posterior_hidden,
                                                  int n_frames, int n_objects_max, const int64_t* n_present,
                                                  const int64_t* n_edges);
int aether_dyn_sequence_logits(const AetherDynFieldQueryParams* field_params, const AetherDynPriorParams* prior_params,
                               const AetherDynPosteriorParams* posterior_params, const AetherDynStepConfig* config,
                               int posterior_layers, int posterior_hidden, int n_frames, int n_objects_max,
                               const int64_t* n_present, const int64_t* n_edges, const float* frames, const float* masks,
                               float* prior_logits, float* posterior_logits, void* workspace, size_t workspace_bytes,
                               void* stream);
size_t aether_dyn_dnri_sequence_logits_workspace_bytes(const AetherDynStepConfig* config, int posterior_layers,
                                                       int posterior_hidden, int n_frames, int n_objects_max,
                                                       const int64_t* n_present, const int64_t* n_edges);
int aether_dyn_dnri_sequence_logits(const AetherDynDnriPriorParams* prior_params, const AetherDynPosteriorParams* posterior_params,
                                    const AetherDynStepConfig* config, int posterior_layers, int posterior_hidden, int n_frames,
                                    int n_objects_max, const int64_t* n_present, const int64_t* n_edges, const float* frames,
                                    const float* masks, float* prior_logits, float* posterior_logits, void* workspace,
                                    size_t workspace_bytes, void* stream);
size_t aether_dyn_loss_rollout_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int n_steps,
                                               const int64_t* n_present, const int64_t* n_edges, const int* in_degree);
int aether_dyn_loss_rollout(const AetherDynFieldQueryParams* field_params, const AetherDynDecoderParams* decoder_params,
                            const AetherDynStepConfig* config, int n_objects_max, int n_steps, int teacher_forcing_steps,
                            const float* inputs, const float* masks, const int64_t* n_present, const int64_t* n_edges,
                            const int* in_degree, const int64_t* const* graph_send, const int64_t* const* graph_recv,
                            const int64_t* const* edge2node, const float* logits, const float* const* uniform,
                            float* predictions, float* edge_types, void* workspace, size_t workspace_bytes, void* stream);
size_t aether_dyn_dnri_loss_rollout_workspace_bytes(const AetherDynStepConfig* config, int n_objects_max, int n_steps,
                                                    const int64_t* n_present, const int64_t* n_edges, const int* in_degree);
int aether_dyn_dnri_loss_rollout(const AetherDynDnriDecoderParams* decoder_params, const AetherDynStepConfig* config,
                                 int n_objects_max, int n_steps, int teacher_forcing_steps, const float* inputs,
                                 const float* masks, const int64_t* n_present, const int64_t* n_edges, const int* in_degree,
                                 const int64_t* const* graph_send, const int64_t* const* graph_recv,
                                 const int64_t* const* edge2node, const float* logits, const float* const* uniform,
                                 float* predictions, float* edge_types, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Scene pack: the data side of the variable-N family on the device.  Replaces, for B scenes and every frame at once, what
 * the reference's data set builds per scene and per frame on the host (experiments/ind/single_ind_data.py:70-89):
 * node_inds = mask[step].nonzero()[:, -1] (:82) and get_knn_graph_info (:186-217) -- the kNN graph of the frame's
 * ground-truth positions (:193-211) and edge2node_inds = (tmp_inds == recv).nonzero()[:, 1].view(-1, k) (:213-215).
 *   inputs [n_steps (+ 1)][B][n_objects_max][4], masks [n_steps][B][n_objects_max] : TIME-MAJOR, exactly what
 *            aether_dyn_rollout_batched takes (the same tensors serve both calls); the first n_steps frames are read
 *   k      : neighbours per object, 1..16; a scene with n present objects has in_degree = min(k, n - 1) per object.  The
 *            rollout needs k = its config's knn_k.
 *   pack   : device buffer of aether_dyn_scene_pack_bytes(...) bytes, 8-byte aligned.  n_scenes 1..256,
 *            n_objects_max 1..512.
 *   view   : HOST struct, out: device pointers into `pack` and the per-step strides (in elements).  Step t's arrays start
 *            at node_inds + t * node_stride, graph_send / graph_recv / edge2node + t * edge_stride (node_stride =
 *            B * n_objects_max, edge_stride = B * n_objects_max * k: a fixed capacity, so the rollout's per-step pointers are
 *            host arithmetic).  Within a step the scenes with n >= 2 follow one another in scene order, each in its own
 *            compacted numbering: node_inds the present rows, ascending; edges in aether_knn_edges' order (querying object
 *            by querying object, nearest first, equal distances in index order; send = the querying object); edge2node the
 *            scene's edge ids in stable order of graph_recv (argsort(recv, stable=True)), viewed as [n][in_degree].  Only
 *            these entries are written; the rest of each step's capacity is left as it was.
 *   n_present, n_edges, in_degree : HOST arrays [n_steps][B], out, as aether_dyn_rollout_batched takes them.
 * Synchronisation: ONE device-to-host copy (the counts, into pinned memory) and ONE hipStreamSynchronize per call; nothing
 * else is synchronised.  No atomics that could change a result: the same input gives the same bytes.
 * Refused before anything is queued: null pointers, n_scenes outside 1..256, k outside 1..16, n_objects_max outside 1..512
 * (AETHER_EINVAL), pack_bytes too small (AETHER_ESPACE).  Refused after the count copy (AETHER_EINVAL): a (scene, step)
 * with exactly one present object -- the rollout refuses it and the reference fails there; aether_last_error names the
 * first such scene and step.  aether_dyn_scene_pack_bytes is host arithmetic only (0 + aether_last_error on bad sizes).
 */
typedef struct AetherDynScenePack {
    int64_t* node_inds;
    int64_t* graph_send;
    int64_t* graph_recv;
    int64_t* edge2node;
    int64_t node_stride, edge_stride;
} AetherDynScenePack;
size_t aether_dyn_scene_pack_bytes(int n_scenes, int n_objects_max, int n_steps, int k);
int aether_dyn_scene_pack(const float* inputs, const float* masks, int n_scenes, int n_objects_max, int n_steps, int k,
                          void* pack, size_t pack_bytes, AetherDynScenePack* view, int64_t* n_present, int64_t* n_edges,
                          int* in_degree, void* stream);

/*
 * The inD runner's forward-prediction metric (experiments/ind/evaluate.py:29-80) for B scenes per call; the reference
 * computes it at batch 1 with a Python loop over objects and several .item() calls per object.
 *   preds, truth  : [B][n_steps][n_objects_max][feat_stride >= 4] -- predict_future's result and inputs[:, 1:]; the first
 *                   four features enter (:59-62)
 *   masks, burn_in_masks : [B][n_steps + 1][n_objects_max], the latter after the caller applied `strict` (:26-28)
 *   scale[4], offset[4]  : device; the un-normalisation y = scale_f x + offset_f (both modes of single_ind_data.py:122-141)
 *   keep          : [B][n_objects_max] or NULL, the data set's non_linear_masks (:55-58); 0 = skip the track
 *   error_norm    : report_error_norm (:63-68): L2 norms of the position / velocity error instead of their MSE
 * Per track (scene, object): skipped without a burn-in entry (:52); pred_mask = (masks - burn_in_masks)[1:] (:29), `first`
 * its first non-zero step, `num` its sum; the errors of steps first .. first + num - 1, each multiplied by pred_mask, are
 * added to horizons 0 .. num - 1 and counts[h] += pred_mask[first + h] (:76-80).
 *   sums [3][n_steps] (total, position, velocity), counts [n_steps] : device fp64; the call ADDS to them, so a data set is
 *                   a sequence of calls (zero them before the first).  The metric is sums / counts.
 *   stats int64[2]: device; stats[0] += tracks whose predicted steps are not contiguous (the reference's bad count, :72-75);
 *                   stats[1] = max(stats[1], longest pred_mask sum of any track of the call): the length of the reference's
 *                   result (:41-46)
 *   scratch       : aether_dyn_eval_scratch_bytes(...) bytes of device memory, 8-byte aligned; rewritten by every call
 * One wave per track writes its contributions as a row of scratch; a second kernel adds the rows column by column in a
 * fixed order in fp64.  No atomics.  Stream-ordered, no host synchronisation.  Errors are computed in fp64 from the fp32
 * inputs.
 */
size_t aether_dyn_eval_scratch_bytes(int n_scenes, int n_objects_max, int n_steps);
int aether_dyn_eval_accumulate(const float* preds, const float* truth, int feat_stride, const float* masks,
                               const float* burn_in_masks, const float* scale, const float* offset, const float* keep,
                               int error_norm, int n_scenes, int n_objects_max, int n_steps, double* sums, double* counts,
                               int64_t* stats, void* scratch, size_t scratch_bytes, void* stream);

/*
 * The rest of the runner's training step (experiments/lorentz/main.py:86,164,289-292): nn.MSELoss with the seed of its
 * backward, and optim.AdamW over every parameter tensor -- one launch each (torch: 4 + 3).
 *
 * aether_mse_loss_grad: *loss = mean((pred - target)^2), dpred[i] = 2 (pred[i] - target[i]) / n.  scratch: at least
 *   aether_mse_scratch_bytes() bytes of device memory, ZERO before the first call (the kernel re-arms it), not shared by
 *   launches that may run concurrently.  Partial sums are added in a fixed order (bit-stable).
 * aether_adamw_step: torch.optim.AdamW(betas, eps, weight_decay; amsgrad = maximize = False) for n_tensors fp32
 *   tensors (64 per launch).  `step` (device float: steps taken so far, incremented by the launch), `lr` (device float) and `counter`
 *   (device int, zero before the first call) live in device memory, so a captured launch follows the step counter and a
 *   learning-rate schedule.  fp32 arithmetic; the bias corrections 1 - beta^t as -expm1(t log beta), betas in (0, 1).
 *   `grad_scale` multiplies every gradient as it is read (1.0: torch's AdamW exactly): a data-parallel step passes
 *   1 / world_size after the SUM all-reduce of the flat gradient buffer, so the mean needs no launch of its own.
 */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} AetherAdamWTensor;
size_t aether_mse_scratch_bytes(void);
int aether_mse_loss_grad(const float* pred, const float* target, int64_t n, float* loss, float* dpred, void* scratch,
                         size_t scratch_bytes, void* stream);
int aether_adamw_step(const AetherAdamWTensor* tensors, int n_tensors, float* step, const float* lr, int* counter,
                      double beta1, double beta2, double eps, double weight_decay, double grad_scale, void* stream);

/*
 * Tuning knobs (process-wide; not thread-safe); any other name returns AETHER_EINVAL:
 * "fused_split" 0|1 (two workgroups per group when there are fewer groups than half the CUs; default 1; read by
 * aether_graph_build), "fused_waves12" 0|1 (inference step of small-graph groups: when every workgroup has one node
 * tile (<= 16 own nodes) and the largest has 9-12 edge tiles, run the fused kernel with twelve waves and one edge
 * tile per wave instead of eight waves with up to two; same arithmetic, same bits; default 1; read at every
 * launch), "fused_granules" 0|1 (that twelve-wave kernel on a split view: the two workgroups of a group hand their
 * P_s rows over as 8-byte {layer tag, value} granules that the receiver re-reads until every tag matches, instead of
 * rows, a store drain and a flag; same bits; 0 gives the rows + flag protocol of the eight-wave kernels; values other
 * than 0 and 1 are refused; default 1; read at every launch), "graph_build" 0|1 (aether_graph_build_counting: 1, the default, builds by counting; 0 forwards
 * every call to the sorting aether_graph_build), "fused_backward" 0|1 (one-launch backward for small-graph groups; default 1, 0 sends them through
 * the layer-by-layer kernels), "outer_defer_max_edges" n (aether_backward keeps every layer's weight-gradient operands
 * and multiplies them in one launch when n_edges <= n, default 2^20; changes aether_workspace_bytes), "edge_acc"
 * 0|non-zero (above outer_defer_max_edges, non-zero -- the default -- accumulates each layer's edge-level weight gradients
 * inside the edge kernel, 0 writes the rows and multiplies them afterwards; changes aether_workspace_bytes),
 * "linear_kwaves" 1|4 (dense layers of the seq2seq / variable-N steps with few 16 x 32 blocks: the four waves of a
 * workgroup share one block and split its k-groups, partial sums added in wave order; default 4, 1 turns it off),
 * "gemm_split" 0|1|2|3 (dense layers of the fused seq2seq step from 128 workgroups on: 1, the default, multiplies
 * fp16 x 2 pieces on the 16-bit matrix pipe and picks the kernel structure per launch -- both operands through an
 * LDS-DMA ring up to 256 workgroups, X rows in registers above; 2 / 3 force the second / the first structure for
 * every launch; 0 sends these layers through the fp32-MFMA job kernel), "filter_splits" 0|1|2|4|8 (k-splits of the
 * anisotropic-filter GEMM of the seq2seq / variable-N prior steps; default 0, chosen by balance; changes the prior /
 * decoder workspace sizes).
 */
int aether_set_option(const char* name, int value);

/*
 * EGNN-Aether: replaces EGNN_vel_Aether.forward (nn/state2state/egnn_aether.py:65-75) with its layers
 * E_GCL_vel_field (nn/state2state/gcl.py:59-83 on nn/state2state/egnn/gcl.py:E_GCL) and the field net
 * (nn/state2state/aether.py:108-134), the model experiments/lorentz/main.py:147 builds for --model egnn_aether.
 *   params      : n_params = 2 + 15 n_layers + 7 fp32 device tensors in the reference's named_parameters() order:
 *                 embedding.{weight,bias}; per layer gcl_l.edge_mlp.{0,2}.{weight,bias}, node_mlp.{0,2}.{weight,bias},
 *                 coord_mlp.0.{weight,bias}, coord_mlp.2.weight, coord_mlp_vel.{0,2}.{weight,bias};
 *                 field_net.net.{0,2,4}.{weight,bias}, field_net.class_embedding.weight (host array of device pointers)
 *   hidden      : hidden_nf, 64 or 128;  in_node_nf : width of h;  edge_attr : float[E][2] (in_edge_nf = 2 + 6 field)
 *   h           : float[n_nodes][in_node_nf];  x, vel : float[n_nodes][3];  charges : float[n_nodes] in {-1, 0, +1}
 *   graph, info : aether_graph_build(edges[1], edges[0], ...) -- the index rows SWAPPED, so that the view groups the
 *                 edges by edges[0] (row), over which every sum and mean of E_GCL runs (egnn/gcl.py:69-101)
 *   out         : float[n_nodes][3], the returned x.  The caller's x is not written (the reference adds into it in
 *                 place, gcl.py:81 / egnn/gcl.py:97; the runner never reads it again)
 *   flags       : AETHER_EGNN_NORM_DIFF (norm_diff), AETHER_EGNN_TANH (tanh), AETHER_EGNN_KEEP (keep-for-backward form:
 *                 every layer's h, x and row sums of m stay in the workspace for aether_egnn_backward)
 * Per layer one launch (edge MLP, phi, clamp and both row sums in the edge loop of a node's workgroup; psi, the x update,
 * node_mlp and the residual after it).  Deterministic: no float atomics.  fp32 throughout (csrc/egnn.h).
 */
#define AETHER_EGNN_NORM_DIFF 1
#define AETHER_EGNN_TANH 2
#define AETHER_EGNN_KEEP 4
size_t aether_egnn_workspace_bytes(int hidden, int n_layers, int in_node_nf, int64_t n_nodes, int64_t n_edges,
                                   int keep_for_backward);
int aether_egnn_forward(const float* const* params, int n_params, int hidden, int n_layers, int in_node_nf, int flags,
                        int64_t n_nodes, int64_t n_edges, const float* h, const float* x, const float* vel,
                        const float* edge_attr, const float* charges, const void* graph, const AetherGraphInfo* info,
                        void* workspace, size_t workspace_bytes, float* out, void* stream);
/*
 * Parameter gradients of a loss given dL/d(out) (grad_out, float[n_nodes][3]): replaces loss.backward() through
 * EGNN_vel_Aether (experiments/lorentz/main.py:254-292; the runner detaches every input, so no input gradient).
 * Reads the workspace of an aether_egnn_forward(... AETHER_EGNN_KEEP) with the same arguments.  OVERWRITES `grad`:
 * one flat fp32 buffer, every parameter at the next multiple of 4 floats in named_parameters() order (the drop-in's
 * _grad_buffers layout), aether_egnn_grad_floats() floats.  Where the +-100 clamp of the translation is active the
 * gradient is zero, as in torch.  Weight gradients: row chunks summed in a fixed order (no atomics).
 */
int aether_egnn_backward(const float* const* params, int n_params, int hidden, int n_layers, int in_node_nf, int flags,
                         int64_t n_nodes, int64_t n_edges, const float* h, const float* x, const float* vel,
                         const float* edge_attr, const float* charges, const void* graph, const AetherGraphInfo* info,
                         void* workspace, size_t workspace_bytes, const float* grad_out, float* grad, int64_t grad_floats,
                         void* stream);
int64_t aether_egnn_grad_floats(int hidden, int n_layers, int in_node_nf);
/* Byte offset, in a keep-for-backward workspace, of "field" (float[n_nodes][3]) or of layer `layer`'s input "h"
 * (float[n_nodes][hidden]) / "x" (float[n_nodes][3]); layer n_layers is the model's last h / output x.  Tests. */
int64_t aether_egnn_workspace_offset(const char* name, int layer, int hidden, int n_layers, int in_node_nf, int64_t n_nodes,
                                     int64_t n_edges);
/*
 * Autoregressive rollout of EGNN-Aether, all on the device: `steps` forward steps back to back,
 *   x_{t+1} = EGNN_vel_Aether(|v_t|, x_t, v_t, edge_attr_t),  v_{t+1} = (x_{t+1} - x_t) / dt,
 * with h = |v_t| (the runner's `nodes`, in_node_nf = 1) and edge_attr_t = [q_row q_col, |x_row - x_col|^2] rebuilt from
 * the current positions by one state kernel per step (csrc/gnn_common.h: k_gnn_rollout_state) -- the runner's per-batch
 * preparation, experiments/lorentz/main.py:254-259, under the protocol of the "20-step rollout MSE" metric (SURVEY.md
 * 8d).  Replaces a Python loop of model calls with a gather, a norm and a concatenation per step; the transposed weight
 * images, which aether_egnn_forward writes per call, are written once per rollout.  The charge product is written at
 * step 0 only.
 *   x0, vel0   : float[n_nodes][3], state at t = 0 (not modified);  charges : float[n_nodes]
 *   send, recv : int64[n_edges], the index arrays graph was built from (send = edges[1], recv = edges[0])
 *   trajectory : float[steps][n_nodes][3], positions x_1 .. x_steps (step t reads row t - 1 and writes row t)
 *   workspace  : aether_egnn_rollout_workspace_bytes() bytes: the inference workspace of aether_egnn_forward, then vel,
 *                h and edge_attr of the step about to run
 *   flags      : AETHER_EGNN_NORM_DIFF, AETHER_EGNN_TANH.  AETHER_EGNN_KEEP and in_node_nf != 1 are errors
 * steps <= 0 returns 0 and writes nothing.  Launches only (no allocation, no synchronisation, nothing read back):
 * stream-ordered, deterministic; capture it in a hipGraph to replay a whole rollout with one launch.
 */
size_t aether_egnn_rollout_workspace_bytes(int hidden, int n_layers, int in_node_nf, int64_t n_nodes, int64_t n_edges);
int aether_egnn_rollout(const float* const* params, int n_params, int hidden, int n_layers, int in_node_nf, int flags,
                        int64_t n_nodes, int64_t n_edges, const float* x0, const float* vel0, const float* charges,
                        const int64_t* send, const int64_t* recv, const void* graph, const AetherGraphInfo* info,
                        void* workspace, size_t workspace_bytes, float* trajectory, int steps, float dt, void* stream);

/*
 * ClofNet: replaces the forward of ClofNet / ClofNet_vel / ClofNet_vel_gbf (nn/state2state/clof/clof.py:86-101, 187-202,
 * 285-302) with their layers Clof_GCL (nn/state2state/clof/gcl.py:54-66 on nn/state2state/egnn/gcl.py:E_GCL), the models
 * experiments/lorentz/main.py:152-157 builds for --model clof, clof_vel and clof_vel_gbf.
 *   variant     : 0 ClofNet, 1 ClofNet_vel, 2 ClofNet_vel_gbf
 *   params      : n_params = head + 19 n_layers fp32 device tensors in the reference's named_parameters() order:
 *                 embedding_node.{weight,bias}; then ClofNet embedding_edge.0.{weight,bias} (never used, clof.py:93),
 *                 fuse_edge.{0,2}.{weight,bias} (head 8); ClofNet_vel fuse_edge.{0,2}.{weight,bias} (head 6);
 *                 ClofNet_vel_gbf gbf.{means,stds,mul,bias}.weight, fuse_edge.{0,2}.{weight,bias} (head 10); per layer
 *                 gcl_l.edge_mlp.{0,2,4}.{weight,bias}, node_mlp.{0,2}.{weight,bias}, coord_mlp.0.{weight,bias},
 *                 coord_mlp.2.weight, coord_mlp_vel.{0,2}.{weight,bias}, layer_norm.{weight,bias}
 *   hidden      : hidden_nf, 64 or 128;  in_node_nf : width of h;  edge_attr : float[E][2] ([q_row q_col, |x_row - x_col|^2])
 *   h           : float[n_nodes][in_node_nf];  x, vel : float[n_nodes][3]
 *   n_per_graph : the forward's n_nodes argument: x is centred per block of n_per_graph rows (clof.py:88-90)
 *   graph, info : aether_graph_build(edges[1], edges[0], ...) -- the index rows SWAPPED, so that the view groups the
 *                 edges by edges[0] (row), over which every sum and mean of Clof_GCL runs
 *   out         : float[n_nodes][3], the returned x.  The caller's x is not written.
 *   flags       : AETHER_CLOF_NORM_DIFF (the layers' norm_diff; ClofNet also scalarizes with it, the _vel variants always
 *                 normalise there, clof.py:113,190), AETHER_CLOF_TANH, AETHER_CLOF_RECURRENT, AETHER_CLOF_KEEP
 *                 (keep-for-backward form: every layer's h, x and pre-activations stay in the workspace)
 * The cross products are per edge.  torch.cross without dim (gcl.py:29, clof.py:69) takes the first axis of size 3,
 * which is the edge axis when there are exactly 3 edges; this entry always takes the per-edge product.  The Gaussian
 * layer's edge type (edge_attr[:, 0] * 0.5 + 0.5, truncated) is clamped to [0, 7] (the reference raises an index error
 * outside it).  Deterministic: no float atomics.  fp32 throughout, edge MLPs on fp32 MFMA (csrc/clof.h).
 */
#define AETHER_CLOF_NORM_DIFF 1
#define AETHER_CLOF_TANH 2
#define AETHER_CLOF_KEEP 4
#define AETHER_CLOF_RECURRENT 8
size_t aether_clof_workspace_bytes(int variant, int hidden, int n_layers, int in_node_nf, int64_t n_nodes, int64_t n_edges,
                                   int keep_for_backward);
int aether_clof_forward(const float* const* params, int n_params, int variant, int hidden, int n_layers, int in_node_nf,
                        int flags, float coords_weight, int n_per_graph, int64_t n_nodes, int64_t n_edges, const float* h,
                        const float* x, const float* vel, const float* edge_attr, const void* graph,
                        const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, float* out, void* stream);
/*
 * Parameter gradients of a loss given dL/d(out) (grad_out, float[n_nodes][3]): replaces loss.backward() through the
 * ClofNet models (experiments/lorentz/main.py:266-292; the runner detaches every input, so no input gradient).  Reads the
 * workspace of an aether_clof_forward(... AETHER_CLOF_KEEP) with the same arguments.  Writes `grad`: one flat fp32
 * buffer, every parameter at the next multiple of 4 floats in named_parameters() order (the drop-in's _grad_buffers
 * layout), aether_clof_grad_floats() floats.  Parameters that do not reach the output -- the last layer's node_mlp and
 * layer_norm, ClofNet's embedding_edge -- are not written.  Where the +-100 clamp of the translation is active the
 * gradient is zero, as in torch.  Weight gradients: fp32 MFMA over row chunks summed in a fixed order (no atomics).
 */
int aether_clof_backward(const float* const* params, int n_params, int variant, int hidden, int n_layers, int in_node_nf,
                         int flags, float coords_weight, int n_per_graph, int64_t n_nodes, int64_t n_edges, const float* h,
                         const float* x, const float* vel, const float* edge_attr, const void* graph,
                         const AetherGraphInfo* info, void* workspace, size_t workspace_bytes, const float* grad_out,
                         float* grad, int64_t grad_floats, void* stream);
int64_t aether_clof_grad_floats(int variant, int hidden, int n_layers, int in_node_nf);
/* Byte offset, in a keep-for-backward workspace, of "edge_feat" (float[n_edges][hidden / 2], row-sorted order) or of
 * layer `layer`'s input "h" (float[n_nodes][hidden]) / centred "x" (float[n_nodes][3]); layer n_layers is the last
 * layer's output.  Tests. */
int64_t aether_clof_workspace_offset(const char* name, int layer, int variant, int hidden, int n_layers, int in_node_nf,
                                     int64_t n_nodes, int64_t n_edges);
/*
 * aether_egnn_rollout for the ClofNet models: x_{t+1} = ClofNet*(|v_t|, x_t, v_t, edge_attr_t, n_nodes = n_per_graph),
 * v_{t+1} = (x_{t+1} - x_t) / dt, the runner's preparation of experiments/lorentz/main.py:266-271 done by the same state
 * kernel; the packed weight images of aether_clof_forward are written once per rollout.  ClofNet's forward takes no
 * charges: they are read here only for the charge product in edge_attr[:, 0].  Arguments as aether_egnn_rollout and
 * aether_clof_forward; workspace aether_clof_rollout_workspace_bytes() bytes; AETHER_CLOF_KEEP and in_node_nf != 1 are
 * errors.
 */
size_t aether_clof_rollout_workspace_bytes(int variant, int hidden, int n_layers, int in_node_nf, int64_t n_nodes,
                                           int64_t n_edges);
int aether_clof_rollout(const float* const* params, int n_params, int variant, int hidden, int n_layers, int in_node_nf,
                        int flags, float coords_weight, int n_per_graph, int64_t n_nodes, int64_t n_edges, const float* x0,
                        const float* vel0, const float* charges, const int64_t* send, const int64_t* recv,
                        const void* graph, const AetherGraphInfo* info, void* workspace, size_t workspace_bytes,
                        float* trajectory, int steps, float dt, void* stream);

/*
 * A kernel cannot return a status.  The one bounded wait in the library -- a split-mode workgroup of the fused
 * kernel polling for its partner's rows -- sets a word in host-mapped memory when it gives up (partner not
 * resident within ~seconds); the results of that launch are then invalid.  Every launching entry point checks and
 * clears the word first (so the NEXT call returns AETHER_EHIP), and this function does so on request, e.g. after
 * synchronising the stream.  Returns AETHER_OK or AETHER_EHIP (message in aether_last_error).
 */
int aether_check_async_error(void);

/*
 * Per-kernel timing for bench.py's roofline line: when enabled, every launch made by
 * aether_forward is bracketed by a pair of HIP events on the launch stream.
 * aether_profile_read synchronises those events, adds up elapsed milliseconds and launch
 * counts per kernel id (0 .. aether_profile_kernels()-1) and clears the record.
 * Not thread-safe; measurement only (the event records perturb back-to-back launches).
 */
int aether_profile_enable(int on);
int aether_profile_kernels(void);
const char* aether_profile_kernel_name(int id);
int aether_profile_read(double* total_ms, int64_t* launches, int n);

#ifdef __cplusplus
}
#endif
#endif /* AETHER_HIP_H */
