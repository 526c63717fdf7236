// host_dyn_pack.inc -- aether_dyn_scene_pack (dyn_pack.h) and aether_dyn_eval_accumulate (dyn_eval.h): the data side and
// the metric of the variable-N family.  Included by aether_hip.hip inside extern "C", after host_graph_build.inc (whose
// pinned words carry the one copy back).

namespace {
struct DynPackLayout {
    size_t node, send, recv, e2n, counts, node_off, edge_off, total;
    int64_t node_stride, edge_stride;
    DynPackLayout(int B, int N, int steps, int k) {
        node_stride = (int64_t)B * N;
        edge_stride = node_stride * k;
        const size_t nb = align_up((size_t)steps * node_stride * 8, 256), eb = align_up((size_t)steps * edge_stride * 8, 256);
        const size_t cb = align_up((size_t)steps * B * 4, 256);
        node = 0; send = node + nb; recv = send + eb; e2n = recv + eb;
        counts = e2n + eb; node_off = counts + cb; edge_off = node_off + cb; total = edge_off + cb;
    }
};
bool dyn_pack_sizes_ok(int n_scenes, int n_objects_max, int n_steps, int k) {
    if (n_scenes < 1 || n_scenes > DP_MAX_SCENES) { fail(AETHER_EINVAL, "dyn_scene_pack: n_scenes must be 1..256"); return false; }
    if (k < 1 || k > KNN_MAX_K) { fail(AETHER_EINVAL, "dyn_scene_pack: k must be 1..16"); return false; }
    if (n_objects_max < 1 || n_objects_max > DP_MAX_OBJECTS) {
        fail(AETHER_EINVAL, "dyn_scene_pack: n_objects_max must be 1..512");
        return false;
    }
    if (n_steps < 1 || (int64_t)n_steps * n_scenes > (1 << 22)) {
        fail(AETHER_EINVAL, "dyn_scene_pack: n_steps must be positive and n_steps * n_scenes at most 2^22");
        return false;
    }
    return true;
}
}  // namespace

size_t aether_dyn_scene_pack_bytes(int n_scenes, int n_objects_max, int n_steps, int k) {
    if (!dyn_pack_sizes_ok(n_scenes, n_objects_max, n_steps, k)) return 0;
    return DynPackLayout(n_scenes, n_objects_max, n_steps, k).total;
}

int aether_dyn_scene_pack(const float* inputs, const float* masks, int n_scenes, int n_objects_max, int n_steps, int k,
                          void* pack, size_t pack_bytes, AetherDynScenePack* view, int64_t* n_present, int64_t* n_edges,
                          int* in_degree, void* stream) {
    if (!inputs || !masks || !pack || !view || !n_present || !n_edges || !in_degree)
        return fail(AETHER_EINVAL, "dyn_scene_pack: null pointer");
    if (!dyn_pack_sizes_ok(n_scenes, n_objects_max, n_steps, k)) return AETHER_EINVAL;
    if (((size_t)pack & 7) != 0) return fail(AETHER_EINVAL, "dyn_scene_pack: pack must be 8-byte aligned");
    const int B = n_scenes, N = n_objects_max;
    const DynPackLayout L(B, N, n_steps, k);
    if (pack_bytes < L.total) return fail(AETHER_ESPACE, "dyn_scene_pack: pack buffer too small");
    const size_t S = (size_t)n_steps * B;
    int32_t* h = graph_build_host_words(S);
    if (!h) return fail(AETHER_EHIP, "dyn_scene_pack: no pinned host memory");
    char* p = (char*)pack;
    view->node_inds = (int64_t*)(p + L.node);
    view->graph_send = (int64_t*)(p + L.send);
    view->graph_recv = (int64_t*)(p + L.recv);
    view->edge2node = (int64_t*)(p + L.e2n);
    view->node_stride = L.node_stride;
    view->edge_stride = L.edge_stride;
    int *counts = (int*)(p + L.counts), *node_off = (int*)(p + L.node_off), *edge_off = (int*)(p + L.edge_off);
    hipStream_t st = (hipStream_t)stream;
    k_dp_count<<<dim3((unsigned)n_steps), dim3(DP_THREADS), 0, st>>>(masks, B, N, k, counts, node_off, edge_off);
    HIP_OK(hipMemcpyAsync(h, counts, S * 4, hipMemcpyDeviceToHost, st));
    // the build runs under the copy and the host's wait
    k_dp_build<<<dim3((unsigned)S), dim3(DP_THREADS), dp_build_lds_bytes(N, k), st>>>(
        inputs, masks, B, N, k, node_off, edge_off, view->node_inds, view->graph_send, view->graph_recv, view->edge2node,
        L.node_stride, L.edge_stride);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    for (size_t i = 0; i < S; ++i) {
        const int n = h[i];
        if (n == 1) {
            snprintf(g_err, sizeof(g_err), "dyn_scene_pack: scene %d has exactly one present object at step %d "
                     "(a step needs 0 or 2..n_objects_max)", (int)(i % B), (int)(i / B));
            return AETHER_EINVAL;
        }
        const int deg = n >= 2 ? (k < n - 1 ? k : n - 1) : 0;
        n_present[i] = n;
        n_edges[i] = (int64_t)n * deg;
        in_degree[i] = deg;
    }
    return AETHER_OK;
}

size_t aether_dyn_eval_scratch_bytes(int n_scenes, int n_objects_max, int n_steps) {
    if (n_scenes < 1 || n_objects_max < 1 || n_steps < 1 || (int64_t)n_scenes * n_objects_max > (1 << 24) ||
        (int64_t)n_steps > (1 << 16)) {
        fail(AETHER_EINVAL, "dyn_eval: n_scenes, n_objects_max, n_steps must be positive (at most 2^24 tracks, 2^16 steps)");
        return 0;
    }
    const size_t tracks = (size_t)n_scenes * n_objects_max;
    return align_up(tracks * 4 * n_steps * 8, 256) + align_up(tracks * 2 * 4, 256);
}

int aether_dyn_eval_accumulate(const float* preds, const float* truth, int feat_stride, const float* masks,
                               const float* burn_in_masks, const float* scale, const float* offset, const float* keep,
                               int error_norm, int n_scenes, int n_objects_max, int n_steps, double* sums, double* counts,
                               int64_t* stats, void* scratch, size_t scratch_bytes, void* stream) {
    if (!preds || !truth || !masks || !burn_in_masks || !scale || !offset || !sums || !counts || !stats || !scratch)
        return fail(AETHER_EINVAL, "dyn_eval: null pointer");
    if (feat_stride < 4) return fail(AETHER_EINVAL, "dyn_eval: feat_stride must be at least 4");
    const size_t need = aether_dyn_eval_scratch_bytes(n_scenes, n_objects_max, n_steps);
    if (need == 0) return AETHER_EINVAL;
    if (((size_t)scratch & 7) != 0) return fail(AETHER_EINVAL, "dyn_eval: scratch must be 8-byte aligned");
    if (scratch_bytes < need) return fail(AETHER_ESPACE, "dyn_eval: scratch too small");
    const int tracks = n_scenes * n_objects_max;
    double* rows = (double*)scratch;
    int* flags = (int*)((char*)scratch + align_up((size_t)tracks * 4 * n_steps * 8, 256));
    hipStream_t st = (hipStream_t)stream;
    k_de_track<<<dim3((unsigned)((tracks + DE_WAVES - 1) / DE_WAVES)), dim3(64 * DE_WAVES), 0, st>>>(
        preds, truth, feat_stride, masks, burn_in_masks, scale, offset, keep, error_norm ? 1 : 0, tracks, n_objects_max,
        n_steps, rows, flags);
    k_de_reduce<<<dim3((unsigned)((4 * n_steps + 1 + 255) / 256)), dim3(256), 0, st>>>(rows, flags, tracks, n_steps, sums,
                                                                                     counts, stats);
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
