// host_graph_build.inc -- aether_graph_build_counting: the graph view of aether_graph_build by the counting sort of
// graph_build.h.  Six launches and one device-to-host copy in front of the host tables; two stream synchronisations.
// Included by aether_hip.hip inside extern "C".

// Pinned host memory for the one copy back (flag, cross, rowptr), kept per thread and grown when a graph needs more.
static int32_t* graph_build_host_words(size_t words) {
    static thread_local int32_t* buf = nullptr;
    static thread_local size_t cap = 0;
    if (words > cap) {
        if (buf) (void)hipHostFree(buf);
        buf = nullptr; cap = 0;
        void* p = nullptr;
        const size_t want = words < 16384 ? 16384 : words + words / 2;
        if (hipHostMalloc(&p, want * 4, hipHostMallocPortable) != hipSuccess) return nullptr;
        buf = (int32_t*)p; cap = want;
    }
    return buf;
}

int aether_graph_build_counting(const int64_t* send, const int64_t* recv, int64_t n_edges, int64_t n_nodes,
                                void* graph, size_t graph_bytes, AetherGraphInfo* info, void* stream) {
    // Bad arguments (aether_graph_build reports them), an empty edge list, more counters than one workgroup scans, or
    // option "graph_build" 0: the sorting builder.
    const bool counting = g_graph_build != 0 && n_nodes > 0 && n_nodes + 1 <= GB_SCAN_MAX && n_edges > 0 &&
                          n_edges < ((int64_t)1 << 31) && graph && info && send && recv;
    if (!counting) return aether_graph_build(send, recv, n_edges, n_nodes, graph, graph_bytes, info, stream);
    GraphLayout G(n_edges, n_nodes);
    if (graph_bytes < G.total) return fail(AETHER_ESPACE, "graph_build: graph buffer too small");
    memset(info, 0, sizeof(*info));
    info->n_nodes = n_nodes;
    info->n_edges = n_edges;
    hipStream_t st = (hipStream_t)stream;
    char* g = (char*)graph;
    int32_t *rowptr = (int32_t*)(g + G.rowptr), *srowptr = (int32_t*)(g + G.srowptr);
    int32_t *diff = (int32_t*)(g + G.diff), *cross = (int32_t*)(g + G.cross), *flag = (int32_t*)(g + G.flag);
    int32_t *perm = (int32_t*)(g + G.perm), *recv_s = (int32_t*)(g + G.recv_s), *send_s = (int32_t*)(g + G.send_s);
    int32_t* sperm = (int32_t*)(g + G.sperm);
    // scratch of the sorting builder: every edge's slot in its receiver's / its sender's list
    int32_t *slot_r = (int32_t*)(g + G.vals), *slot_s = (int32_t*)(g + G.keys);
    // diff | cross | flag lie behind one another (GraphLayout): one copy brings back rowptr (k_gb_scan's copy in
    // diff), cross and the two flag words
    const size_t back_words = (G.flag - G.diff) / 4 + 2;
    int32_t* h = graph_build_host_words(back_words);
    if (!h) return fail(AETHER_EHIP, "graph_build: no pinned host memory");
    const unsigned edge_blocks = (unsigned)((n_edges + 255) / 256);
    k_gb_zero<<<dim3((unsigned)((n_nodes + 2 + 255) / 256)), dim3(256), 0, st>>>(rowptr, srowptr, diff, flag, n_nodes);
    k_gb_count<<<dim3(edge_blocks), dim3(256), 0, st>>>(send, recv, n_edges, n_nodes, rowptr, srowptr, diff, slot_r,
                                                        slot_s, flag);
    k_gb_scan<<<dim3(1), dim3(GB_SCAN_THREADS), 0, st>>>(rowptr, srowptr, diff, cross, (int)(n_nodes + 1), flag);
    HIP_OK(hipMemcpyAsync(h, diff, back_words * 4, hipMemcpyDeviceToHost, st));
    // the rest of the device work runs under the copy and the host's wait; lists longer than GB_CAP are left as they
    // are (the fallback below rebuilds everything)
    k_gb_place<<<dim3(edge_blocks), dim3(256), 0, st>>>(recv, n_edges, n_nodes, rowptr, slot_r, perm);
    k_gb_recv<<<dim3((unsigned)n_nodes), dim3(64), 0, st>>>(send, n_nodes, rowptr, srowptr, slot_s, perm, recv_s, send_s,
                                                            sperm);
    k_gb_send<<<dim3((unsigned)(n_nodes + (n_edges + 15) / 16)), dim3(64), 0, st>>>(
        (int)n_nodes, srowptr, sperm, recv_s, n_edges, (uint32_t*)(g + G.gsel));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    const int32_t* h_flag = h + (G.flag - G.diff) / 4;
    if (h_flag[0]) return fail(AETHER_EINDEX, "graph_build: edge index outside [0, n_nodes)");
    if (h_flag[1] > GB_CAP) return aether_graph_build(send, recv, n_edges, n_nodes, graph, graph_bytes, info, stream);
    return graph_build_tables(G, g, n_edges, n_nodes, h + (G.cross - G.diff) / 4, h, info, st);
}
