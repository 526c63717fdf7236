"""What every model on the scene engine (``AetherDynamicVars``, ``DNRIDynamicVars``) and its stages share on the host: the
step configuration, device scene packs, the tensor conversions and the cached workspace."""
from __future__ import annotations

import ctypes as C

import torch

from ... import _lib


def f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def i64(t, dev):
    return t.to(device=dev, dtype=torch.int64).contiguous()


def cached_workspace(owner, attr, need, dev, capture_check=None):
    """``owner``'s cached byte buffer ``attr`` (``_ws`` of a stage, ``_step_ws`` of a model), replaced when it is smaller than
    ``need`` or on another device.  ``capture_check``: the refusal to raise instead of allocating under stream capture (a
    captured graph bakes the old address in)."""
    ws = owner.__dict__.get(attr)
    if ws is None or ws.numel() < need or ws.device != dev:
        if capture_check and torch.cuda.is_current_stream_capturing():
            raise _lib.AetherHipError(capture_check)
        ws = owner.__dict__[attr] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


_DynStepConfig = _lib.AetherDynStepConfig


class ScenePack:
    """The per-frame graphs of B scenes, built on the device by ``pack_scenes`` (``aether_dyn_scene_pack``): what the
    reference's data set keeps as Python lists per scene and per frame (experiments/ind/single_ind_data.py:70-89).
    ``buf`` holds the arrays, ``view`` the device pointers and per-frame strides into it, ``n_present`` / ``n_edges`` /
    ``in_degree`` the host arrays [n_frames][B] the rollout takes as they are."""

    def __init__(self, buf, view, n_present, n_edges, in_degree, n_scenes, n_frames, n_objects_max, k):
        self.buf, self.view, self.n_present, self.n_edges, self.in_degree = buf, view, n_present, n_edges, in_degree
        self.n_scenes, self.n_frames, self.n_objects_max, self.k = n_scenes, n_frames, n_objects_max, k

    def _frames(self, ptr, stride):
        """[n_frames][stride] int64 view of one of the pack's arrays."""
        lo = ptr - self.buf.data_ptr()
        return self.buf[lo:lo + self.n_frames * stride * 8].view(torch.int64).view(self.n_frames, stride)

    def arrays(self):
        """(node_inds [n_frames][B Nmax], graph_send, graph_recv, edge2node [n_frames][B Nmax k]): views into the pack; of
        frame t the first sum_b n_present[t][b] / sum_b n_edges[t][b] entries are meaningful."""
        v = self.view
        return (self._frames(v.node_inds, v.node_stride), self._frames(v.graph_send, v.edge_stride),
                self._frames(v.graph_recv, v.edge_stride), self._frames(v.edge2node, v.edge_stride))

    def counts(self):
        """(n_present, n_edges, in_degree) as host int64 tensors [n_frames][B]."""
        shape = (self.n_frames, self.n_scenes)
        return tuple(torch.tensor(list(a), dtype=torch.int64).view(shape) for a in (self.n_present, self.n_edges,
                                                                                     self.in_degree))

    def as_lists(self):
        """-> (node_inds[b][t], graph_info[b][t] = (send, recv, edge2node [n][in_degree])): views into the pack, in the form
        ``predict_future`` takes (the compatibility path: this is per-(scene, frame) Python again)."""
        ni, gs, gr, e2n = self.arrays()
        n, e, d = (c.tolist() for c in self.counts())
        B = self.n_scenes
        node_inds, graph_info = [[] for _ in range(B)], [[] for _ in range(B)]
        for t in range(self.n_frames):
            no = eo = 0
            for b in range(B):
                nb, eb = n[t][b], e[t][b]
                node_inds[b].append(ni[t, no:no + nb])
                graph_info[b].append((gs[t, eo:eo + eb], gr[t, eo:eo + eb],
                                      e2n[t, eo:eo + eb].view(nb, d[t][b]) if nb else e2n[t, eo:eo].view(0, 1)))
                no += nb; eo += eb
        return node_inds, graph_info


@torch.no_grad()
def pack_scenes(inputs, masks, k=10):
    """inputs [B, T, Nmax, 4], masks [B, T, Nmax] (device) -> ``ScenePack`` of all T frames: present rows, kNN graph of the
    ground-truth positions (``k`` neighbours) and edge2node per (scene, frame), in ONE library call with one
    device-to-host copy (the counts).  Raises if a scene has exactly one present object in a frame."""
    if not inputs.is_cuda:
        raise _lib.AetherHipError("pack_scenes runs on an MI355X only; got a CPU tensor (there is no CPU fallback)")
    lib = _lib.load()
    dev = inputs.device
    B, T, Nmax = int(inputs.size(0)), int(inputs.size(1)), int(inputs.size(2))
    if inputs.size(-1) != 4 or tuple(masks.shape) != (B, T, Nmax):
        raise ValueError("pack_scenes: inputs must be [B, T, Nmax, 4] and masks [B, T, Nmax]")
    x = inputs.detach().to(torch.float32).transpose(0, 1).contiguous()                  # time-major, as the rollout takes it
    m = masks.detach().to(device=dev, dtype=torch.float32).transpose(0, 1).contiguous()
    need = lib.aether_dyn_scene_pack_bytes(B, Nmax, T, int(k))
    if need == 0:
        raise _lib.AetherHipError("aether_dyn_scene_pack_bytes: " + lib.aether_last_error().decode())
    buf = torch.empty(need, dtype=torch.uint8, device=dev)
    view = _lib.AetherDynScenePack()
    n_present, n_edges, in_degree = (C.c_int64 * (T * B))(), (C.c_int64 * (T * B))(), (C.c_int * (T * B))()
    st = lib.aether_dyn_scene_pack(x.data_ptr(), m.data_ptr(), B, Nmax, T, int(k), buf.data_ptr(), buf.numel(), C.byref(view),
                                   n_present, n_edges, in_degree, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(st, "aether_dyn_scene_pack")
    return ScenePack(buf, view, n_present, n_edges, in_degree, B, T, Nmax, int(k))
