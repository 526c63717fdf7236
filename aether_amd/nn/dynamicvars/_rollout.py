"""Host marshalling of the variable-N prediction loop, shared by the models of the family (``AetherDynamicVars``,
``DNRIDynamicVars``): ``predict_future`` of B scenes as ONE library call, from per-(scene, step) lists or from a ``ScenePack``.
The model supplies its configuration (``_step_config``) and its two entries with their parameter structs
(``_rollout_entries``); everything else -- time-major tensors, host size arrays, per-step pointer tables, the edge2node range
check, the workspace, the initial states -- is the same for every model on the scene engine.
"""
from __future__ import annotations

import ctypes as C

import torch

from ... import _lib


class SceneRolloutMixin:
    """``_rollout_entries(lib) -> (workspace_bytes_fn, rollout_fn, name, head)``: the model's ``*_rollout_batched_workspace_bytes``
    and ``*_rollout_batched`` entries, the latter's name for error messages, and the ``C.byref`` parameter structs it takes in
    front of the configuration."""

    def _rollout_guard(self, inputs):
        if not inputs.is_cuda:
            raise _lib.AetherHipError(f"aether_amd {type(self).__name__} runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        if self.encoder.training:
            raise _lib.AetherHipError("the prior step uses BatchNorm running statistics: call .eval() first")

    def _rollout_call(self, lib, cfg, B, Nmax, n_steps, inputs, x, m, burn, n_host, e_host, deg, ptrs):
        """Workspace, initial states and the one library call -> predictions [n_steps][B][Nmax][4] (time-major)."""
        dev = inputs.device
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        ws_bytes, rollout, name, head = self._rollout_entries(lib)
        need = ws_bytes(C.byref(cfg), B, Nmax, n_steps, n_host, e_host, deg)
        if need == 0:
            raise _lib.AetherHipError(f"{name}_workspace_bytes failed: " + lib.aether_last_error().decode())
        ws = self.__dict__.get("_step_ws")
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self.__dict__["_step_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        prior_h, prior_c = (f32(s)[0].clone() for s in self.encoder.get_initial_hidden(inputs))
        dec = f32(self.decoder.get_initial_hidden(inputs)).clone()                       # [B][Nmax][hd]
        preds = torch.empty(n_steps, B, Nmax, 4, dtype=torch.float32, device=dev)
        st = rollout(*head, C.byref(cfg), B, Nmax, n_steps, x.data_ptr(), m.data_ptr(), burn.data_ptr(), n_host, e_host, deg,
                     ptrs["ni"], ptrs["gs"], ptrs["gr"], ptrs["e2n"], ptrs["u"], prior_h.data_ptr(), prior_c.data_ptr(),
                     dec.data_ptr(), preds.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, name)
        return preds

    @torch.no_grad()
    def _predict_future_rollout(self, inputs, masks, node_inds, graph_info, burn_in_masks, uniform=None, return_pack=False):
        """``predict_future`` of B scenes (B = 1 included) as ONE library call (``*_rollout_batched``): per step the burn-in mix
        and the batched step over the present objects of all scenes, queued on the current stream without a host round trip
        in between.  The per-scene index arrays of a step are concatenated in scene order (scene-local numbering); the time
        axis comes first in what the library sees.  ``uniform[t][b]``: the Gumbel draws of scene b at step t ([E, K]); drawn
        here, one ``torch.rand`` per step that has edges, when omitted.  ``return_pack``: also return the arrays handed to the
        library (the tests call the C entry points with them)."""
        self._rollout_guard(inputs)
        lib = _lib.load()
        dev = inputs.device
        B, T, Nmax = int(inputs.size(0)), int(inputs.size(1)), int(inputs.size(2))
        n_steps, K = T - 1, self.num_edge_types
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        i64 = lambda t: t.to(device=dev, dtype=torch.int64).contiguous()
        # time-major (views of the caller's tensors when B = 1: a dimension of size one has no stride to speak of)
        x = f32(inputs).transpose(0, 1).contiguous()                                   # [T][B][Nmax][4]
        m = f32(masks)[:, :n_steps].transpose(0, 1).contiguous()                       # [n_steps][B][Nmax]
        burn = f32(burn_in_masks)[:, :n_steps].transpose(0, 1).contiguous()
        if m.shape[0] < n_steps or burn.shape[0] < n_steps:
            raise ValueError("masks / burn_in_masks must cover every step")
        n_host = (C.c_int64 * (n_steps * B))()
        e_host = (C.c_int64 * (n_steps * B))()
        deg = (C.c_int * (n_steps * B))()
        ptrs = {k: (C.c_void_p * n_steps)() for k in ("ni", "gs", "gr", "e2n", "u")}
        keep, e2n_range = [], []                                   # device tensors the pointer arrays refer to; (step, lo, hi, limit)
        for t in range(n_steps):
            live = {k: [] for k in ptrs}
            bounds = []
            for b in range(B):
                n_b = int(node_inds[b][t].numel())
                n_host[t * B + b] = n_b
                if n_b < 2:
                    continue                                   # empty scene (0); a single object is refused by the library
                gs, gr, e2n = (i64(g) for g in graph_info[b][t])
                E = int(gs.numel())
                if gr.numel() != E or e2n.ndim != 2 or e2n.shape[0] != n_b:
                    raise ValueError(f"graph_info of scene {b}, step {t} does not match its present objects")
                e_host[t * B + b] = E
                deg[t * B + b] = int(e2n.shape[1])
                bounds.append((E, int(e2n.numel())))
                if uniform is not None:
                    u = f32(uniform[t][b]).reshape(-1, K)
                    if u.shape[0] != E:
                        raise ValueError(f"uniform of scene {b}, step {t} must be [E, K]")
                    live["u"].append(u)
                for k, v in (("ni", i64(node_inds[b][t])), ("gs", gs), ("gr", gr), ("e2n", e2n.reshape(-1))):
                    live[k].append(v)
            if not bounds:
                continue                                       # nobody anywhere at this step: null pointers, no draws
            if uniform is None:
                live["u"] = [torch.rand(sum(E for E, _ in bounds), K, device=dev)]
            step = {k: v[0] if len(v) == 1 else torch.cat(v) for k, v in live.items()}
            keep.append(step)
            for k in ptrs:
                ptrs[k][t] = step[k].data_ptr()
            # edge2node names edges of its own scene's graph: an id >= E would index past the scene's message rows
            if not step["e2n"].numel():
                continue
            if len(bounds) == 1:
                e2n_range.append((t, *torch.aminmax(step["e2n"]), bounds[0][0]))
            else:
                bound = torch.repeat_interleave(torch.tensor([E for E, _ in bounds], device=dev),
                                                torch.tensor([c for _, c in bounds], device=dev),
                                                output_size=step["e2n"].numel())
                e2n_range.append((t, step["e2n"].min(), (step["e2n"] - bound).max(), 0))
        if e2n_range:                                              # (one device round trip for all steps)
            got = torch.stack([v for _, lo, hi, _ in e2n_range for v in (lo, hi)]).cpu().tolist()
            for i, (t, _, _, limit) in enumerate(e2n_range):
                if got[2 * i] < 0 or got[2 * i + 1] >= limit:
                    raise ValueError(f"graph_info of step {t}: an edge2node entry names an edge its scene's graph does not have")
        cfg = self._step_config()
        preds = self._rollout_call(lib, cfg, B, Nmax, n_steps, inputs, x, m, burn, n_host, e_host, deg, ptrs)
        out = preds.transpose(0, 1).contiguous()
        if return_pack:
            return out, dict(cfg=cfg, n_objects_max=Nmax, n_steps=n_steps, inputs=x, masks=m, burn_in_masks=burn, n_present=n_host,
                             n_edges=e_host, in_degree=deg, ptrs=ptrs, keep=keep)
        return out

    @torch.no_grad()
    def predict_future_packed(self, inputs, masks, burn_in_masks, pack, uniform=None):
        """``predict_future`` of B scenes (1..256) on a ``ScenePack`` of the same inputs and masks: ONE ``*_rollout_batched``
        call on the pack's arrays.  No per-(scene, step) Python, no host lists and no edge2node range check (the library built
        them).  ``uniform``: None (one ``torch.rand`` for the call, step by step and scene by scene in the rows of one tensor)
        or ``uniform[t][b]`` ([E, K]) as ``predict_future`` takes it."""
        self._rollout_guard(inputs)
        lib = _lib.load()
        dev = inputs.device
        B, T, Nmax = int(inputs.size(0)), int(inputs.size(1)), int(inputs.size(2))
        n_steps, K = T - 1, self.num_edge_types
        cfg = self._step_config()
        if (pack.n_scenes, pack.n_objects_max) != (B, Nmax) or pack.n_frames < n_steps or n_steps < 1:
            raise ValueError("the pack was built for other scenes (scenes, object rows or frames differ)")
        if pack.k != cfg.knn_k:
            raise ValueError(f"the rollout needs a pack with k = {cfg.knn_k}")
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        x = f32(inputs).transpose(0, 1).contiguous()                                   # [T][B][Nmax][4]
        m = f32(masks)[:, :n_steps].transpose(0, 1).contiguous()                       # [n_steps][B][Nmax]
        burn = f32(burn_in_masks)[:, :n_steps].transpose(0, 1).contiguous()
        if m.shape[0] < n_steps or burn.shape[0] < n_steps:
            raise ValueError("masks / burn_in_masks must cover every step")
        v = pack.view
        steps = torch.arange(n_steps, dtype=torch.int64)
        e_step = torch.tensor(list(pack.n_edges), dtype=torch.int64).view(pack.n_frames, B)[:n_steps].sum(1)
        if uniform is None:
            u = torch.rand(int(e_step.sum()), K, device=dev)
        else:
            n_host = pack.n_present
            rows = [f32(uniform[t][b]).reshape(-1, K) for t in range(n_steps) for b in range(B) if n_host[t * B + b] >= 2]
            u = torch.cat(rows) if rows else torch.empty(0, K, device=dev)
            if u.shape[0] != int(e_step.sum()):
                raise ValueError("uniform[t][b] must be [E, K] of the scene's graph at that step")
        u_off = torch.cumsum(e_step, 0) - e_step
        arr = lambda vals: (C.c_void_p * n_steps)(*vals.tolist())
        ptrs = dict(ni=arr(v.node_inds + steps * (v.node_stride * 8)), gs=arr(v.graph_send + steps * (v.edge_stride * 8)),
                    gr=arr(v.graph_recv + steps * (v.edge_stride * 8)), e2n=arr(v.edge2node + steps * (v.edge_stride * 8)),
                    u=arr((u.data_ptr() if u.numel() else pack.buf.data_ptr()) + u_off * (K * 4)))
        preds = self._rollout_call(lib, cfg, B, Nmax, n_steps, inputs, x, m, burn, pack.n_present, pack.n_edges, pack.in_degree,
                                   ptrs)
        return preds.transpose(0, 1).contiguous()
