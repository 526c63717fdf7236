"""Host side of the variable-N prediction path, shared by the models of the family (``AetherDynamicVars``,
``DNRIDynamicVars``): one step of one scene as ONE library call, ``predict_future`` of B scenes as ONE library call (from
per-(scene, step) lists or from a ``ScenePack``), the staged loop, the dispatch between them, ``save`` / ``load`` and the guards.
The model supplies its configuration (``_step_config``), its entries with their parameter structs (``_step_entries``,
``_rollout_entries``) and one staged step (``_staged_step``); everything else -- time-major tensors, host size arrays, per-step
pointer tables, the edge2node range check, the workspace, the initial states -- is the same for every model on the scene engine.
"""
from __future__ import annotations

import ctypes as C
import functools

import torch

from ... import _lib
from ._scene import cached_workspace, f32, i64


def time_major(inputs, masks, burn_in_masks, n_steps):
    """-> x [T][B][Nmax][4], masks / burn_in_masks [n_steps][B][Nmax] as the rollout entries take them (views of the caller's
    tensors when B = 1: a dimension of size one has no stride to speak of)."""
    dev = inputs.device
    x = f32(inputs, dev).transpose(0, 1).contiguous()
    m = f32(masks, dev)[:, :n_steps].transpose(0, 1).contiguous()
    burn = f32(burn_in_masks, dev)[:, :n_steps].transpose(0, 1).contiguous()
    if m.shape[0] < n_steps or burn.shape[0] < n_steps:
        raise ValueError("masks / burn_in_masks must cover every step")
    return x, m, burn


class SceneRolloutMixin:
    """What a model supplies:

    ``_step_config() -> _DynStepConfig``.
    ``_rollout_entries(lib) -> (workspace_bytes_fn, rollout_fn, name, head)``: the model's ``*_rollout_batched_workspace_bytes``
    and ``*_rollout_batched`` entries, the latter's name for error messages, and the ``C.byref`` parameter structs it takes in
    front of the configuration.
    ``_step_entries(lib) -> (workspace_bytes_fn, step_fn, name)``: the same for one step of one scene;
    ``workspace_bytes_fn(cfg, Nmax, n, E, in_degree)`` and ``step_fn(cfg, Nmax, n, E, in_degree, state, mask, node_inds, send,
    recv, edge2node, prior_h, prior_c, decoder_hidden, uniform, prediction, edge_types, workspace, workspace_bytes, stream)``
    wrap the model's entry (the parameter structs are built inside ``step_fn``, behind the allocations).
    ``_staged_step(state, present, node_inds_t, graph_info_t, prior_state, dec_state, uniform_t, **kw) -> (prediction,
    prior_state, dec_state)``: one step of one scene through the staged calls.
    ``_batched_staged_step``: the same for B scenes (lists per scene), or None: B scenes always take the one-call rollout."""

    _TRAINING_REFUSAL = "the prior step uses BatchNorm running statistics: call .eval() first"
    _STEP_WS_CAPTURE_CHECK = None              # the refusal to allocate ``_step_ws`` under stream capture, where steps are captured
    _batched_staged_step = None

    def _in_training(self):
        return self.encoder.training

    def _guard(self, inputs):
        if not inputs.is_cuda:
            raise _lib.AetherHipError(f"aether_amd {type(self).__name__} runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        if self._in_training():
            raise _lib.AetherHipError(self._TRAINING_REFUSAL)

    def save(self, path):
        torch.save(self.state_dict(), path)                       # as the reference's save / load

    def load(self, path):
        self.load_state_dict(torch.load(path))

    @torch.no_grad()
    def _step_one_call(self, state, present, node_inds_t, gsend, grecv, e2n, prior_h, prior_c, dec_state, uniform_t,
                       pass_node_inds=True, return_edge_types=False):
        """One step of one scene as ONE library call (``_step_entries``): the same stage kernels as the staged calls, the index
        work between them in small kernels of the library instead of ~60 torch launches; bit-identical to the staged path.
        state [1, Nmax, 4], present [1, Nmax], prior_h / prior_c [1, Nmax (Nmax - 1), R], dec_state [1, Nmax, hd].
        ``pass_node_inds=False``: the library takes the mask's non-zero rows (what the data set's node_inds are)."""
        self._guard(state)
        lib = _lib.load()
        dev = state.device
        Nmax, n, E = int(state.shape[1]), int(node_inds_t.numel()), int(gsend.numel())
        if grecv.numel() != E or e2n.ndim != 2 or e2n.shape[0] != n or uniform_t.numel() != E * self.num_edge_types:
            raise ValueError("graph_info / uniform do not match the present objects")
        state, present, uniform_t = f32(state, dev), f32(present, dev).reshape(-1), f32(uniform_t, dev)
        ni, gs, gr, e2n = i64(node_inds_t, dev), i64(gsend, dev), i64(grecv, dev), i64(e2n, dev)
        new_h, new_c, new_dec = f32(prior_h, dev).clone(), f32(prior_c, dev).clone(), f32(dec_state, dev).clone()
        cfg = self._step_config()
        ws_bytes, step, name = self._step_entries(lib)
        sizes = (C.byref(cfg), Nmax, n, E, int(e2n.shape[1]) if n else 0)
        need = ws_bytes(*sizes)
        if need == 0:
            raise _lib.AetherHipError(f"{name}_workspace_bytes: " + lib.aether_last_error().decode())
        ws = cached_workspace(self, "_step_ws", need, dev, capture_check=self._STEP_WS_CAPTURE_CHECK)
        pred = torch.empty(1, Nmax, 4, dtype=torch.float32, device=dev)
        edge_types = torch.empty(E, self.num_edge_types, dtype=torch.float32, device=dev) if return_edge_types else None
        st = step(*sizes, state.data_ptr(), present.data_ptr(), ni.data_ptr() if pass_node_inds else None, gs.data_ptr(),
                  gr.data_ptr(), e2n.data_ptr(), new_h.data_ptr(), new_c.data_ptr(), new_dec.data_ptr(), uniform_t.data_ptr(),
                  pred.data_ptr(), edge_types.data_ptr() if edge_types is not None else None, ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, name)
        if return_edge_types:
            return pred, new_h, new_c, new_dec, edge_types
        return pred, new_h, new_c, new_dec

    def _staged_loop(self, inputs, masks, burn_in_masks, uniform, step, graph_at):
        """The reference's prediction loop around a staged step (``_staged_step`` / ``_batched_staged_step``), with
        ``graph_at(t) -> (node_inds, graph_info)`` of step t: observed objects are fed their ground truth, the others the
        model's own last prediction."""
        prior_state = self.encoder.get_initial_hidden(inputs)
        dec_state = self.decoder.get_initial_hidden(inputs)
        last = inputs[:, 0]
        preds = []
        for t in range(inputs.size(1) - 1):
            observed = burn_in_masks[:, t].unsqueeze(-1).type(inputs.dtype)
            state = observed * inputs[:, t] + (1 - observed) * last
            last, prior_state, dec_state = step(state, masks[:, t], *graph_at(t), prior_state, dec_state,
                                                None if uniform is None else uniform[t])
            preds.append(last)
        return torch.stack(preds, dim=1)

    def _predict_future(self, inputs, masks, node_inds, graph_info, burn_in_masks, uniform, **step_kw):
        """``predict_future`` of every model: B > 1 scenes go to ``predict_future_batched``; one scene is ONE library call
        (``_predict_future_rollout``) or, with ``one_call_step = False``, the staged loop over ``_staged_step``."""
        self._guard(inputs)
        if inputs.size(0) > 1:
            return self.predict_future_batched(inputs, masks, node_inds, graph_info, burn_in_masks, uniform)
        if self.one_call_step and inputs.size(1) > 1:
            return self._predict_future_rollout(inputs, masks, node_inds, graph_info, burn_in_masks,
                                                None if uniform is None else [[u] for u in uniform])
        return self._staged_loop(inputs, masks, burn_in_masks, uniform, functools.partial(self._staged_step, **step_kw),
                                 lambda t: (node_inds[0][t], graph_info[0][t]))

    @torch.no_grad()
    def predict_future_batched(self, inputs, masks, node_inds, graph_info, burn_in_masks, uniform=None):
        """``predict_future`` for B scenes (1..256) at once -- the reference raises on batch > 1: per time step ONE batched step
        over the present objects of ALL scenes, the whole loop ONE library call (``*_rollout_batched``).  A model with a batched
        staged step (``AetherDynamicVars``) takes it, step by step, with ``one_call_step = False`` or more than 256 scenes."""
        self._guard(inputs)
        B = inputs.size(0)
        fits = inputs.size(1) > 1 and B <= 256
        if fits and (self.one_call_step or self._batched_staged_step is None):
            return self._predict_future_rollout(inputs, masks, node_inds, graph_info, burn_in_masks, uniform)
        if self._batched_staged_step is None:
            raise ValueError("predict_future_batched takes 1..256 scenes of at least two frames")
        return self._staged_loop(inputs, masks, burn_in_masks, uniform, self._batched_staged_step,
                                 lambda t: ([node_inds[b][t] for b in range(B)], [graph_info[b][t] for b in range(B)]))

    def _rollout_call(self, lib, cfg, B, Nmax, n_steps, inputs, x, m, burn, n_host, e_host, deg, ptrs):
        """Workspace, initial states and the one library call -> predictions [n_steps][B][Nmax][4] (time-major)."""
        dev = inputs.device
        ws_bytes, rollout, name, head = self._rollout_entries(lib)
        need = ws_bytes(C.byref(cfg), B, Nmax, n_steps, n_host, e_host, deg)
        if need == 0:
            raise _lib.AetherHipError(f"{name}_workspace_bytes failed: " + lib.aether_last_error().decode())
        ws = cached_workspace(self, "_step_ws", need, dev)
        prior_h, prior_c = (f32(s, dev)[0].clone() for s in self.encoder.get_initial_hidden(inputs))
        dec = f32(self.decoder.get_initial_hidden(inputs), dev).clone()                       # [B][Nmax][hd]
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
        self._guard(inputs)
        lib = _lib.load()
        dev = inputs.device
        B, T, Nmax = int(inputs.size(0)), int(inputs.size(1)), int(inputs.size(2))
        n_steps, K = T - 1, self.num_edge_types
        x, m, burn = time_major(inputs, masks, burn_in_masks, n_steps)
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
                gs, gr, e2n = (i64(g, dev) for g in graph_info[b][t])
                E = int(gs.numel())
                if gr.numel() != E or e2n.ndim != 2 or e2n.shape[0] != n_b:
                    raise ValueError(f"graph_info of scene {b}, step {t} does not match its present objects")
                e_host[t * B + b] = E
                deg[t * B + b] = int(e2n.shape[1])
                bounds.append((E, int(e2n.numel())))
                if uniform is not None:
                    u = f32(uniform[t][b], dev).reshape(-1, K)
                    if u.shape[0] != E:
                        raise ValueError(f"uniform of scene {b}, step {t} must be [E, K]")
                    live["u"].append(u)
                for k, v in (("ni", i64(node_inds[b][t], dev)), ("gs", gs), ("gr", gr), ("e2n", e2n.reshape(-1))):
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
        self._guard(inputs)
        lib = _lib.load()
        dev = inputs.device
        B, T, Nmax = int(inputs.size(0)), int(inputs.size(1)), int(inputs.size(2))
        n_steps, K = T - 1, self.num_edge_types
        cfg = self._step_config()
        if (pack.n_scenes, pack.n_objects_max) != (B, Nmax) or pack.n_frames < n_steps or n_steps < 1:
            raise ValueError("the pack was built for other scenes (scenes, object rows or frames differ)")
        if pack.k != cfg.knn_k:
            raise ValueError(f"the rollout needs a pack with k = {cfg.knn_k}")
        x, m, burn = time_major(inputs, masks, burn_in_masks, n_steps)
        v = pack.view
        steps = torch.arange(n_steps, dtype=torch.int64)
        e_step = torch.tensor(list(pack.n_edges), dtype=torch.int64).view(pack.n_frames, B)[:n_steps].sum(1)
        if uniform is None:
            u = torch.rand(int(e_step.sum()), K, device=dev)
        else:
            n_host = pack.n_present
            rows = [f32(uniform[t][b], dev).reshape(-1, K) for t in range(n_steps) for b in range(B) if n_host[t * B + b] >= 2]
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
