"""What tests/test_gpu_clof_shapes.py and tests/test_gpu_egnn_aether_shapes.py share: one description per model family
(how to build the drop-in, call it and restate it in fp64), the named input sets, and the checks themselves.

Test helper, not a test module.  The bars are the project's: forward 1e-5, parameter gradients 5e-5, max|a - b| / max|b|.

Every input set was first run through the restatement alone, on the CPU, in fp32 and in fp64 (`conditioning`, printed by
``python tests/gnn_shape_checks.py``); the worst figure of each set is in the docstring of the test that uses it.  An
input on which fp32 arithmetic by itself leaves the bar would say nothing about a kernel.
"""
from __future__ import annotations

import torch

import clof_restatement as CR
import egnn_restatement as ER
import graph_cases as GC
import test_clof as TC
import test_egnn_aether as TE

FWD_TOL, GRAD_TOL = 1e-5, 5e-5
DEV = "cuda"


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


class Clof:
    models = ("clof", "clof_vel", "clof_vel_gbf")

    @staticmethod
    def cfg(model, H, L, seed, N, in_nf=1, norm_diff=True, tanh=False, recurrent=True, coords_weight=1.0):
        return dict(model=model, H=H, L=L, seed=seed, N=N, in_nf=in_nf, norm_diff=norm_diff, tanh=tanh,
                    recurrent=recurrent, coords_weight=coords_weight, coord_scale=1.0)

    build = staticmethod(TC.build)

    @staticmethod
    def args(gi, cfg):
        return (gi["h"], gi["x"], gi["edges"], gi["vel"], gi["edge_attr"]), dict(n_nodes=cfg["N"])

    @staticmethod
    def step_args(gi, cfg):
        return [gi["h"], gi["x"], gi["edges"], gi["vel"], gi["edge_attr"], None, cfg["N"]]

    @staticmethod
    def restate(sd, inp, cfg):
        """((out, hs, xs), {key: gradient, None where the reference leaves .grad None}) in sd's dtype."""
        v = CR.VARIANTS[cfg["model"]]
        a = (inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"])
        fw = CR.forward(sd, v, *a, cfg["L"], cfg["N"], **TC.kwargs(cfg))
        g, _ = CR.grads(sd, v, *a, inp["target"], cfg["L"], cfg["N"], **TC.kwargs(cfg))
        return fw, g

    @staticmethod
    def dead(m):
        keys = [k for k, _ in m.named_parameters()]
        return {keys[i] for i in m._dead()}

    @staticmethod
    def edge_side(k):
        """Parameters that only edges reach: with no edge their gradient is zero."""
        return k.startswith(("fuse_edge.", "gbf.", "embedding_edge.")) or ".edge_mlp." in k or ".coord_mlp." in k


class Egnn:
    models = ("egnn_aether",)

    @staticmethod
    def cfg(model, H, L, seed, N, in_nf=1, norm_diff=False, tanh=False, **unused):
        return dict(model=model, H=H, L=L, seed=seed, N=N, in_nf=in_nf, norm_diff=norm_diff, tanh=tanh, phi_scale=1.0)

    build = staticmethod(TE.build)

    @staticmethod
    def args(gi, cfg):
        return (gi["h"], gi["x"], gi["edges"], gi["vel"], gi["edge_attr"], gi["charges"]), {}

    @staticmethod
    def step_args(gi, cfg):
        return [gi["h"], gi["x"], gi["edges"], gi["vel"], gi["edge_attr"], gi["charges"]]

    @staticmethod
    def restate(sd, inp, cfg):
        """The last layer's node_mlp does not reach the output: zeros, as the kernels write them."""
        a = (inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"])
        fw = ER.forward(sd, *a, cfg["L"], cfg["norm_diff"], cfg["tanh"])
        g, _ = ER.grads(sd, *a, inp["target"], cfg["L"], cfg["norm_diff"], cfg["tanh"])
        return fw, g

    @staticmethod
    def dead(m):
        return set()

    @staticmethod
    def edge_side(k):
        return ".edge_mlp." in k or ".coord_mlp." in k


# ---- the named input sets ----------------------------------------------------------------------------------------------
def cast(inp, dtype):
    return {k: (v if k == "edges" else v.to(dtype)) for k, v in inp.items()}


def dev(inp):
    return {k: ([t.to(DEV) for t in v] if k == "edges" else v.to(DEV, torch.float32)) for k, v in inp.items()}


def deep128(K, model, seed=41):
    """B 16, N 20 (6080 edges), hidden 128, 4 layers, the family's README options."""
    return K.cfg(model, 128, 4, seed, 20, norm_diff=True), ER.runner_batch(16, 20, seed + 1, dtype=torch.float64)


def multigraph(K, model, H, seed):
    """3 graphs of 7 nodes (21 nodes: a partial node block), 3 layers; odd seeds carry a self loop and run the layers
    without norm_diff (sqrt at 0 has a NaN gradient in the reference)."""
    loop = seed % 2 == 1
    return K.cfg(model, H, 3, 200 + seed, 7, norm_diff=not loop), GC.random_multigraph(3, 7, 300 + seed, self_loop=loop)


def hub(K, model, H, last):
    """301 nodes, one of degree 300 at the first or the last node id, nodes of degree 1, 2, 3 and 5; 2 layers."""
    inp, special = GC.hub_graph(301, 300 if last else 0, 52 + int(last))
    return K.cfg(model, H, 2, 51, 301, norm_diff=True), inp


TILE_E = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)


def tile(K, model, E, H=64):
    """One complete graph of 20 nodes thinned to exactly E edges, 2 layers."""
    return K.cfg(model, H, 2, 61, 20, norm_diff=True), GC.thinned_complete(1, 20, E, 62)


def no_edges(K, model, H):
    """B 3, N 5 without a single edge, 3 layers."""
    return K.cfg(model, H, 3, 71, 5, norm_diff=True), GC.without_edges(ER.runner_batch(3, 5, 72, dtype=torch.float64))


OPTIONS = {"norec": dict(recurrent=False), "cw": dict(coords_weight=0.5), "tanh": dict(tanh=True),
           "nonorm": dict(norm_diff=False), "norm": dict(norm_diff=True)}


def options(K, model, names, B=2, N=5, H=64):
    """The named constructor options at 4 layers, at the fixtures' shape or B 16, N 20."""
    kw = dict(norm_diff=K is Clof)
    for n in names:
        kw.update(OPTIONS[n])
    return K.cfg(model, H, 4, 81, N, **kw), ER.runner_batch(B, N, 82, dtype=torch.float64)


def wide_h(K, model, in_nf, H=64):
    """B 4, N 5 with in_node_nf columns of node features, 2 layers."""
    cfg = K.cfg(model, H, 2, 91, 5, in_nf=in_nf, norm_diff=True)
    return cfg, GC.with_wide_h(ER.runner_batch(4, 5, 92, dtype=torch.float64), in_nf)


def plain(K, model, B, seed, H=64, L=2, N=5):
    return K.cfg(model, H, L, 101, N, norm_diff=True), ER.runner_batch(B, N, seed, dtype=torch.float64)


# ---- the checks --------------------------------------------------------------------------------------------------------
def state64(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def hip_step(K, m, gi, cfg, zero=True):
    """(out, {key: .grad or None}) of one forward / backward of MSELoss(out, target)."""
    if zero:
        m.zero_grad(set_to_none=True)
    a, kw = K.args(gi, cfg)
    out = m(*a, **kw)
    torch.nn.functional.mse_loss(out, gi["target"]).backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in m.named_parameters()}


def snapshot(g):
    return {k: (None if v is None else v.detach().clone()) for k, v in g.items()}


def same_bits(g1, g2, keys=None):
    for k in (keys if keys is not None else g1):
        assert (g1[k] is None) == (g2[k] is None), k
        assert g1[k] is None or torch.equal(g1[k], g2[k]), k


def against_restatement(K, m, inp, cfg, layers=False, show=None):
    """Forward (every layer's h and x with `layers`) and every parameter gradient of the HIP path against the fp64
    restatement at the bars; the parameters that do not reach the output keep .grad None.  Returns (out, gradients)."""
    gi = dev(inp)
    (o64, hs64, xs64), g64 = K.restate(state64(m), cast(inp, torch.float64), cfg)
    worst = [0.0, 0.0]
    if layers:
        a, kw = K.args(gi, cfg)
        _, hs, xs = m.forward_layers(*a, **kw)
        for l in range(cfg["L"] + 1):
            eh, ex = rel(hs[l].cpu(), hs64[l]), rel(xs[l].cpu(), xs64[l])
            worst[0] = max(worst[0], eh, ex)
            assert eh < FWD_TOL and ex < FWD_TOL, (l, eh, ex)
    out, g = hip_step(K, m, gi, cfg)
    e = rel(out.cpu(), o64)
    worst[0] = max(worst[0], e)
    assert torch.isfinite(out).all() and e < FWD_TOL, e
    dead = K.dead(m)
    for k, gv in g.items():
        if k in dead:
            assert gv is None and g64[k] is None, k
            continue
        assert gv is not None and g64[k] is not None, k
        e = rel(gv.cpu(), g64[k])
        worst[1] = max(worst[1], e)
        assert torch.isfinite(gv).all() and e < GRAD_TOL, (k, e)
    if show is not None:
        print(f"{show}: forward {worst[0]:.2e}, gradients {worst[1]:.2e}")
    return out, snapshot(g)


def fresh_step(K, cfg, inp):
    """(out, gradients) of a module built for this one call."""
    out, g = hip_step(K, K.build(cfg, DEV), dev(inp), cfg)
    return out, snapshot(g)


def check_tile_edges(K, model, E, H=64):
    """E edges, then E - 37 on the same module: each at the bars, and the second bit for bit what a fresh module gives
    (rows that the larger call left in the reused workspace are not read)."""
    cfg, big = tile(K, model, E, H)
    _, small = tile(K, model, E - 37, H)
    m = K.build(cfg, DEV)
    against_restatement(K, m, big, cfg)
    out, g = against_restatement(K, m, small, cfg)
    out0, g0 = fresh_step(K, cfg, small)
    assert torch.equal(out, out0)
    same_bits(g, g0)
    with torch.no_grad():                                   # the inference workspace: larger call first, too
        a, kw = K.args(dev(big), cfg)
        m(*a, **kw)
        a, kw = K.args(dev(small), cfg)
        assert torch.equal(m(*a, **kw), out0)


def check_no_edges(K, model, H):
    cfg, inp = no_edges(K, model, H)
    m = K.build(cfg, DEV)
    out, g = against_restatement(K, m, inp, cfg, layers=True)
    _, g64 = K.restate(state64(m), cast(inp, torch.float64), cfg)
    n_zero = 0
    for k, gv in g.items():
        if gv is None:
            continue
        assert torch.equal(gv.cpu() == 0, g64[k] == 0), k             # zero exactly where the reference's is
        if K.edge_side(k):
            assert int(torch.count_nonzero(gv)) == 0 and int(torch.count_nonzero(g64[k])) == 0, k
            n_zero += 1
    assert n_zero >= 7 * cfg["L"]
    return out


def check_accumulation(K, model, as_view, H=64):
    cfg, a = plain(K, model, 2, 111, H)
    _, b = plain(K, model, 4, 113, H)
    ga_, gb_ = dev(a), dev(b)
    _, g1 = fresh_step(K, cfg, a)
    _, g2 = fresh_step(K, cfg, b)
    live = [k for k in g1 if g1[k] is not None]
    m = K.build(cfg, DEV)
    m.grad_as_view = as_view
    hip_step(K, m, ga_, cfg)
    _, g = hip_step(K, m, gb_, cfg, zero=False)                        # a second backward without zero_grad
    for k in live:
        assert torch.equal(g[k], g1[k] + g2[k]), k
    _, g = hip_step(K, m, ga_, cfg, zero=False)                        # and a third
    for k in live:
        assert torch.equal(g[k], (g1[k] + g2[k]) + g1[k]), k
    m.zero_grad(set_to_none=False)
    _, g = hip_step(K, m, gb_, cfg, zero=False)
    same_bits(snapshot(g), g2)
    # some .grad replaced by foreign tensors before the next backward: autograd adds into them
    params = dict(m.named_parameters())
    for i, k in enumerate(live):
        if i % 2 == 0:
            params[k].grad = torch.full_like(params[k], 0.5)
    _, g = hip_step(K, m, ga_, cfg, zero=False)
    for i, k in enumerate(live):
        want = (torch.full_like(g1[k], 0.5) if i % 2 == 0 else g2[k]) + g1[k]
        assert torch.equal(g[k], want), k
    for k in g1:
        if g1[k] is None:
            assert g[k] is None, k


def check_frozen(K, model, which, H=64):
    cfg, inp = plain(K, model, 4, 113, H, L=3)
    _, g0 = fresh_step(K, cfg, inp)
    m = K.build(cfg, DEV)
    prefix = {"layer": "gcl_1.", "embedding": "embedding"}[which]
    frozen = [k for k, p in m.named_parameters() if k.startswith(prefix)]
    assert frozen
    for k, p in m.named_parameters():
        if k in frozen:
            p.requires_grad_(False)
    for _ in range(2):
        _, g = hip_step(K, m, dev(inp), cfg)
        for k in g:
            if k in frozen:
                assert g[k] is None, k
        same_bits(g, g0, [k for k in g if k not in frozen])


def check_two_forwards(K, model, first, H=64):
    cfg, a = plain(K, model, 2, 111, H)
    _, b = plain(K, model, 4, 113, H)
    singles = {"a": fresh_step(K, cfg, a), "b": fresh_step(K, cfg, b)}
    m = K.build(cfg, DEV)
    m.zero_grad(set_to_none=True)
    outs, losses = {}, {}
    for name, inp in (("a", a), ("b", b)):
        gi = dev(inp)
        args, kw = K.args(gi, cfg)
        outs[name] = m(*args, **kw)
        losses[name] = torch.nn.functional.mse_loss(outs[name], gi["target"])
    for name in (first, "b" if first == "a" else "a"):
        m.zero_grad(set_to_none=True)
        losses[name].backward()
        torch.cuda.synchronize()
        assert torch.equal(outs[name].detach(), singles[name][0]), name
        same_bits({k: p.grad for k, p in m.named_parameters()}, singles[name][1])


def check_alternating_sizes(K, model, H=64):
    cfg, _ = plain(K, model, 2, 0, H)
    m = K.build(cfg, DEV)
    for step in range(10):
        B = 2 if step % 2 == 0 else 32
        _, inp = plain(K, model, B, 500 + step, H)
        gi = dev(inp)                                                   # fresh edge tensors every call
        out, g = hip_step(K, m, gi, cfg)
        out0, g0 = fresh_step(K, cfg, inp)
        assert torch.equal(out, out0), step
        same_bits(g, g0)
        assert len(m._graphs._d) <= m._graphs.max_entries
    assert len(m._graphs._d) == m._graphs.max_entries                   # entries were evicted on the way
    against_restatement(K, m, inp, cfg)


def check_checkpoint_load(K, model, H=64):
    cfg, inp = plain(K, model, 4, 113, H)
    m = K.build(cfg, DEV)
    against_restatement(K, m, inp, cfg)
    other = K.build(dict(cfg, seed=cfg["seed"] + 1), DEV)
    _, g_other = fresh_step(K, dict(cfg, seed=cfg["seed"] + 1), inp)
    before = m.state_dict()["gcl_0.edge_mlp.0.weight"].clone()
    m.load_state_dict({k: v.cpu() for k, v in other.state_dict().items()})
    assert not torch.equal(m.state_dict()["gcl_0.edge_mlp.0.weight"], before)
    out, g = against_restatement(K, m, inp, cfg)                        # the restatement reads m's own state_dict
    same_bits(g, g_other)
    m.to("cpu")
    m.to(DEV)
    out2, g2 = against_restatement(K, m, inp, cfg)
    assert torch.equal(out, out2)
    same_bits(g, g2)


def conditioning(K, cfg, inp):
    """(forward, gradient) distance of the fp32 restatement from the fp64 one, at the tests' metric, on the CPU."""
    sd = K.build(cfg).state_dict()
    (o32, hs32, _), g32 = K.restate({k: v.float() for k, v in sd.items()}, cast(inp, torch.float32), cfg)
    (o64, hs64, _), g64 = K.restate({k: v.double() for k, v in sd.items()}, cast(inp, torch.float64), cfg)
    fwd = max([rel(o32, o64)] + [rel(a, b) for a, b in zip(hs32, hs64)])
    grad = max(rel(g32[k], g64[k]) for k in g64 if g64[k] is not None)
    return fwd, grad


def _table():
    rows = []
    for K in (Clof, Egnn):
        for model in K.models:
            sets = {"deep128": [deep128(K, model)],
                    "multigraph": [multigraph(K, model, H, s) for H in (64, 128) for s in (0, 1, 2, 3)],
                    "hub": [hub(K, model, H, last) for H in (64, 128) for last in (False, True)],
                    "tile": [tile(K, model, E) for E in TILE_E + tuple(e - 37 for e in TILE_E)] + [tile(K, model, 129, 128)],
                    "no_edges": [no_edges(K, model, H) for H in (64, 128)],
                    "options": [options(K, model, [n]) for n in (("norec", "cw", "tanh", "nonorm") if K is Clof else
                                                                  ("tanh", "norm"))] +
                               [options(K, model, ("norec", "cw", "tanh", "nonorm") if K is Clof else ("tanh", "norm"),
                                        16, 20, H) for H in (64, 128)],
                    "wide_h": [wide_h(K, model, n, H) for n, H in ((3, 64), (5, 128))],
                    "plain": [plain(K, model, B, s) for B, s in ((2, 111), (32, 112), (4, 113))] +
                             [plain(K, model, 8, 121, 128, 4, 20)]}
            for name, cases in sets.items():
                c = [conditioning(K, *case) for case in cases]
                rows.append((model, name, max(f for f, _ in c), max(g for _, g in c)))
                print("%-13s %-11s forward %.1e  gradients %.1e" % rows[-1], flush=True)
    return rows


if __name__ == "__main__":
    torch.set_num_threads(8)
    _table()
