"""Variable-N (inD) family: the per-frame graphs of a batch of scenes built on the device (``pack_scenes`` /
``aether_dyn_scene_pack``) against the host lists the reference's data set keeps, and ``predict_future_packed`` against
``predict_future`` on those lists.

3 scenes x 12 object rows x 7 frames: k = 1 (two objects); a frame nobody is in; an empty scene next to full ones; n = 11
with in_degree n - 1 = 10; n = 12 with in_degree 10 < n - 1; a scene count that is no power of two.  Random normal
positions: no distance ties."""
import pytest
import torch

from conftest import scale_rel_err
from aether_amd import _lib
from aether_amd.nn.dynamicvars.aether_dynamicvars import ScenePack, pack_scenes
from guarded_alloc import GuardedAlloc, POISON
from oracle import dynamicvars_oracle as DO
from test_gpu_dynamicvars import TOL, _scene_model, _scenes

pytestmark = pytest.mark.gpu

COUNTS = [[2, 2, 0, 5, 3, 12, 2], [3, 0, 0, 2, 5, 11, 4], [0, 12, 0, 7, 2, 0, 3]]
N, T, B = 12, 7, 3
_S = {}


def _setup():
    """Built once, never modified: the model, the host lists of ``_scenes``, the device inputs and their pack."""
    if _S:
        return _S
    model, sd, MP = _scene_model()
    model = model.cuda()
    K = MP["num_edge_types"]
    h = _scenes(COUNTS, N, 61, K)
    cu = lambda t: t.cuda()
    inputs, masks, burn = cu(h["inputs"]), cu(h["masks"]), cu(h["burn"])
    _S.update(model=model, sd=sd, MP=MP, K=K, host=h, inputs=inputs, masks=masks, burn=burn,
              node_inds=[[cu(n) for n in ni_b] for ni_b in h["node_inds"]],
              graph_info=[[tuple(cu(x) for x in gi) for gi in gi_b] for gi_b in h["graph_info"]],
              uniform=[[cu(u) for u in h["uniform"][t]] for t in range(T - 1)], pack=pack_scenes(inputs, masks))
    return _S


def test_pack_arrays_equal_the_host_lists():
    s = _setup()
    pack, h = s["pack"], s["host"]
    assert isinstance(pack, ScenePack) and (pack.n_scenes, pack.n_frames, pack.n_objects_max, pack.k) == (B, T, N, 10)
    node_inds, graph_info = pack.as_lists()
    for b in range(B):
        for t in range(T):
            assert torch.equal(node_inds[b][t].cpu(), h["node_inds"][b][t]), (b, t)
            for got, want, what in zip(graph_info[b][t], h["graph_info"][b][t], ("send", "recv", "edge2node")):
                assert got.shape == want.shape and torch.equal(got.cpu(), want), (b, t, what)
    # the arrays and counts the list path marshals for the library (first T - 1 frames) are the pack's
    _, listed = s["model"]._predict_future_rollout(s["inputs"], s["masks"], s["node_inds"], s["graph_info"], s["burn"],
                                                   s["uniform"], return_pack=True)
    n_steps = T - 1
    for name, mine in (("n_present", pack.n_present), ("n_edges", pack.n_edges), ("in_degree", pack.in_degree)):
        assert list(listed[name]) == list(mine)[:n_steps * B], name
    assert [int(x) for x in list(pack.n_present)[n_steps * B:]] == [c[T - 1] for c in COUNTS]
    ni, gs, gr, e2n = pack.arrays()
    n, e, _ = pack.counts()
    live = iter(listed["keep"])
    for t in range(n_steps):
        nt, et = int(n[t].sum()), int(e[t].sum())
        if nt == 0:
            assert listed["ptrs"]["ni"][t] is None
            continue
        step = next(live)
        for mine, key, cnt in ((ni, "ni", nt), (gs, "gs", et), (gr, "gr", et), (e2n, "e2n", et)):
            assert torch.equal(mine[t, :cnt], step[key]), (t, key)


def test_predict_future_packed_equals_the_list_path():
    s = _setup()
    model, pack, U = s["model"], s["pack"], s["uniform"]
    node_inds, graph_info = pack.as_lists()
    got = model.predict_future_packed(s["inputs"], s["masks"], s["burn"], pack, uniform=U)
    want = model.predict_future(s["inputs"], s["masks"], node_inds, graph_info, s["burn"], uniform=U)
    assert got.shape == (B, T - 1, N, 4) and torch.equal(got, want)
    assert float(got[:, 2].abs().max()) == 0.0 and float(got[2, 0].abs().max()) == 0.0       # nobody there: zeros
    # scene 0 alone
    one = pack_scenes(s["inputs"][:1], s["masks"][:1])
    ni1, gi1 = one.as_lists()
    u0 = [U[t][0] for t in range(T - 1)]
    got0 = model.predict_future_packed(s["inputs"][:1], s["masks"][:1], s["burn"][:1], one, uniform=[[u] for u in u0])
    want0 = model.predict_future(s["inputs"][:1], s["masks"][:1], ni1, gi1, s["burn"][:1], uniform=u0)
    assert torch.equal(got0, want0)
    h, MP = s["host"], s["MP"]
    oracle = DO.predict_future(s["sd"], h["inputs"][:1], h["masks"][:1], h["node_inds"][0], h["graph_info"][0], h["burn"][:1],
                               [h["uniform"][t][0] for t in range(T - 1)], MP["gumbel_temp"], MP["skip_first"],
                               MP["pos_representation"])
    err = scale_rel_err(got0.cpu(), oracle)
    print("packed, scene 0 alone vs oracle:", err)
    assert err <= 2 * TOL
    # uniform=None: ONE torch.rand for the call, rows step by step and scene by scene
    torch.cuda.manual_seed(5)
    free = model.predict_future_packed(s["inputs"], s["masks"], s["burn"], pack)
    torch.cuda.manual_seed(5)
    _, e, _ = pack.counts()
    draws = torch.rand(int(e[:T - 1].sum()), s["K"], device="cuda")
    sizes = [int(v) for v in e[:T - 1].reshape(-1)]
    parts = list(draws.split(sizes))
    hand = [[parts[t * B + b] for b in range(B)] for t in range(T - 1)]
    assert torch.equal(model.predict_future_packed(s["inputs"], s["masks"], s["burn"], pack, uniform=hand), free)


def test_a_single_present_object_is_refused_by_name():
    s = _setup()
    masks = s["masks"].clone()
    masks[1, 3] = 0
    masks[1, 3, 7] = 1
    with pytest.raises(_lib.AetherHipError) as info:
        pack_scenes(s["inputs"], masks)
    assert "scene 1" in str(info.value) and "step 3" in str(info.value), str(info.value)


def _unwritten_is_poison(pack, alloc):
    """Every byte of ``pack.buf`` outside the documented outputs still holds the poison; the outputs hold none."""
    ni, gs, gr, e2n = pack.arrays()
    n, e, _ = pack.counts()
    for t in range(pack.n_frames):
        nt, et = int(n[t].sum()), int(e[t].sum())
        assert bool((ni[t, nt:] == -1).all()) and bool((ni[t, :nt] >= 0).all()), t
        for arr in (gs, gr, e2n):
            assert bool((arr[t, et:] == -1).all()) and bool((arr[t, :et] >= 0).all()), t
    # between and behind the arrays: the alignment pads, and the words behind the three per-(frame, scene) int tables
    v, base, S = pack.view, pack.buf.data_ptr(), pack.n_frames * pack.n_scenes
    ends = [v.node_inds - base + pack.n_frames * v.node_stride * 8] + \
           [p - base + pack.n_frames * v.edge_stride * 8 for p in (v.graph_send, v.graph_recv)]
    starts = [v.graph_send - base, v.graph_recv - base, v.edge2node - base]
    for lo, hi in zip(ends, starts):
        assert bool((pack.buf[lo:hi] == POISON).all())
    tables = v.edge2node - base + pack.n_frames * v.edge_stride * 8
    tables = (tables + 255) // 256 * 256
    per = (S * 4 + 255) // 256 * 256
    assert tables + 3 * per == pack.buf.numel() == alloc.nbytes
    for i in range(3):
        assert bool((pack.buf[tables + i * per + S * 4:tables + (i + 1) * per] == POISON).all()), i


def test_pack_and_scratch_stay_inside_their_buffers_and_runs_repeat():
    """Through guarded, poisoned allocations: ``pack`` and ``scratch`` are exactly their ``_bytes``, the guard bands stay
    intact, nothing but the documented outputs is written, and two runs give equal bytes (whole buffer, poison included)."""
    s = _setup()
    lib = _lib.load()
    with GuardedAlloc() as ga:
        x, m = ga.guarded_copy(s["inputs"]), ga.guarded_copy(s["masks"])
        first = pack_scenes(x, m)
        second = pack_scenes(x, m)
        a, b = ga.holds(first.buf), ga.holds(second.buf)
        assert a is not None and b is not None and a.nbytes == lib.aether_dyn_scene_pack_bytes(B, N, T, 10)
        ga.check()
        _unwritten_is_poison(first, a)
        assert torch.equal(first.buf, second.buf)
        assert list(first.n_present) == list(second.n_present) and list(first.n_edges) == list(second.n_edges)
        # the metric's scratch, at exactly its size
        S = T - 1
        need = lib.aether_dyn_eval_scratch_bytes(B, N, S)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert ga.holds(scratch).nbytes == need
        preds = ga.guarded_copy(torch.randn(B, S, N, 4, device="cuda"))
        truth = ga.guarded_copy(s["inputs"][:, 1:])
        burn = ga.guarded_copy(s["burn"])
        so = ga.guarded_copy(torch.tensor([1.5, 1.5, 2.0, 2.0, 0.0, 0.0, 0.5, 0.5], device="cuda"))
        acc = ga.guarded_copy(torch.zeros(4 * S, dtype=torch.float64, device="cuda"))
        stats = ga.guarded_copy(torch.zeros(2, dtype=torch.int64, device="cuda"))
        st = lib.aether_dyn_eval_accumulate(preds.data_ptr(), truth.data_ptr(), 4, m.data_ptr(), burn.data_ptr(), so.data_ptr(),
                                            so.data_ptr() + 16, None, 0, B, N, S, acc.data_ptr(), acc.data_ptr() + 3 * S * 8,
                                            stats.data_ptr(), scratch.data_ptr(), need,
                                            torch.cuda.current_stream().cuda_stream)
        assert st == 0, lib.aether_last_error()
        ga.check()
        rows, flags = B * N * 4 * S * 8, B * N * 2 * 4
        rows_end = (rows + 255) // 256 * 256
        assert bool((scratch[rows:rows_end] == POISON).all()) and bool((scratch[rows_end + flags:] == POISON).all())
        assert bool(torch.isfinite(acc).all()) and int(stats[1]) > 0
