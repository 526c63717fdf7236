"""The scene engine's size arithmetic, held to what the library returned before the two variable-N models' host drivers were
merged (tests/golden/dyn_workspace_sizes.json, written by tools/dyn_workspace_sizes.py from that build): the six step / rollout
size functions of both models and the stage size functions, over 1..256 scenes with empty, two-object and full scenes, both
in_degree forms and 1 / 3 steps; and the refusing inputs of test_dyn_dnri.py, by status and by text.  Host only."""
import ctypes as C
import json
import os
import sys

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import dyn_workspace_sizes as WS                                          # noqa: E402
from test_dyn_dnri import _codes, _config                                # noqa: E402


def test_workspace_sizes_equal_the_recorded_ones():
    from aether_amd import _lib
    lib = _lib.load()
    want = json.load(open(os.path.join(GOLDEN, "dyn_workspace_sizes.json")))
    assert want["functions"] == list(WS.FUNCTIONS) and want["configs"] == [list(c) for c in WS.CONFIGS]
    cases = WS.cases()
    assert [w["case"] for w in want["cases"]] == [list(c) for c in cases]
    # the table covers what it says: every scene count and row count, empty / two-object / full scenes, an all-empty step
    assert {c[1] for c in cases} == {2, 5, 9, 20} and {c[2] for c in cases} == {1, 2, 6, 256}
    assert {c[3] for c in cases} == {"one", "knn"} and {c[4] for c in cases} == {1, 3} and any(c[5] for c in cases)
    assert {c[0] for c in cases} == set(range(len(WS.CONFIGS)))
    n = WS.counts(20, 6, 3, False)
    assert {0, 2, 20} <= set(n[0]) and not any(n[1])
    for case, w in zip(cases, want["cases"]):
        got = WS.measure(lib, case)
        for name, g, v in zip(WS.FUNCTIONS, got, w["sizes"]):
            assert g == v, (name, case)
        # an all-empty step needs the two alignment pads only; every batched size of a non-empty case is positive
        if any(WS.counts(*case[1:3], *case[4:])[0]):
            assert min(got[1], got[4]) > 512
        else:
            assert got[1] == got[4] == 512
        assert min(got[3], got[5]) > 0


def test_refusing_inputs_still_refuse_with_the_same_text():
    from aether_amd import _lib
    lib = _lib.load()
    cfg = _config()
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    i32 = lambda *v: (C.c_int * len(v))(*v)
    one_object = ("dyn_step_batched: a scene with one present object (the reference fails there as well, "
                  "aether_dynamicvars.py:843-851)")
    edges = ("dyn_step: n_edges must be n_present * min(knn_k, n_present - 1), the size of the encoder's own kNN graph")
    err = lambda: lib.aether_last_error().decode()
    for size in (lib.aether_dyn_dnri_step_batched_workspace_bytes, lib.aether_dyn_step_batched_workspace_bytes):
        assert size(C.byref(cfg), 2, 9, i64(7, 1), i64(42, 0), i32(6, 0)) == 0 and err() == one_object
        assert size(C.byref(cfg), 1, 9, i64(7), i64(41), i32(6)) == 0 and err() == edges
    for size in (lib.aether_dyn_dnri_rollout_batched_workspace_bytes, lib.aether_dyn_rollout_batched_workspace_bytes):
        assert size(C.byref(cfg), 1, 9, 2, i64(7, 1), i64(42, 0), i32(6, 0)) == 0 and err() == one_object
        assert size(C.byref(cfg), 1, 9, 2, i64(7, 7), i64(42, 40), i32(6, 6)) == 0 and err() == edges
    # the rollout entries return from their host checks (the device pointers are placeholders, never read)
    einval = _codes()["AETHER_EINVAL"]
    fake = C.c_void_p(4096)
    ptrs = (C.c_void_p * 2)(4096, 4096)
    tail = (ptrs, ptrs, ptrs, ptrs, ptrs, fake, fake, fake, fake, fake, 1 << 30, None)
    for head, roll in (((fake, fake), lib.aether_dyn_dnri_rollout_batched), ((fake, fake, fake), lib.aether_dyn_rollout_batched)):
        st = roll(*head, C.byref(cfg), 1, 9, 2, fake, fake, fake, i64(7, 1), i64(42, 0), i32(6, 0), *tail)
        assert st == einval and err() == one_object
        st = roll(*head, C.byref(cfg), 1, 9, 2, fake, fake, fake, i64(7, 7), i64(42, 40), i32(6, 6), *tail)
        assert st == einval and err() == edges
    # each entry's own refusals carry its own name
    null = (None,) * 5 + (fake,) * 5 + (1 << 30, None)
    st = lib.aether_dyn_dnri_rollout_batched(fake, fake, C.byref(cfg), 1, 9, 2, fake, fake, fake, i64(7, 7), i64(42, 42), i32(6, 6),
                                             *null)
    assert st == einval and err() == "dyn_dnri_rollout_batched: null pointer"
    st = lib.aether_dyn_rollout_batched(fake, fake, fake, C.byref(cfg), 1, 9, 0, fake, fake, fake, i64(7), i64(42), i32(6), *tail)
    assert st == einval and err() == "dyn_rollout_batched: n_steps must be positive"
    bad = _config(K=1, skip=1)                                # skip_first with one edge type: the dNRI entries' own check
    st = lib.aether_dyn_dnri_rollout_batched(fake, fake, C.byref(bad), 1, 9, 2, fake, fake, fake, i64(7, 7), i64(42, 42), i32(6, 6),
                                             *tail)
    assert st == einval and err() == "dyn_dnri_rollout_batched: skip_first needs two edge types"
    st = lib.aether_dyn_dnri_step_batched(None, fake, C.byref(cfg), 1, 9, i64(7), i64(42), i32(6), *(fake,) * 12, fake, 1 << 30, None)
    assert st == einval and err() == "dyn_dnri_step_batched: null pointer"
    st = lib.aether_dyn_step_batched(fake, fake, fake, C.byref(cfg), 1, 9, i64(7), i64(42), i32(6), fake, fake, *(None,) * 4, fake, fake,
                                     fake, None, fake, None, fake, 1 << 30, None)
    assert st == einval and err() == "dyn_step_batched: null graph / uniform pointer"
