"""The job-table launches of the NRI host chain, held to what the library issued before the chains of the seq2seq and the
variable-N engines were written once (csrc/host_nri_chain.inc): tests/golden/nri_chain_launch_log.json, written by
tools/nri_chain_launch_log.py from that build on the MI355X.  Every call of the table -- the seq2seq dNRI (both decoders) and
Aether at 60 edge rows: one step, the step on given logits, encoder_features, a rollout of one burn-in and two predicted
steps; the same three models at 2,280 edge rows, where the LSTM job takes the split GEMM with the cell in its epilogue; the
variable-N dNRI's staged prior and decoder steps, one-call step and two-step rollout on the N3 and N2 fixture scenes -- must
issue the same s2s_launch_jobs launches, record for record and in order, and none beyond the log's length.

The log sees job tables only.  The kernels launched outside them (pair, gate, aggregate, LSTM cell, output, and the s2s_linear
launches of the two staged Aether prior steps) are held by the parity tests of the models (test_gpu_s2s_dnri.py,
test_gpu_dyn_dnri.py, test_gpu_seq2seq.py, test_gpu_dynamicvars.py) and by the byte comparison of HISTORY R29."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import nri_chain_launch_log as NL                                         # noqa: E402

pytestmark = pytest.mark.gpu


def _golden():
    return json.load(open(os.path.join(GOLDEN, "nri_chain_launch_log.json")))


def test_the_fixture_covers_the_table():
    want = _golden()
    assert want["fields"] == list(NL.FIELDS)
    assert [w["case"] for w in want["cases"]] == [list(c) for c in NL.cases()]
    by = {tuple(w["case"]): w for w in want["cases"]}
    kind, k2, images = NL.FIELDS.index("kind"), NL.FIELDS.index("K2"), NL.FIELDS.index("images")
    # what the cases are there for: at 60 edge rows everything is on the fp32 job kernel, at 2,280 the LSTM table (the one
    # with a second K segment) is on a split GEMM; the stateless decoder's burn-in step is the prior alone
    for w in want["cases"]:
        assert 0 < w["logged"] == len(w["log"])
        if w["case"][2] != "e2280":
            assert all(r[kind] == 0 for r in w["log"]), w["case"]
        elif w["case"][0] == "s2s":
            lstm = [r for r in w["log"] if r[k2] > 0]
            assert len(lstm) == 1 and lstm[0][kind] != 0 and lstm[0][images] == 1, w["case"]
    for model in ("dnri_rec", "dnri_mlp"):
        step, roll = by[("s2s", model, "small", "step")], by[("s2s", model, "small", "rollout")]
        assert by[("s2s", model, "small", "ext_logits")]["logged"] < step["logged"]
        assert by[("s2s", model, "small", "encoder_features")]["logged"] < step["logged"]
        assert (roll["logged"] < 3 * step["logged"]) == (model == "dnri_mlp")
        assert roll["logged"] == 3 * step["logged"] or model == "dnri_mlp"


@pytest.mark.parametrize("case", NL.cases(), ids=lambda c: "-".join(c))
def test_launches_equal_the_recorded_ones(case):
    from aether_amd import _lib
    lib = _lib.load()
    want = {tuple(w["case"]): w for w in _golden()["cases"]}[case]
    try:
        logged, log = NL.measure(lib, case)
    finally:
        lib.aether_s2s_launch_stats_reset()
    print(f"launch log {'-'.join(case)}: {logged} launches (recorded: {want['logged']})")
    assert logged <= _lib.S2S_LAUNCH_LOG, "the log is shorter than the call"
    assert logged == want["logged"] and len(log) == len(want["log"])
    for i, (g, w) in enumerate(zip(log, want["log"])):
        assert g == w, (i, dict(zip(NL.FIELDS, g)), dict(zip(NL.FIELDS, w)))
