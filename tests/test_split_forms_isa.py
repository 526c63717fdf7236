"""Vector instructions of the range test and the fp16 split (csrc/common.h: absmax4 / split_scale_of, split_pair / split8),
checked on the built code object (CPU test; DESIGN.md 4.0, profiles/r20_split_forms.txt).

Every k_fused instantiation, k_fused_bwd, k_s2s_gemm_split(_r1), k_s2s_filter_split, k_wgemm and k_edge_layer are
disassembled (tools/isa_check.py) and counted:

  (a) no `v_max_f32 d, |x|, |x|` -- the quieting of a fabsf operand in front of an IEEE fmaxf, 16 per range test in the
      parent (154 in the flagship k_fused<2, 12, 1, false, true>).  The lane maximum is eight v_max3_f32 with abs modifiers.
      One pair of them is not the range test's and stays: the device math library's atan2f (node_frame, once per node in the
      prologue) forms min(|x|, |y|) and max(|x|, |y|) from two quieted operands; that pair is recognised by the v_min_f32
      that reads both results and is allowed once per atan2f call site (one in k_fused).  Everything else fails.
  (b) no v_cvt_f32_f16 (the parent widened every hi piece again to subtract it: 184 in the flagship);
      lo = fp16(fma(fp32(hi), -1, x)) is one v_fma_mixlo_f16 / v_fma_mixhi_f16 per value, its fp16 source read from the low
      half of a register (no op_sel bit on a source: DESIGN.md 4.0b).
  (c) v_cvt_pk_f16_f32 at most half the parent's count (the lo pieces no longer go through it).
  (d) no instantiation gains scratch memory; the 12-wave kernels stay at or below 168 VGPRs."""
import functools
import os
import re
import sys

import pytest

from conftest import REPO

# parent (commit 538eb68): kernel -> (v_cvt_pk_f16_f32, scratch bytes)
PARENT_FUSED = {(D, W, R, K, E): v for D in (2, 3) for (W, R, K, E), v in {
    (12, 1, 0, 0): (184, 0), (12, 1, 0, 1): (184, 0), (8, 1, 0, 0): (168, 0), (8, 1, 1, 0): (168, 0), (8, 2, 0, 0): (208, 0),
    (8, 2, 1, 0): (208, 0), (8, 3, 0, 0): (248, 0), (8, 3, 1, 0): (248, 12)}.items()}
PARENT_OTHER = {"k_fused_bwdILi1E": (120, 0), "k_fused_bwdILi2E": (240, 0), "k_fused_bwdILi3E": (360, 0),
                "k_s2s_gemm_splitILi1E": (32, 0), "k_s2s_gemm_splitILi2E": (64, 0), "k_s2s_gemm_split_r1ILi1E": (16, 0),
                "k_s2s_gemm_split_r1ILi2E": (32, 0), "7k_wgemmE": (64, 0), "12k_edge_layerE": (40, 0),
                "k_s2s_filter_splitILi11E": (0, 60), "k_s2s_filter_splitILi15E": (0, 60), "k_s2s_filter_splitILi18E": (0, 60),
                "k_s2s_filter_splitILi24E": (0, 60), "k_s2s_filter_splitILi28E": (0, 60), "k_s2s_filter_splitILi39E": (0, 64),
                "k_s2s_filter_splitILi43E": (0, 68), "k_s2s_filter_split_typesILi15E": (0, 60)}
TWELVE_WAVES = [k for k in PARENT_FUSED if k[1] == 12] + ["12k_edge_layerE"]
ALL = sorted(PARENT_FUSED) + sorted(PARENT_OTHER)


@functools.lru_cache(maxsize=None)
def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_check
    from aether_amd import _lib
    _lib.load()                                                   # builds the library if it is stale
    lib = os.environ.get("AETHER_ISA_LIB", _lib.LIB_PATH)         # (another build of the library, for comparison)
    notes = isa_check.kernel_notes(lib, counts=True)
    out = {}
    for name, body in isa_check.split_kernels(isa_check.disassemble(lib)):
        m = re.search(r"7k_fusedILi(\d)ELi(\d+)ELi(\d)ELb([01])ELb([01])E", name)
        key = tuple(int(g) for g in m.groups()) if m else next((k for k in PARENT_OTHER if k in name), None)
        if key is not None:
            assert key not in out, (key, name)
            out[key] = ([" ".join(ins.split()) for ins in body], notes[name], isa_check.operands)
    return out


def _op(ins):
    return ins.split()[0]


def _count(body, prefix):
    return sum(1 for ins in body if _op(ins).startswith(prefix))


def test_every_kernel_is_found():
    assert sorted(_kernels(), key=str) == sorted(ALL, key=str)


@pytest.mark.parametrize("key", ALL, ids=str)
def test_no_quieting_self_max(key):
    body, _notes, operands = _kernels()[key]
    selfmax = []
    for k, ins in enumerate(body):
        ops = operands(ins)
        if _op(ins).startswith("v_max_f32") and len(ops) == 3 and ops[1] == ops[2] and ops[1].startswith("|"):
            selfmax.append(k)
    # atan2f's pair: two of them, both read by one v_min_f32 within the next four instructions
    atan2 = []
    for a, b in zip(selfmax, selfmax[1:]):
        da, db = operands(body[a])[0], operands(body[b])[0]
        if any(_op(ins).startswith("v_min_f32") and {da, db} <= set(operands(ins)[1:]) for ins in body[b + 1:b + 5]):
            atan2 += [a, b]
    allowed = 2 if isinstance(key, tuple) else 0                  # k_fused calls atan2f once (node_frame); the others never
    assert len(atan2) <= allowed, [body[k] for k in atan2]
    rest = [body[k] for k in selfmax if k not in atan2]
    assert not rest, rest


@pytest.mark.parametrize("key", ALL, ids=str)
def test_split_is_cvt_pk_and_mix(key):
    body, _notes, _ = _kernels()[key]
    parent_pk = (PARENT_FUSED.get(key) or PARENT_OTHER.get(key))[0]
    pk, mix = _count(body, "v_cvt_pk_f16_f32"), _count(body, "v_fma_mix")
    assert _count(body, "v_cvt_f32_f16") == 0
    assert 2 * pk <= parent_pk, (pk, parent_pk)
    assert mix == 2 * pk, (mix, pk)                               # one per value
    bad = [ins for ins in body if _op(ins).startswith("v_fma_mix") and re.search(r"op_sel:\[", ins)]
    assert not bad, bad[:3]                                       # fp16 sources from the low half only


@pytest.mark.parametrize("key", ALL, ids=str)
def test_registers_and_scratch(key):
    _body, notes, _ = _kernels()[key]
    parent_scratch = (PARENT_FUSED.get(key) or PARENT_OTHER.get(key))[1]
    assert notes[2] <= parent_scratch, (notes[2], parent_scratch)
    if key in TWELVE_WAVES:
        assert notes[3]["vgpr_count"] <= 168, notes[3]
