"""Memory waits of k_fused's prologue and edge tiles, checked on the built code object (CPU test; DESIGN.md 4.1, HISTORY R12).

The inference kernels with one and two tiles per wave, k_fused<D, 8, R, false> for D in {2, 3}, R in {1, 2}, are
disassembled (tools/isa_check.py) and read as one instruction list each.  The test looks at `s_waitcnt` and at
`flat_` instructions only.  Landmarks, all positions in the linear listing:

  (a) whole kernel: no instruction whose mnemonic starts with `flat_` (the LDS word `arrived` is an LDS-typed pointer:
      ds_write / ds_read, not flat stores and loads with sc0 sc1 and a vmcnt(0) each).
  (b) the field wave's load block.  Segment = kernel entry .. first `s_barrier` (end of P1).  In it: M = the first
      `v_mfma`; S = the last `s_load` in front of M; G = the first `global_load_dword*` behind S.  The span [G, M) is
      straight-line code of the field wave (its pointers come by scalar loads at the top of its branch, everything else
      of P1 lies in front of S or behind M).  It must hold exactly one `s_waitcnt` that names `vmcnt`, no `global_load*`
      behind that wait, and no `s_waitcnt` naming `lgkmcnt` between two `global_load*`.
  (c) the layer's tile code.  Segment = second `s_barrier` (end of P2) .. third `s_barrier` (end of the edge phase of the
      layer loop's body).  No `s_waitcnt` naming `vmcnt` may directly precede a `v_lshl_add_u64` or a fragment load
      (`global_load_dwordx4` / `buffer_load_dwordx4` into registers).  The partner-row receive of the last wave is a
      `buffer_load_dwordx4 ... sc1` followed by its own wait and is not a fragment load.

The parent of this change fails all three on all four kernels: 7-9 flat instructions, two or three vmcnt(0) in the span
of (b), and a vmcnt(0) in front of the address arithmetic of every part of the node phase's prefetch in (c)."""
import functools
import os
import re
import sys

import pytest

from conftest import REPO

KERNELS = [(D, R) for D in (2, 3) for R in (1, 2)]


@functools.lru_cache(maxsize=None)
def _kernels():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_check
    from aether_amd import _lib
    _lib.load()                                                   # builds the library if it is stale
    lib = os.environ.get("AETHER_ISA_LIB", _lib.LIB_PATH)         # (another build of the library, for comparison)
    out = {}
    for name, body in isa_check.split_kernels(isa_check.disassemble(lib)):
        m = re.search(r"7k_fusedILi(\d)ELi8ELi(\d)ELb0E", name)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = [" ".join(ins.split()) for ins in body]
    return out


def _op(ins):
    return ins.split()[0]


def _is_vm_wait(ins):
    return _op(ins) == "s_waitcnt" and "vmcnt" in ins


def _barriers(body):
    return [k for k, ins in enumerate(body) if _op(ins) == "s_barrier"]


@pytest.mark.parametrize("D,R", KERNELS)
def test_no_flat_instruction(D, R):
    body = _kernels()[(D, R)]
    flat = [ins for ins in body if _op(ins).startswith("flat_")]
    assert not flat, flat


@pytest.mark.parametrize("D,R", KERNELS)
def test_field_wave_load_block_has_one_wait(D, R):
    body = _kernels()[(D, R)]
    seg = body[:_barriers(body)[0]]
    M = next(k for k, ins in enumerate(seg) if _op(ins).startswith("v_mfma"))
    S = max(k for k in range(M) if _op(seg[k]).startswith("s_load"))
    G = next(k for k in range(S + 1, M) if _op(seg[k]).startswith("global_load_dword"))
    span = seg[G:M]
    loads = [k for k, ins in enumerate(span) if _op(ins).startswith("global_load")]
    waits = [k for k, ins in enumerate(span) if _is_vm_wait(ins)]
    assert len(loads) >= 30, len(loads)                            # the landmarks found the load block, not a fragment of it
    assert len(waits) == 1, [span[k] for k in waits]
    assert loads[-1] < waits[0], [span[k] for k in loads if k > waits[0]]
    lgkm = [span[k] for k in range(loads[0], loads[-1]) if _op(span[k]) == "s_waitcnt" and "lgkmcnt" in span[k]]
    assert not lgkm, lgkm


@pytest.mark.parametrize("D,R", KERNELS)
def test_no_wait_in_front_of_a_prefetch_part(D, R):
    body = _kernels()[(D, R)]
    b = _barriers(body)
    seg = body[b[1]:b[2]]

    def fragment_or_address(ins):
        if _op(ins) == "v_lshl_add_u64":
            return True
        return _op(ins) in ("global_load_dwordx4", "buffer_load_dwordx4") and " sc1" not in ins and not ins.endswith(" lds")

    frags = [ins for ins in seg if _op(ins) in ("global_load_dwordx4", "buffer_load_dwordx4") and fragment_or_address(ins)]
    assert len(frags) >= 16, len(frags)                            # the segment holds the node phase's prefetch
    bad = [(seg[k], seg[k + 1]) for k in range(len(seg) - 1) if _is_vm_wait(seg[k]) and fragment_or_address(seg[k + 1])]
    assert not bad, bad
