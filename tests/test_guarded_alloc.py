"""The guard-band harness of the buffer-contract tests (tests/guarded_alloc.py), exercised on CPU tensors: the device
type to guard is a parameter, and the interposer does not care which allocator the bytes come from."""
import pytest
import torch

from guarded_alloc import BAND, GuardedAlloc, GuardError


def _cpu():
    return GuardedAlloc(device_type="cpu")


def test_a_clean_run_reports_nothing_and_records_exact_payloads():
    g = _cpu()
    with g:
        a = torch.empty(5, 3, dtype=torch.float32)
        b = torch.empty_like(a)
        c = torch.empty((7,), dtype=torch.int64, device="cpu")
        a.zero_()
        b.fill_(2.0)
        c.copy_(torch.arange(7))
    g.check()
    assert [r.nbytes for r in g.allocations] == [60, 60, 56]
    assert [r.shape for r in g.allocations] == [(5, 3), (5, 3), (7,)]
    assert [r.dtype for r in g.allocations] == [torch.float32, torch.float32, torch.int64]
    assert [r.kind for r in g.allocations] == ["empty", "empty_like", "empty"]
    for r, t in zip(g.allocations, (a, b, c)):
        assert r.raw.numel() == 2 * BAND + r.nbytes and r.raw.dtype == torch.uint8
        assert t.data_ptr() == r.raw.data_ptr() + BAND and t.is_contiguous()
        assert g.holds(t) is r
    assert g.find(nbytes=56)[0] is g.allocations[2] and g.find(shape=(5, 3), dtype=torch.float32) == g.allocations[:2]
    assert BAND == 64 * 1024 and BAND % 512 == 0


def test_a_fresh_payload_reads_back_as_nan_and_minus_one():
    g = _cpu()
    with g:
        f32 = torch.empty(4, 6)
        f16 = torch.empty(9, dtype=torch.float16)
        i32 = torch.empty(3, dtype=torch.int32)
        i64 = torch.empty(2, 2, dtype=torch.int64)
        u8 = torch.empty(5, dtype=torch.uint8)
    assert torch.isnan(f32).all() and torch.isnan(f16).all()
    assert (i32 == -1).all() and (i64 == -1).all() and (u8 == 0xFF).all()
    g.check()


@pytest.mark.parametrize("side,offset", [("below", -1), ("below", -BAND), ("above", 0), ("above", BAND - 1)])
def test_one_byte_in_a_band_is_reported_with_allocation_and_offset(side, offset):
    g = _cpu()
    with g:
        torch.empty(8)
        t = torch.empty(3, 5, dtype=torch.float32)
        torch.empty(2)
    rec = g.allocations[1]
    pos = BAND + offset if side == "below" else BAND + rec.nbytes + offset
    rec.raw[pos] = 0
    with pytest.raises(GuardError) as e:
        g.check()
    msg = str(e.value)
    want = offset if side == "below" else rec.nbytes + offset
    assert "allocation #1" in msg and "shape=(3, 5)" in msg and "torch.float32" in msg and "bytes=60" in msg
    assert "from tests/test_guarded_alloc.py:" in msg          # the call site of the allocation
    assert f"band {side} the payload" in msg and f"offsets {want}..{want} " in msg
    assert "allocation #0" not in msg and "allocation #2" not in msg
    assert torch.isnan(t).all()                      # the payload itself was not touched


def test_a_run_of_bytes_reports_first_and_last_offset():
    g = _cpu()
    with g:
        torch.empty(16, dtype=torch.float32)
    rec = g.allocations[0]
    rec.raw[BAND + 64 + 4:BAND + 64 + 4 + 256] = 7
    with pytest.raises(GuardError, match=r"256 byte\(s\) of the band above the payload changed, payload-relative offsets 68\.\.323 "):
        g.check()


def test_torch_empty_is_the_original_again_after_the_block_and_after_an_exception():
    empty, empty_like = torch.empty, torch.empty_like
    g = _cpu()
    with g:
        assert torch.empty is not empty and torch.empty_like is not empty_like
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(RuntimeError, match="boom"):
        with g:
            torch.empty(3)
            raise RuntimeError("boom")
    assert torch.empty is empty and torch.empty_like is empty_like
    n = len(g.allocations)
    torch.empty(3)
    assert len(g.allocations) == n                   # nothing is recorded outside the block


def test_zero_element_requests_work():
    g = _cpu()
    with g:
        a = torch.empty(0)
        b = torch.empty(0, 2, dtype=torch.int64)
        c = torch.empty_like(b)
        d = torch.empty((3, 0, 4), dtype=torch.float16)
    assert a.shape == (0,) and b.shape == (0, 2) and c.shape == (0, 2) and d.shape == (3, 0, 4)
    assert [r.nbytes for r in g.allocations] == [0, 0, 0, 0]
    g.check()
    g.allocations[1].raw[BAND] = 1                   # with an empty payload the upper band starts at offset 0
    with pytest.raises(GuardError, match=r"allocation #1 .*offsets 0\.\.0 "):
        g.check()


def test_other_devices_strided_results_and_out_pass_through():
    g = GuardedAlloc(device_type="cuda")             # guards CUDA only: CPU requests pass through unchanged
    with g:
        t = torch.empty(4)
    assert g.allocations == [] and t.shape == (4,)
    g = _cpu()
    with g:
        m = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        like = torch.empty_like(torch.zeros(4, 6).t())
        meta = torch.empty(3, device="meta")
        dst = torch.zeros(5)
        torch.empty(5, out=dst)
    assert g.allocations == []
    assert m.is_contiguous(memory_format=torch.channels_last) and like.stride() == (1, 6) and meta.is_meta
    assert (dst == 0).all()


def test_views_modules_and_an_optimizer_step_work_inside_the_block():
    g = _cpu()
    torch.manual_seed(0)
    with g:
        buf = torch.empty(1024, dtype=torch.uint8)
        v = buf[256:512].view(torch.float32).view(8, 8)
        v.fill_(1.0)
        lin = torch.nn.Linear(6, 3)
        opt = torch.optim.AdamW(lin.parameters(), lr=1e-2)
        x = torch.empty(4, 6, requires_grad=True)
        with torch.no_grad():
            x.normal_()
        lin(x).square().sum().backward()
        before = lin.weight.detach().clone()
        opt.step()
    assert x.requires_grad and x.grad is not None and torch.isfinite(x.grad).all()
    assert not torch.equal(before, lin.weight.detach()) and torch.isfinite(lin.weight).all()
    assert g.holds(lin.weight) is not None and g.holds(lin.bias) is not None and g.holds(buf) is not None
    assert float(v.sum()) == 64.0 and (buf[:256] == 0xFF).all() and (buf[512:] == 0xFF).all()
    g.check()


def test_guarded_copy_poisons_float_inputs_and_zeroes_index_inputs():
    g = _cpu()
    x = torch.randn(5, 2)
    idx = torch.arange(10, dtype=torch.int64).view(2, 5)
    mask = torch.tensor([True, False, True])
    gx, gi, gm = g.guarded_copy(x), g.guarded_copy(idx), g.guarded_copy(mask)
    gt = g.guarded_copy(x.t())                       # a strided input is copied in its contiguous form
    assert torch.equal(gx, x) and torch.equal(gi, idx) and torch.equal(gm, mask) and torch.equal(gt, x.t())
    assert gt.is_contiguous() and [r.kind for r in g.allocations] == ["input"] * 4
    rx, ri, rm = g.allocations[:3]
    assert rx.nbytes == 40 and ri.nbytes == 80 and rm.nbytes == 3
    for r, byte in ((rx, 0xFF), (ri, 0), (rm, 0)):
        assert (r.raw[:BAND] == byte).all() and (r.raw[BAND + r.nbytes:] == byte).all()
    # what a kernel that reads one row past the end would get
    assert torch.isnan(rx.raw[BAND + 40:BAND + 48].view(torch.float32)).all()
    assert (ri.raw[BAND + 80:BAND + 96].view(torch.int64) == 0).all()
    assert g.find() == []                            # inputs are not among the operation's own allocations
    g.check()
    ri.raw[BAND + 80] = 1                            # a write past an index input is found against ITS fill byte
    with pytest.raises(GuardError, match=r"allocation #1 \(input\).*band above"):
        g.check()
