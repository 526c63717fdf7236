"""Inputs and numpy restatement for tests/test_gpu_split_forms.py: 24 tiles of [16 rows][64 features] for
aether_debug_split, and what csrc/common.h (split_scale_of, split8) makes of them.

A lane of the wave that owns a tile holds row i = lane & 15 and, with q = lane >> 4, the features 16 b + 4 q + j
(b, j < 4): lanes 48-63 are the features f with f % 16 >= 12 -- the lanes the packed-fp32 operand hazard of DESIGN.md 4.0b
corrupted.  Every special value is placed there and in lanes 0-15."""
import numpy as np

N_TILES = 24
F32 = np.float32
SCALES = (-30, -24, -18, -12, -7, 0, 5, 10, 15, 20)
Q3, Q0 = (12, 29, 46, 63), (0, 17, 34, 51)                     # features of lanes 48-63 / 0-15, one per 16-feature block


def _below(v):
    return np.nextafter(F32(v), F32(0))


def _above(v):
    return np.nextafter(F32(v), F32(np.inf))


def _place(tile, values):
    """values[k] into (row, feature) slots that alternate between lanes 48-63 and lanes 0-15, signs alternating by row"""
    for k, v in enumerate(values):
        for row, feats in ((k % 16, Q3), ((k + 5) % 16, Q0)):
            f = feats[(k // 4 + k // 16) % 4]
            tile[row, f] = F32(v) if row % 2 == 0 else -F32(v)


def make_inputs():
    rng = np.random.default_rng(20240607)
    x = np.zeros((N_TILES, 16, 64), F32)
    for t, e in enumerate(SCALES):                              # 0-9: one scale per tile, 2^-30 .. 2^20
        x[t] = (rng.standard_normal((16, 64)) * 2.0 ** e).astype(F32)
    x[10] = (rng.standard_normal((16, 64)) * 2.0 ** rng.integers(-30, 21, (16, 64))).astype(F32)   # every scale in one tile
    # 11: nothing but +0
    sub = (rng.integers(1, 1 << 23, (16, 64)).astype(np.uint32)).view(F32)                          # 12: +-0 and fp32 subnormals
    x[12] = np.where(rng.random((16, 64)) < 0.5, sub, F32(0)) * np.where(rng.random((16, 64)) < 0.5, F32(1), F32(-1))
    x[12, 3, 12] = np.uint32(1).view(F32)
    x[12, 4, 0] = -np.uint32(0x007FFFFF).view(F32)
    base = lambda: (rng.standard_normal((16, 64)) * 0.5).astype(F32)
    x[13] = base()                                              # 13: fp16 rounding ties (to even: down, up), next to them
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.0, 2051.0, 0.5 + 2.0 ** -12, 2.0 ** -14 + 2.0 ** -25, 3 * 2.0 ** -25,
            2.0 ** -25]
    _place(x[13], ties + [_below(t) for t in ties] + [_above(t) for t in ties])
    x[14] = base()                                              # 14: lo an fp16 subnormal; hi an fp16 subnormal
    _place(x[14], [0.5 + 2.0 ** -20, 0.25 + 3 * 2.0 ** -24, 1 + 2.0 ** -15 - 2.0 ** -24, 0.125 + 2.0 ** -24, 2.0 ** -15,
                   3 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 0.75 + 2.0 ** -25, 2.0 ** -26])
    x[15] = base()                                              # 15: maximum just below 2^15 (plain path: hi rounds up to 2^15)
    _place(x[15], [_below(32768.0), 32752.0, 16384.0 + 4.0])
    x[16] = base()                                              # 16: maximum 2^15 exactly (scaled)
    _place(x[16], [32768.0, _below(32768.0)])
    x[17] = base()                                              # 17: around fp16's top
    _place(x[17], [_below(65504.0), 65504.0, _above(65504.0), _below(65520.0), 65520.0, 70000.0])
    small = lambda: (rng.standard_normal((16, 64)) * 2.0 ** -10).astype(F32).clip(-2.0 ** -7, 2.0 ** -7)
    x[18] = small()                                             # 18: maximum just below 2^-6 (scaled)
    _place(x[18], [_below(2.0 ** -6)])
    x[19] = small()                                             # 19: maximum 2^-6 exactly (plain)
    _place(x[19], [2.0 ** -6, _below(2.0 ** -6)])
    x[20] = base(); x[20, 2, 63] = np.inf; x[20, 9, 17] = np.inf            # 20 / 21: inf
    x[21] = base(); x[21, 5, 0] = -np.inf; x[21, 5, 46] = -np.inf
    x[22] = base(); x[22, 7, 29] = np.nan                                   # 22: NaN in one lane (48-63), plain range
    x[23] = small() * F32(2.0 ** -8); x[23, 11, 20] = np.nan                # 23: NaN in one lane (16-31), scaled range
    return x


def scale_decision(tile):
    """split_scale_of on a wave's tile -> (on, s).  A lane's maximum drops NaN elements (fmaxf / v_max3_f32 in IEEE mode),
    so the three ballots see the maximum over the tile's non-NaN values."""
    m = np.fmax.reduce(np.abs(tile).ravel(), initial=F32(0))
    big, some, any_ = m >= F32(32768), m >= F32(0.015625), m > 0
    on = bool(big or (any_ and not some))
    if not on:
        return False, F32(1)
    E = (int(np.asarray(m, F32).view(np.uint32)) >> 23) & 255
    sh = max(-40, min(40, 140 - E))
    return True, F32(2.0 ** sh)


def reference(x):
    """-> hi, lo (uint16 bit patterns), on (int32), scale (float32) per tile"""
    hi = np.zeros(x.shape, np.uint16)
    lo = np.zeros(x.shape, np.uint16)
    on = np.zeros(len(x), np.int32)
    scale = np.zeros(len(x), F32)
    with np.errstate(all="ignore"):
        for t, tile in enumerate(x):
            on[t], scale[t] = scale_decision(tile)
            xs = (tile * scale[t]).astype(F32) if on[t] else tile
            h = xs.astype(np.float16)
            l = (xs - h.astype(F32)).astype(np.float16)
            hi[t], lo[t] = h.view(np.uint16), l.view(np.uint16)
    return hi, lo, on, scale


def same_bits_or_both_nan(got, want):
    """bit patterns equal; where `want` is a NaN, any NaN will do (payloads are not compared)"""
    if got.dtype == np.uint16:
        nan = lambda a: ((a & 0x7C00) == 0x7C00) & ((a & 0x03FF) != 0)
    else:
        got, want = got.view(np.uint32), want.view(np.uint32)
        nan = lambda a: ((a & 0x7F800000) == 0x7F800000) & ((a & 0x007FFFFF) != 0)
    return np.where(nan(want), nan(got), got == want)
