"""The HBM-level kernels on batch-strided long-side tensors (csrc/ffc_big.h BigArgs::pin / pout / pgate; ffc_outer_pass*_strided), on the CPU wave
simulator: one level run on operands that are channel slices of a wider (B, 3H, L) array -- the way the fused Hyena / M2 operator hands x1, x2, v
and the slices of d(uc) to the levels (flashfftconv/hyena.py); the gate comes from an array of another width, so that every operand has a pitch of
its own -- against the same level on contiguous copies through the entry points without pitches.

The arithmetic of the two runs is the same and only the addresses differ, so the results must agree BIT FOR BIT; that is derived, not measured.
The other slices hold a NaN sentinel: a level that reads a neighbour poisons its result, and after an inverse level every element outside the target
slice must still hold the sentinel.  Every form of a level that forms a long-side row offset is covered: the plain level of factor 16 and 32, the
factors 64 / 128 as one launch per pass (the inverse passes c > 0 read-modify-write the output) and as one launch, and the half-row form (B = 1); an odd
batch (the last pair has no partner row: the kernels clamp the batch index) and B = 1; rows of a multiple of 8 elements on 16-byte aligned slices
(16-byte accesses) and an odd length just below it (element-wise accesses, unaligned slices, pitches that are no multiple of 8); both dtypes."""
import numpy as np
import pytest

import simlib as S
import simlib_strided as SS

H = 2
# form -> (factor n0, all passes in one launch, half rows, Mi: the smallest the level accepts = its column block, as tests/test_sim_kernels.py uses)
FORMS = {
    "16": (16, True, False, 1024),
    "32": (32, True, False, 512),
    "64-per-pass": (64, False, False, 512),
    "128-per-pass": (128, False, False, 512),
    "64-one-launch": (64, True, False, 512),
    "128-one-launch": (128, True, False, 512),
    "32-half": (32, True, True, 512),
    "64-half": (64, True, True, 512),
    "64-half-per-pass": (64, False, True, 512),
}
CASES = [(f, B) for f, v in FORMS.items() for B in ((1,) if v[2] else (3, 1))]


def _ops(cls, one_launch, half):
    ops = cls()
    ops.one_launch, ops.half = one_launch, half
    return ops


def _embed(values, j, width=3):
    """values (B, H, L) bits as slice j of a 16-byte aligned (B, width * H, L) array of sentinels -> (array, view of the slice)"""
    B, Hh, L = values.shape
    big = SS.aligned_full((B, width * Hh, L), SS.SENTINEL)
    view = big[:, j * Hh:(j + 1) * Hh]
    view[...] = values
    return big, view


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("odd", [False, True], ids=["L%8==0", "odd-L"])
@pytest.mark.parametrize("form,B", CASES, ids=[f"{f}-B{b}" for f, b in CASES])
def test_level_on_channel_slices_is_the_level_on_copies(form, B, odd, dt, gated):
    from flashfftconv import bigfft as BG
    n0, one_launch, half, mi = FORMS[form]
    lmax = min(n0, 32) * mi                      # the long side of the factors 64 / 128 is the first 32 rows
    L = lmax - 24 - (1 if odd else 0)            # the last row is cut short; odd: no 16-byte access anywhere
    npair = (B + 1) // 2
    rows = n0 // 2 + 1 if half else n0
    rng = np.random.default_rng(n0 * 1000 + B * 10 + L % 7)
    x, g = (S.to_bits(rng.standard_normal((B, H, L)).astype(np.float32), dt) for _ in range(2))
    cont, strd = _ops(S.SimOps, one_launch, half), _ops(SS.StridedSimOps, one_launch, half)
    nan = 0x7fc0 if dt == 0 else 0x7e00

    # ---- forward: input = slice 2 of a (B, 3H, L) array, gate = slice 1 of a (B, 2H, L) array: the two pitches differ, so a kernel that took
    # one operand's pitch for the other's would read sentinels; the pair-plane output is contiguous
    uc, xv = _embed(x, 2)
    garr, gv = _embed(g, 1, width=2)
    assert SS.pitch(xv, H, L) == 3 * H * L and SS.pitch(gv, H, L) == 2 * H * L and (xv.ctypes.data % 16 == 0) == (not odd)
    mids = []
    for ops, a, b in ((cont, x, g), (strd, xv, gv)):
        mid = np.full((2 * npair, H * rows, mi), nan, np.uint16)       # NaN-filled: every element must be written
        ops.outer(dt, n0, True, a, mid, b if gated else None, B, npair, H, mi, L, BG.level_scale(n0))
        mids.append(mid)
    assert np.array_equal(mids[0], mids[1]), f"forward: {int((mids[0] != mids[1]).sum())} elements differ"
    assert not np.isnan(S.from_bits(mids[0], dt)).any()
    keep, gkeep = np.full(uc.shape, SS.SENTINEL, np.uint16), np.full(garr.shape, SS.SENTINEL, np.uint16)
    keep[:, 2 * H:], gkeep[:, H:] = x, g
    assert np.array_equal(uc, keep) and np.array_equal(garr, gkeep), "the forward level wrote to its input"

    # ---- inverse: output = slice 1 of a (B, 3H, L) array of sentinels (a gradient slice of d(uc)), gate = the (B, 2H, L) array's slice
    sc = 1.0 / (n0 * BG.level_scale(n0))
    out_c = np.full((B, H, L), SS.SENTINEL, np.uint16)
    cont.outer(dt, n0, False, mids[0], out_c, g if gated else None, B, npair, H, mi, L, sc)
    duc = SS.aligned_full((B, 3 * H, L), SS.SENTINEL)
    ov = duc[:, H:2 * H]
    strd.outer(dt, n0, False, mids[0], ov, gv if gated else None, B, npair, H, mi, L, sc)
    assert np.array_equal(ov, out_c), f"inverse: {int((ov != out_c).sum())} elements differ"
    assert not np.isnan(S.from_bits(np.ascontiguousarray(ov), dt)).any()
    assert (duc[:, :H] == SS.SENTINEL).all() and (duc[:, 2 * H:] == SS.SENTINEL).all(), "the inverse level wrote outside its slice"
    assert np.array_equal(garr, gkeep), "the inverse level wrote to its gate"


def test_pitch_rules_of_the_strided_entry_points():
    """a pitch below Hin * Llong, or one on the (contiguous) pair-plane side, is refused; 0 means contiguous"""
    import ctypes
    dt, n0, mi, L, B = 0, 32, 512, 16000, 2
    x = S.to_bits(np.ones((B, H, L), np.float32), dt)
    mid = np.zeros((2, H * n0, mi), np.uint16)
    i64, f = ctypes.c_int64, ctypes.c_float(0.125)
    call = lambda pi, po, pg: S.lib().ffcsim_big_outer_strided(n0, dt, 1, S.p(x), S.p(mid), None, B, 1, H, mi, L, f, i64(pi), i64(po), i64(pg))
    assert call(0, 0, 0) == 0 and call(H * L, 0, 0) == 0
    ref = mid.copy()
    S.SimOps().outer(dt, n0, True, x, ref, None, B, 1, H, mi, L, 0.125)
    assert np.array_equal(mid, ref)
    assert call(H * L - 8, 0, 0) != 0 and call(0, H * n0 * mi, 0) != 0
