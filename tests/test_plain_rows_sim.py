"""Plain-row kernels of fft 32768 at L <= N/2 (csrc/ffc_route.h plain_rows_ok, Body::rows_load_pl / rows_store_pl, Modes::bwd<.., PL>) on
the CPU wave simulator: the kernels that are plain on the input side at compile time against the direct-store kernels with the run-time
arms (tuning flag 512).  Nothing arithmetic differs between the two -- the same loads, masks, LDS writes and transforms in the same order --
so equality of the bits is the derived gate, not a tolerance.  And the launch rule that chooses between them."""
import ctypes
import numpy as np
import pytest

import simlib as S
import simlib_phase_c as PC

N = 32768
# (B, H, L), the rows of tests/test_phase_c_half_gpu.py: all 16 rows live; an odd batch (missing partner row); a partly filled row; a short
# last chunk; one row and one chunk; exactly 15 rows
SHAPES = [(2, 2, 16384), (3, 2, 16384), (2, 3, 8200), (2, 2, 16376), (2, 2, 1032), (4, 1, 15360)]
_pl_total = 0


def pl_count():
    """runs of a plain-input kernel variant so far (monotonic)"""
    global _pl_total
    S.lib().ffcsim_pl_count.restype = ctypes.c_long
    _pl_total += S.lib().ffcsim_pl_count()
    return _pl_total


def inputs(dt, B, H, L):
    rng = np.random.default_rng(B * 1000 + H * 77 + L + dt)
    u, d = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(2))
    k = (rng.standard_normal((H, L)) * 0.1).astype(np.float32)
    return S.to_bits(u, dt), S.to_bits(d, dt), S.make_kf_internal(k, N, dt)


def dk_from_slabs(dt, ws, H, L):
    nt, _, _, _ = S.plan_info(N, dt)
    nslab = ws.size // (H * nt * 2048)
    dk = np.full((H, L), np.nan, np.float32)
    assert S.lib().ffcsim_kernel_ifft_grad(N, dt, S.p(ws), nslab, H, L, S.p(dk)) == 0
    return dk


def run_case(dt, B, H, L, save, flags=0, pre=None, post=None, slow=False):
    """forward (spectrum-saving or not) + fused backward (on the saved spectra or recomputing): y, du bits, dk fp32, and how many of the
    two launches took a direct-store kernel (gs) and its plain-input form (pl)"""
    ub, db, kf = inputs(dt, B, H, L)
    S.lib().ffcsim_force_slow_io(int(slow))
    try:
        with PC.flags(flags):
            gs0, pl0 = PC.gs_count(), pl_count()
            if save:
                y, du, _, _, ws = S.sim_fwd_bwd_z(N, dt, ub, db, kf, pre, post)
                dk = dk_from_slabs(dt, ws, H, L)
            else:
                y = S.sim_conv_fwd(N, dt, ub, kf, pre, post)
                du, _, dk = S.sim_bwd(N, dt, db, ub, kf, L, pre, post)
            gs, pl = PC.gs_count() - gs0, pl_count() - pl0
    finally:
        S.lib().ffcsim_force_slow_io(0)
    return dict(y=y, du=du, dk=dk, gs=gs, pl=pl)


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp16"])
def test_plain_variant_bit_identical_to_flag_512(dt, save, B, H, L):
    """forward with / without spectra and backward saved / recomputing: the default (plain-input kernels) against tuning flag 512 (the
    direct-store kernels with the run-time arms): y, du and dk bit for bit"""
    new, old = run_case(dt, B, H, L, save), run_case(dt, B, H, L, save, flags=512)
    assert (new["gs"], new["pl"]) == (2, 2), "forward and backward must both have taken the plain-input kernels"
    assert (old["gs"], old["pl"]) == (2, 0), "flag 512 keeps the direct-store kernels with the run-time arms"
    for key in ("y", "du"):
        assert np.array_equal(new[key], old[key]), f"{key}: {int((new[key] != old[key]).sum())} elements differ"
    assert not np.isnan(new["dk"]).any()
    assert np.array_equal(new["dk"].view(np.uint32), old["dk"].view(np.uint32)), "dk"


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
def test_general_kernels_where_the_input_side_is_not_plain(save):
    """the route names the general kernels for a ragged length, an input gate and a misaligned base (element-wise rows); an all-ones gate
    multiplies by 1.0 exactly and element-wise rows carry the same values, so the bits are those of the plain call"""
    dt, B, H = 0, 2, 1
    r = run_case(dt, B, H, 8198, save)                       # L % 8 != 0: element-wise rows, neither form of the direct store
    assert (r["gs"], r["pl"]) == (0, 0)
    L = 8200
    plain = run_case(dt, B, H, L, save)
    assert (plain["gs"], plain["pl"]) == (2, 2)
    ones = S.to_bits(np.ones((B, H, L), np.float32), dt)
    if not save:      # (the simulator's saved pair keeps y_raw for any gate: it gates both sides or none)
        # forward: u * pregate, plain output -> direct store, run-time arms; backward: its output gate is that pregate -> E + rows_out
        fwd_gate = run_case(dt, B, H, L, save, pre=ones)
        assert (fwd_gate["gs"], fwd_gate["pl"]) == (1, 0)
        assert np.array_equal(fwd_gate["y"], plain["y"]) and np.array_equal(fwd_gate["du"], plain["du"])
        bwd_gate = run_case(dt, B, H, L, save, post=ones)
        # backward: dout * postgate on the way in, plain du rows -> direct store, run-time arms; the forward's output gate -> rows_out
        assert (bwd_gate["gs"], bwd_gate["pl"]) == (1, 0)
        assert np.array_equal(bwd_gate["y"], plain["y"]) and np.array_equal(bwd_gate["du"], plain["du"])
    slow = run_case(dt, B, H, L, save, slow=True)            # misaligned base: the library clears `fast`, as this switch does
    assert (slow["gs"], slow["pl"]) == (0, 0)
    assert np.array_equal(slow["y"], plain["y"]) and np.array_equal(slow["du"], plain["du"])


FAST, Z, GATE, SIDE, DPOST = 1 << 19, 1 << 16, 1 << 20, 1 << 21, 1 << 22


def launch_plain(n, L, fl, B=4, H=2, dt=0):
    out = np.zeros(2, np.int32)
    assert S.lib().ffcsim_launch_plain(n, dt, B, H, L, fl, S.p(out)) == 0
    return tuple(int(v) for v in out)


def test_launch_rule_picks_the_plain_variant():
    """ffc::plain_rows_ok through fwd_route / bwd_route: (forward, fused backward)"""
    for L in (16384, 8200, 16376, 1032, 15360, 8):
        for z in (0, Z):
            assert launch_plain(N, L, FAST | z) == (1, 1), (L, z)
            assert launch_plain(N, L, FAST | z, dt=1) == (1, 1)
            assert launch_plain(N, L, FAST | z | 512) == (0, 0)       # tuning flag 512: the kernels with the run-time arms
            assert launch_plain(N, L, FAST | z | 256) == (0, 0)       # no direct store, so no plain-input form of it
            assert launch_plain(N, L, FAST | z | GATE) == (0, 0)      # an input gate: pregate (forward), postgate (backward)
            assert launch_plain(N, L, FAST | z | SIDE) == (0, 0)      # the side product of the row load
            assert launch_plain(N, L, FAST | z | DPOST) == (1, 0)     # the backward's dpost transform
            assert launch_plain(N, L, FAST | z | 8) == (1, 0)         # tuning flag 8: the backward's rows through registers
            assert launch_plain(N, L, z) == (0, 0)                    # a misaligned base or stride: element-wise rows
    assert launch_plain(N, 8198, 0) == (0, 0)                         # L % 8 != 0
    assert launch_plain(N, 16392, FAST) == (0, 0)                     # L > N/2: full-height kernels
    for n, L in ((65536, 16384), (131072, 16384), (16384, 8192), (8192, 4096), (4096, 2048), (1024, 512)):
        assert launch_plain(n, L, FAST) == (0, 0), n                  # multi-pass sizes and fft <= 16384: unchanged
