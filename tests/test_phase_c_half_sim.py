"""Half-height phase C of fft 32768 at L <= N/2 (Body::outer_inv_half) on the CPU wave simulator: the 16x16x32 MFMA model, the stage
against its definition, forward + backward through both sinks (E + rows_out / direct store) and the launch rule that chooses between them."""
import ctypes
import numpy as np
import pytest

import simlib as S
import simlib_phase_c as PC
from oracle import ref_fft_conv as O

N = 32768
TOL = {0: 1.2e-2, 1: 1.5e-3}     # rel-L2 gates of tests/test_sim_kernels.py: bf16, fp16


def rel(a, b):
    a = np.asarray(a, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def q(x, dt):
    return S.from_bits(S.to_bits(x, dt), dt).astype(np.float64)


@pytest.mark.parametrize("dt", [0, 1])
def test_mfma16_against_matrix_product(dt):
    """v_mfma_f32_16x16x32 in the simulator backend: D = A B + C with the ISA's lane layouts, against a float64 product.  A and B are
    asymmetric small integers (exact in both dtypes and in the fp32 sums), so a swapped row / column or k order cannot pass."""
    rng = np.random.default_rng(16 + dt)
    A = rng.integers(-8, 9, (16, 32)).astype(np.float32)
    Bm = rng.integers(-8, 9, (32, 16)).astype(np.float32)
    C = rng.integers(-64, 65, (16, 16)).astype(np.float32)
    D = PC.mfma16(dt, A, Bm, C)
    assert np.array_equal(D.astype(np.float64), A.astype(np.float64) @ Bm.astype(np.float64) + C)
    # random operands: fp32 sums of exact products, to fp32 rounding of a 32-term sum
    A, Bm = rng.standard_normal((16, 32)).astype(np.float32), rng.standard_normal((32, 16)).astype(np.float32)
    D = PC.mfma16(dt, A, Bm, np.zeros((16, 16), np.float32))
    assert rel(D, q(A, dt) @ q(Bm, dt)) < 32 * 2.0 ** -24


@pytest.mark.parametrize("dt", [0, 1])
def test_stage_against_its_definition(dt):
    """the stage alone: rows n1 < 16 of the unscaled inverse 32-point DFT over E's rows k1, per column, both planes"""
    rng = np.random.default_rng(32 + dt)
    e = (rng.standard_normal((2, 32, 1024)) * 0.125).astype(np.float32)
    out = PC.stage(dt, e)
    z = q(e[0], dt) + 1j * q(e[1], dt)
    n1, k1 = np.arange(16)[:, None], np.arange(32)[None, :]
    ref = np.exp(2j * np.pi * n1 * k1 / 32) @ z
    got = out[0].astype(np.float64) + 1j * out[1].astype(np.float64)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < TOL[dt]


# (B, H, L): all 16 rows live with an odd batch; a partly filled row; a short last chunk; one row and one chunk
SHAPES = [(3, 2, 16384), (2, 1, 8200), (2, 1, 16376), (2, 1, 1032)]


def run_case(dt, B, H, L, flags=0, pre=None, post=None, z=True):
    rng = np.random.default_rng(B * 1000 + L + dt)
    u, d = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(2))
    k = (rng.standard_normal((H, L)) * 0.1).astype(np.float32)
    kf = S.make_kf_internal(k, N, dt)
    ub, db = S.to_bits(u, dt), S.to_bits(d, dt)
    with PC.flags(flags):
        gs0 = PC.gs_count()
        if z:
            y, du, _, _, ws = S.sim_fwd_bwd_z(N, dt, ub, db, kf, pre, post)
        else:
            y = S.sim_conv_fwd(N, dt, ub, kf, pre, post)
            du, _, _ = S.sim_bwd(N, dt, db, ub, kf, L, pre, post)
        gs = PC.gs_count() - gs0
    return dict(u=u, d=d, k=k, y=y, du=du, gs=gs)


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("dt", [0, 1])
def test_forward_backward_against_oracle(dt, B, H, L):
    """forward + fused backward on saved spectra, default route (direct store): y and du against oracle/ref_fft_conv.py"""
    r = run_case(dt, B, H, L)
    assert r["gs"] == 2, "forward and backward must both have taken the direct-store kernels"
    assert rel(S.from_bits(r["y"], dt), O.ref_fft_conv(q(r["u"], dt), r["k"], N)) < TOL[dt]
    dref, _ = O.ref_grads(q(r["u"], dt), r["k"], q(r["d"], dt), N)
    assert rel(S.from_bits(r["du"], dt), dref) < TOL[dt]


@pytest.mark.parametrize("B,H,L", SHAPES[:2])
@pytest.mark.parametrize("dt", [0, 1])
def test_recomputing_backward_against_oracle(dt, B, H, L):
    r = run_case(dt, B, H, L, z=False)
    assert r["gs"] == 2
    dref, _ = O.ref_grads(q(r["u"], dt), r["k"], q(r["d"], dt), N)
    assert rel(S.from_bits(r["du"], dt), dref) < TOL[dt]


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("dt", [0, 1])
def test_both_sinks_bit_identical(dt, B, H, L):
    """plain rows take the direct store; the same call with all-ones gates takes E + rows_out (a multiply by 1.0 is exact): y and du agree
    bit for bit"""
    plain = run_case(dt, B, H, L)
    ones = S.to_bits(np.ones((B, H, L), np.float32), dt)
    gated = run_case(dt, B, H, L, pre=ones, post=ones)
    assert plain["gs"] == 2 and gated["gs"] == 0
    assert np.array_equal(plain["y"], gated["y"])
    assert np.array_equal(plain["du"], gated["du"])


@pytest.mark.parametrize("dt", [0, 1])
def test_flag_256_keeps_the_earlier_stage(dt):
    """tuning flag 256: the two-K-step stages and rows_out, no direct store; same result to the dtype's tolerance"""
    B, H, L = 3, 1, 16384
    new, old = run_case(dt, B, H, L), run_case(dt, B, H, L, flags=256)
    assert new["gs"] == 2 and old["gs"] == 0
    for key in ("y", "du"):
        assert rel(S.from_bits(new[key], dt), S.from_bits(old[key], dt).astype(np.float64)) < TOL[dt]


def test_ragged_length_takes_rows_out():
    """L % 8 != 0: element-wise rows, so the E sink; against the oracle"""
    r = run_case(0, 2, 1, 8198)
    assert r["gs"] == 0
    assert rel(S.from_bits(r["y"], 0), O.ref_fft_conv(q(r["u"], 0), r["k"], N)) < TOL[0]
    dref, _ = O.ref_grads(q(r["u"], 0), r["k"], q(r["d"], 0), N)
    assert rel(S.from_bits(r["du"], 0), dref) < TOL[0]


FAST, Z, YRAW, SPARSE, GATE, EXTRA = 1 << 19, 1 << 16, 1 << 17, 1 << 18, 1 << 20, 1 << 21


def test_launch_rule_picks_the_sink():
    """ffc::direct_store_ok through fwd_route / bwd_route: (forward, fused backward, dk_f accumulation)"""
    sink = PC.launch_sink
    assert sink(N, 16384, FAST) == (1, 1, 0)                  # plain, aligned, L % 8 == 0; the dk_f-only kernel stores no rows
    assert sink(N, 16384, FAST | Z) == (1, 1, 0)              # spectrum-saving forward
    assert sink(N, 8, FAST) == (1, 1, 0)
    assert sink(N, 16384, 0) == (0, 0, 0)                     # element-wise rows (misaligned or L % 8 != 0)
    assert sink(N, 16392, FAST) == (0, 0, 0)                  # L > N/2: full-height kernels
    assert sink(N, 16384, FAST | 256) == (0, 0, 0)            # tuning flag 256
    assert sink(N, 16384, FAST | GATE) == (0, 0, 0)           # output gate (forward) / input gate (backward)
    assert sink(N, 16384, FAST | EXTRA) == (0, 0, 0)          # addend (forward) / dpregate (backward)
    assert sink(N, 16384, FAST | Z | YRAW) == (0, 1, 0)       # second copy of the forward rows; the backward's du rows stay plain
    assert sink(N, 16384, FAST | SPARSE) == (0, 1, 0)         # frequency-sparse forward keeps rows_out
    for n, L in ((65536, 16384), (131072, 16384), (16384, 8192), (8192, 4096), (4096, 2048), (1024, 512)):
        assert sink(n, L, FAST) == (0, 0, 0), n               # multi-pass sizes and fft <= 16384: unchanged
