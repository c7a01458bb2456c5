"""Rotated pair loops of the plain-row kernels of fft 32768 at L <= N/2 on the CPU wave simulator (csrc/ffc_body.h Body::outer_jobs, ROT:
the next pair's rows are written to E at the bottom of an iteration, behind phase C; csrc/ffc_modes.h Modes::bwd, ROT: the finish of
the next pair's row copies -- wait, zeroing of what lies beyond L / B, fence -- stands there too, the first pair's in a prologue).

The comparison partner is the same call under tuning flag 512: the direct-store kernels with the run-time arms, whose pair loops keep the
earlier order.  The rotation moves instructions and changes no arithmetic, so y, the saved spectra, du and dk must agree bit for bit.
The flag-512 path is checked against the float64 oracle on its own on every shape, so a failure of the equality points at the rotation.

Shapes, (B, H, L) -- chosen for where a rotated loop can go wrong, one property per row as far as the simulator's speed allows:
  B = 2: one pair, the prologue alone and no successor;  B = 4: exactly one back edge;  B = 7: three back edges and an odd batch, the
  last pair's missing row is zeroed by the moved store / finish;  L = 16376: a tail inside the last row;  L = 8200: a tail inside row 8
  and seven rows that are dead altogether, zeroed at the bottom of the loop;  H = 3: a workgroup's loop starts again with a prologue
  for every head.  L = 1032 (not asked for by name): below 4 rows the du / y stores of whole instructions have no active lane -- the
  counted wait of the backward counts instructions, active or not.
More than one chunk per head: the simulator's forward always runs one chunk per head (ffcsim_conv_fwd), its backward takes a chunk count:
B = 7 in two chunks of two pairs, each with its own prologue and one back edge, the second one ending on the odd pair."""
import ctypes
import numpy as np
import pytest

import simlib as S
import simlib_phase_c as PC
from oracle import ref_fft_conv as O

N = 32768
TOL = {0: 1.2e-2, 1: 1.5e-3}     # rel-L2 gates of tests/test_sim_kernels.py and tests/test_phase_c_half_sim.py: bf16, fp16 (dk: 1.5 x bf16's)
SHAPES = [(2, 1, 16384), (4, 1, 16376), (7, 1, 8200), (4, 3, 8200), (2, 3, 16376), (7, 1, 16384), (4, 1, 1032)]
CHUNKED = (7, 1, 16376)          # backward in two chunks per head
_RUNS = {}
_pl_total = 0


def pl_count():
    """runs of a plain-input kernel variant so far (monotonic)"""
    global _pl_total
    S.lib().ffcsim_pl_count.restype = ctypes.c_long
    _pl_total += S.lib().ffcsim_pl_count()
    return _pl_total


def dk_from_slabs(dt, ws, H, L):
    nt, _, _, _ = S.plan_info(N, dt)
    dk = np.full((H, L), np.nan, np.float32)
    assert S.lib().ffcsim_kernel_ifft_grad(N, dt, S.p(ws), ws.size // (H * nt * 2048), H, L, S.p(dk)) == 0
    return dk


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30)


def q(x, dt):
    return S.from_bits(S.to_bits(x, dt), dt).astype(np.float64)


def inputs(dt, B, H, L):
    rng = np.random.default_rng(B * 1000 + H * 77 + L + dt)
    u, d = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(2))
    k = (rng.standard_normal((H, L)) * 0.1).astype(np.float32)
    return u, d, k


def run(dt, B, H, L, flags, nchunk=1):
    """forward without spectra (y0), spectrum-saving forward (y1, z) and the backward on those spectra (du, dk), all under `flags`; computed
    once per argument set and shared by the tests below (nobody writes to the results)"""
    key = (dt, B, H, L, flags, nchunk)
    if key in _RUNS:
        return _RUNS[key]
    u, d, k = inputs(dt, B, H, L)
    ub, db, kf = S.to_bits(u, dt), S.to_bits(d, dt), S.make_kf_internal(k, N, dt)
    lib = S.lib()
    nt, _, _, _ = S.plan_info(N, dt)
    with PC.flags(flags):
        pl0 = pl_count()
        y0 = S.sim_conv_fwd(N, dt, ub, kf)
        z = np.zeros(((B + 1) // 2) * H * N * 2, np.uint16)
        y1, du = np.zeros_like(ub), np.zeros_like(ub)
        ws = np.full(nchunk * lib.ffcsim_upw(N) * H * nt * 2048, np.nan, np.float32)
        lib.ffcsim_set_z(S.p(z), None, 0)
        try:
            assert lib.ffcsim_conv_fwd(N, dt, S.p(ub), S.p(kf), None, None, S.p(y1), B, H, L, 0) == 0
            nslab = lib.ffcsim_conv_bwd(N, dt, S.p(db), S.p(ub), S.p(kf), None, None, S.p(du), None, None, S.p(ws), B, H, L, nchunk)
        finally:
            lib.ffcsim_set_z(None, None, 0)
        assert nslab == nchunk, nslab
        pl = pl_count() - pl0
    dk = dk_from_slabs(dt, ws[: nslab * H * nt * 2048].copy(), H, L)
    _RUNS[key] = dict(u=u, d=d, k=k, y0=y0, y1=y1, z=z, du=du, dk=dk, pl=pl)
    return _RUNS[key]


def check_oracle(r, dt):
    yref = O.ref_fft_conv(q(r["u"], dt), r["k"], N)
    duref, dkref = O.ref_grads(q(r["u"], dt), r["k"], q(r["d"], dt), N)
    errs = dict(y0=rel(S.from_bits(r["y0"], dt), yref), y1=rel(S.from_bits(r["y1"], dt), yref), du=rel(S.from_bits(r["du"], dt), duref),
                dk=rel(r["dk"], dkref))
    print({k: f"{v:.3e}" for k, v in errs.items()})
    assert errs["y0"] < TOL[dt] and errs["y1"] < TOL[dt] and errs["du"] < TOL[dt], errs
    assert not np.isnan(r["dk"]).any() and errs["dk"] < 1.5 * TOL[0], errs


def check_equal(new, old):
    assert new["pl"] == 3, "the two forwards and the backward must all have taken the plain-input kernels"
    assert old["pl"] == 0, "flag 512 keeps the direct-store kernels with the run-time arms"
    for key in ("y0", "y1", "z", "du"):
        assert np.array_equal(new[key], old[key]), f"{key}: {int((new[key] != old[key]).sum())} elements differ from the flag-512 run"
    assert np.array_equal(new["dk"].view(np.uint32), old["dk"].view(np.uint32)), "dk differs from the flag-512 run"


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp16"])
def test_flag_512_alone_against_oracle(dt, B, H, L):
    """the comparison partner on its own: the kernels with the earlier loop order against the float64 oracle"""
    check_oracle(run(dt, B, H, L, 512), dt)


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp16"])
def test_rotated_loops_bit_identical_to_flag_512(dt, B, H, L):
    """forward with and without spectra, backward on the saved spectra: y, the spectra, du and dk bit for bit, and the oracle tolerance"""
    new = run(dt, B, H, L, 0)
    check_equal(new, run(dt, B, H, L, 512))
    check_oracle(new, dt)


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp16"])
def test_backward_in_two_chunks_per_head(dt):
    """every chunk starts with a prologue of its own (full wait) and ends without a finish; the second chunk ends on the odd pair"""
    B, H, L = CHUNKED
    old = run(dt, B, H, L, 512, nchunk=2)
    check_oracle(old, dt)
    new = run(dt, B, H, L, 0, nchunk=2)
    check_equal(new, old)
    check_oracle(new, dt)
