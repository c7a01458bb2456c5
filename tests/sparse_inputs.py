"""Inputs and gates shared by tests/test_sparse_gpu.py (GPU) and tests/test_sparse_recipe.py (CPU): the tone-on-a-bin recipe that makes a
frequency mask's edge visible, and the conditions under which it does.

FrequencySparseFFTConv keeps the rfft bins f < keep of the N = 2 L point spectrum of k.  On white inputs one bin more or less moves a row by
about 1 / sqrt(keep) of its norm, and by far less once the filter decays: nothing a gate of 2e-2 is sure to see.  Here x, dout and k carry, on top of
white noise 1 / 25 of their usual scale, one tone exactly on bin f0 of the N-point grid,

    s / 25 * randn + 8 s / sqrt(n) * cos(2 pi f0 t / N + phi)        (n: the row's own length, phi random per row; s = 1, k: s = 0.1)

whose bin is 4 sqrt(n) s: 4 x the rms bin (sqrt(n) s) of the unit-scale white rows the suite runs at the same size, so that no transform meets
a magnitude the other tests have not shown to be in range.  A row fills half the grid (k may fill it), so the tone also leaks 2 / pi of its
height into f0 +- 1: the results for keep = f0, f0 + 1 and f0 + 2 all differ by a large fraction of a row.

phi is drawn per (b, h) row; dout[b, h] carries phi[b, h] + DOUT_PHASE, the same offset on every row.  dk[h] sums dout[b, h] * conj(x[b, h]) over the
batch: with independent phases the B tone terms, each of the full height, add with random relative phases and cancel (B = 2: |1 + exp(i d)|).  The
rounding noise of every term stays, so that the relative error of dk then measures the cancellation and not the kernel: on the float64 oracle
sqrt(sum_b |dk_b|^2) / |dk| was 6 .. 16 on the worst head of the B = 2 cases, and exactly those missed the dk gate on the GPU by 1.1 .. 4.9 x with out
and dx at 0.1 .. 0.5 of theirs.  With one offset for all b every term has the phase DOUT_PHASE and they add in phase whatever B is.  The offset is
not zero, so that the tone's bin of dout * conj(x) is not real: a conjugation or an operand swap in the dk path turns it by 2 DOUT_PHASE = 2 rad."""
import numpy as np
import torch

from test_flashfftconv_gpu import REL

NAMES = ("out", "dx", "dk")
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
DOUT_PHASE = 1.0      # rad, see above


def gates(dtype):
    """the suite's gates (tests/test_flashfftconv_gpu.py REL; dk max(REL, 1e-2)), applied to the worst row"""
    return {"out": REL[dtype], "dx": REL[dtype], "dk": max(REL[dtype], 1e-2)}


def _tone_rows(rng, phi, n, N, f0, s):
    rows = phi.shape[:-1]
    t = np.arange(n, dtype=np.float64)
    ph = 2.0 * np.pi * ((f0 * t) % N) / N
    return (s / 25.0 * rng.standard_normal(rows + (n,)) + 8.0 * s / np.sqrt(n) * np.cos(ph + phi)).astype(np.float32)


def tone_inputs(L, Lk, B, H, f0, seed):
    """(x (B, H, L), k (H, Lk), dout (B, H, L)) float32 numpy: the recipe above, tone on bin f0 of the 2 L point grid"""
    rng = np.random.default_rng(seed)
    N = 2 * L
    phi, phi_k = rng.uniform(0.0, 2.0 * np.pi, size=(B, H, 1)), rng.uniform(0.0, 2.0 * np.pi, size=(H, 1))
    return _tone_rows(rng, phi, L, N, f0, 1.0), _tone_rows(rng, phi_k, Lk, N, f0, 0.1), _tone_rows(rng, phi + DOUT_PHASE, L, N, f0, 1.0)


def white_inputs(L, Lk, B, H, seed):
    """unit-scale x and dout, k = 0.1 randn without decay"""
    rng = np.random.default_rng(seed)
    x, dout = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(2))
    return x, (0.1 * rng.standard_normal((H, Lk))).astype(np.float32), dout


def tie_to(dout, x, sigmas=4.0):
    """dout + a x with a = sigmas / sqrt(B L): for filters of a few taps.  dk[h, j] = sum_{b, t} dout[b, h, t + j] x[b, h, t] of white rows is a sum
    of B L products of random sign, rms sqrt(B L), and any ONE of them can come out near zero -- PartialFFTConv(1) has no other, and its relative error
    is then the rounding noise of an ordinary tap over a tap that happens to be small (on the float64 oracle |dk[h, 0]| was 0.02 .. 0.07 of the row's rms
    tap where the GPU missed the gate by 5 .. 46 x, with P = 7 on the same inputs inside it).  The term a x adds a B L = sigmas sqrt(B L) to tap 0: it
    stands `sigmas` rms taps above zero, the other taps and both spectra keep their white statistics."""
    B, _, L = x.shape
    return (dout + sigmas / np.sqrt(B * L) * x).astype(np.float32)


def peak_over_white_rms(row, N, s):
    """largest bin of the row's N-point spectrum / rms bin of white noise of scale s and the row's length"""
    return float(np.abs(np.fft.rfft(np.asarray(row, np.float64), n=N)).max() / (s * np.sqrt(row.shape[-1])))


def separation(a, b):
    """how far two oracle results are apart: per row |a - b| / max(|a|, |b|) (what a module that computes b where a is wanted, or a where b is
    wanted, shows AT LEAST as its relative error), the smallest over the rows"""
    a = np.asarray(a, np.float64).reshape(-1, a.shape[-1])
    b = np.asarray(b, np.float64).reshape(-1, b.shape[-1])
    den = np.maximum(np.maximum(np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)), 1e-30)
    return float((np.linalg.norm(a - b, axis=-1) / den).min())


def min_separations(want, f0, k_fills_grid=False):
    """{name: smallest pairwise separation of the oracle's results for keep = f0, f0 + 1, f0 + 2}.
    k_fills_grid (Lk = N, the routes reached only with such a k): the tone of k is then periodic over the grid and leaks NOTHING into f0 + 1, so that
    out and dx, which carry a factor k_f, differ between keep = f0 + 1 and f0 + 2 by x's leak times k's noise floor only (measured 0.0066) -- that
    pair cannot be apart there and is left out for them (dk = dout * conj(x) keeps it).  The pairs with f0 are what the two runs keep = f0 and
    keep = f0 + 1 need: a mask one bin too wide shows in the first, one bin too narrow in the second.  The same routes run with Lk = 3 N / 4 and all pairs."""
    pairs = ((f0, f0 + 1), (f0 + 1, f0 + 2), (f0, f0 + 2))
    with_k = tuple(p for p in pairs if p != (f0 + 1, f0 + 2)) if k_fills_grid else pairs
    return {nm: min(separation(want[p][i], want[q][i]) for p, q in (pairs if nm == "dk" else with_k)) for i, nm in enumerate(NAMES)}


def assert_separated(want, f0, dtype, k_fills_grid=False):
    """the condition under which a mask edge off by one bin cannot pass: 5 x the gate between any two of the three neighbouring keeps"""
    sep, tol = min_separations(want, f0, k_fills_grid), gates(dtype)
    for nm in NAMES:
        assert sep[nm] >= 5 * tol[nm], f"f0 = {f0}: the oracle's {nm} for keep = f0, f0 + 1, f0 + 2 are only {sep[nm]:.3g} apart (< 5 x {tol[nm]:.1e})"
    return sep
