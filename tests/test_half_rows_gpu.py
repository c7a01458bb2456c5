"""The half-row form of the HBM levels (csrc/ffc_big.h BigArgs::half, flashfftconv/conv.py _big_half): every B = 1 call that runs through a single
level stores the rows k0 <= K / 2 only, and the inverse level gives each stored row weight 2, or 1 for the self-conjugate rows k0 = 0 and K / 2.
One case per single-level route the product reaches with B = 1, both dtypes, gated and not, at UNIT scale with a filter that does not decay
(every row of the level and every frequency is live), against the numpy float64 oracle on the CPU (oracle/ref_fft_conv.py) evaluated on the
inputs as rounded to the module dtype.  A wrong weight on one self-conjugate row is ~ sqrt(1 / K) relative (0.25 at K = 16, 0.09 at K = 128), a
dropped mirror half ~ 0.7: far above the gates, which are the suite's own (tests/test_flashfftconv_gpu.py REL; x 1.5 gated; dk max(REL, 1e-2)),
applied per (b, h) row so that one wrong head is not diluted."""
import time
import numpy as np
import pytest
import torch

from oracle import ref_fft_conv as O
from test_flashfftconv_gpu import REL, rel

pytestmark = pytest.mark.gpu

# N, L = Lk, expected (factors, inner size), H, fit_fft
ROUTES = [
    (131072, 100004, ((32,), 4096), 2, True),        # routed by length (L > N / 2: one level around the fused 4096 kernel)
    (262144, 100004, ((16,), 16384), 2, True),       # folded outer twiddle of the inner size
    (524288, 262144, ((16,), 32768), 2, True),
    (1048576, 400004, ((32,), 32768), 2, True),
    (2097152, 1000001, ((64,), 32768), 2, True),     # L <= N / 2, L % 8 != 0: element-wise long-side accesses
    (2097152, 1500001, ((32,), 65536), 2, True),     # two-pass inner kernel, no kept spectra
    (4194304, 1048576, ((128,), 32768), 2, False),   # L <= N / 4; fit_fft off: the rows would fit 2097152 points
]
IDS = [f"{n}-{l}" for n, l, _, _, _ in ROUTES]
NAMES = ("out", "du", "dk", "dpregate", "dpostgate")


def _row_rel(got, want):
    """worst relative L2 error over the (b, h) rows (dk: the h rows)"""
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape, (got.shape, want.shape)
    g2, w2 = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    return max(rel(g2[i], w2[i]) for i in range(g2.shape[0]))


def _gates(dtype, gated):
    f = 1.5 if gated else 1.0
    return {nm: f * (max(REL[dtype], 1e-2) if nm == "dk" else REL[dtype]) for nm in NAMES}


class _Route:
    """asserts that a call really ran the route its case names: the factorisation, and what conv._big_half answered"""

    def __init__(self, monkeypatch, N, L, fac):
        from flashfftconv import bigfft, conv as C
        assert bigfft.choose(N, L, C._TorchOps) == fac, (bigfft.choose(N, L, C._TorchOps), fac)
        self.seen = []
        inner = C._big_half

        def recording(mod, B, Lmax, f):
            r = inner(mod, B, Lmax, f)
            self.seen.append((mod.seqlen, f, r))
            return r
        monkeypatch.setattr(C, "_big_half", recording)
        self.N, self.fac = N, fac

    def expect(self, half, calls=1):
        assert self.seen == [(self.N, self.fac, half)] * calls, self.seen
        self.seen.clear()


def _module(N, dtype, fit):
    from flashfftconv import FlashFFTConv
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    conv.fit_fft = fit
    return conv


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,L,fac,H,fit", ROUTES, ids=IDS)
def test_half_rows_against_the_float64_oracle(N, L, fac, H, fit, dtype, gated, monkeypatch):
    """forward, du, dk and both gate gradients of the half-row form with kept spectra, without them and (forward) under no_grad, and of the
    full-row form of the same call (conv._BIG_HALF off), each against the float64 oracle"""
    from flashfftconv import conv as C
    t0 = time.time()
    torch.manual_seed(N + L + 2 * int(gated) + int(dtype == torch.float16))
    B = 1
    conv = _module(N, dtype, fit)
    assert conv._fit_seqlen(L, L) == N
    route = _Route(monkeypatch, N, L, fac)
    u, pre, post, dout = (torch.randn(B, H, L, device="cuda").to(dtype) for _ in range(4))
    k = torch.randn(H, L, device="cuda") * 0.1
    gates = (pre, post) if gated else ()
    # the oracle, once: numpy float64 on the host, on the inputs as rounded to the module dtype
    h = [t.double().cpu().numpy() for t in (u, k, dout) + gates]
    if gated:
        want = (O.ref_fft_conv_gated(h[0], h[1], h[3], h[4], N),) + tuple(O.ref_grads(h[0], h[1], h[2], N, h[3], h[4]))
    else:
        want = (O.ref_fft_conv(h[0], h[1], N),) + tuple(O.ref_grads(h[0], h[1], h[2], N))
    t_ref = time.time() - t0
    tol = _gates(dtype, gated)

    def run(save):
        conv.save_spectrum = save
        leaves = [t.clone().requires_grad_(True) for t in (u, k) + gates]
        y = conv(*leaves)
        return (y.detach(),) + tuple(torch.autograd.grad(y, leaves, dout))

    res = {}
    for what, save in (("half, spectra kept", True), ("half, recomputed", False)):
        res[what] = run(save)
        route.expect(True)
    with torch.no_grad():
        res["half, no_grad"] = (conv(u, k, *gates),)
    route.expect(True)
    # without a graph no spectra are stored (another kernel variant): the same output bit for bit, as run_case asserts for fft >= 4096
    for what in ("half, spectra kept", "half, recomputed"):
        assert torch.equal(res["half, no_grad"][0], res[what][0]), f"forward under no_grad against '{what}': {int((res['half, no_grad'][0] != res[what][0]).sum())} elements differ"
    monkeypatch.setattr(C, "_BIG_HALF", False)
    res["full rows"] = run(True)
    route.expect(False)
    errs = {what: {nm: _row_rel(a, w) for nm, a, w in zip(NAMES, r, want)} for what, r in res.items()}
    print(f"\nhalf_rows N={N} L={L} {fac[0][0]}x{fac[1]} H={H} {'fp16' if dtype == torch.float16 else 'bf16'} {'gated' if gated else 'plain'}: "
          + "  ".join(f"{nm} {errs['half, spectra kept'][nm]:.2e}|{errs['full rows'][nm]:.2e}" for nm in NAMES[:len(want)])
          + f"  (half|full, worst row; oracle {t_ref:.1f} s, case {time.time() - t0:.1f} s)")
    for what, e in errs.items():
        for nm, v in e.items():
            assert v < tol[nm], f"{what}: {nm} rel-L2 of the worst (b, h) row {v:.3e} >= {tol[nm]:.1e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,L,fac,H,fit", ROUTES, ids=IDS)
def test_half_rows_shift_a_single_tap(N, L, fac, H, fit, dtype, monkeypatch):
    """k = one tap of value 1 at q: the output is u delayed by q samples (circularly over the N zero-padded points) and du is dout advanced by q,
    for q at the start, across the first inner row (M - 1, M; M = the inner size) and at the filter's end.  Needs no oracle.
    The error is taken relative to the norm of the WHOLE shifted sequence (= |u| resp. |dout|: a shift moves energy, it does not change it), of which
    the L returned samples are a window: the rounding noise of an N-point FFT convolution is proportional to the energy that goes through the
    transforms and lands on all N points alike.  For q << L the window holds nearly all of that energy and this is the plain relative error; at
    q = Lk - 1 with L <= N / 2 the window holds ONE live sample (u[0] at t = L - 1) next to L - 1 samples of that noise, where an error relative to the
    window's own norm measures |u| / |u[0]| and not the kernel (measured: 0.13 .. 16 at every such route)."""
    torch.manual_seed(N + L + int(dtype == torch.float16))
    B, M = 1, fac[1]
    conv = _module(N, dtype, fit)
    assert conv._fit_seqlen(L, L) == N
    route = _Route(monkeypatch, N, L, fac)
    u, dout = (torch.randn(B, H, L, device="cuda").to(dtype) for _ in range(2))
    pad = lambda t: torch.nn.functional.pad(t, (0, N - L))
    for q in (0, 1, M - 1, M, L - 1):
        k = torch.zeros(H, L, device="cuda")
        k[:, q] = 1.0
        ul = u.clone().requires_grad_(True)
        y = conv(ul, k)
        (du,) = torch.autograd.grad(y, (ul,), dout)
        route.expect(True)
        want_y = torch.roll(pad(u), q, -1)[..., :L]
        want_du = torch.roll(pad(dout), -q, -1)[..., :L]
        for nm, a, w, src in (("out", y, want_y, u), ("du", du, want_du, dout)):
            e = ((a.double() - w.double()).norm(dim=-1) / src.double().norm(dim=-1)).max().item()      # per (b, h) row, no floor
            assert e < REL[dtype], f"q = {q}: {nm} error of the worst row / norm of the shifted row {e:.3e}"
        if q == L - 1:
            # the samples that no wrap-around and no zero padding touches at the last tap: y[L - 1] = u[0], du[0] = dout[L - 1].  On the routes with
            # L <= N / 2 they are the only live ones, so they get a check of their own: the row gate above bounds the rms error per sample by
            # REL * rms(row); one sample of that noise stays below 4 x its rms (4 sigma), an error of the order of the sample itself does not
            for nm, got, want, src in (("out", y[..., L - 1], u[..., 0], u), ("du", du[..., 0], dout[..., L - 1], dout)):
                bound = 4 * REL[dtype] * src.double().pow(2).mean(dim=-1).sqrt()
                err = (got.double() - want.double()).abs()
                assert bool((err < bound).all()), f"q = {q}: {nm}, the one sample carried across the whole filter: |error| {err.max().item():.3e}, bound {bound.min().item():.3e}"
