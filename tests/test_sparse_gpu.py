"""FrequencySparseFFTConv and PartialFFTConv (flashfftconv/sparse_conv.py) on every route an fft size 2 L can take, forward, dx and dk against the
numpy float64 oracle on the CPU (oracle/ref_fft_conv.py), evaluated on the inputs as rounded to the module dtype.  The gates are the suite's own
(tests/test_flashfftconv_gpu.py REL: bf16 2e-2, fp16 5e-3; dk max(REL, 1e-2)), applied to the worst (b, h) row of out and dx and the worst h row of dk.

(a) the mask's edge: a tone on bin f0 (tests/sparse_inputs.py) with keep = f0 and f0 + 1, where one bin more or less is most of a row;
(b) white unit-scale inputs with a graph, under no_grad and in eval mode, with an odd batch and with more than one fp32 dk_f slab;
(c) the edges of N_partial, the module's conv cache and its errors;
(d) PartialFFTConv;
(e) (a) again with a mask deliberately built one bin too wide: the comparison must fail, or (a) proves nothing.

Every case asserts the route it names (_SparseRoute): what bigfft.choose returned, that conv._big_half answered False (the masks are laid out over all inner
rows) and with which `rows` the compute-skipping kernel ran (conv._conv_sparse), or that it did not.  Every module run prints one `sparse_parity` line
(pytest -s): profiles/sparse_parity.txt is made of them."""
import math
import time
import numpy as np
import pytest
import torch

from oracle import ref_fft_conv as O
import sparse_inputs as SI
from test_half_rows_gpu import _row_rel

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
# L, Lk, path, (outer factors, inner size) of the HBM-level routes.  fft size N = 2 L.
ROUTES = [
    (128, 128, "tile", None), (256, 256, "tile", None), (512, 512, "tile", None),
    (1024, 1024, "2pass", None),                         # fft 2048: 2 passes of the 1024 kernel
    (2048, 2048, "dense", None), (4096, 4096, "dense", None),
    (8192, 8192, "sp", None), (16384, 16384, "sp", None),        # compute-skipping forward for rows 1 .. 4, dense above
    (32768, 32768, "multipass", None), (65536, 65536, "multipass", None),      # 2 / 4 passes of the 32768 kernel, mask over the multi-pass k_f index
    (65536, 131072, "level", ((32,), 4096)),             # routed by length (Lk > N / 2); k fills the grid
    (65536, 98304, "level", ((32,), 4096)),              # ... the same route with a k that does not (sparse_inputs.min_separations)
    (131072, 131072, "level", ((16,), 16384)),
    (262144, 262144, "level", ((16,), 32768)),
    (524288, 524288, "level", ((32,), 32768)),
    (1048576, 1048576, "level", ((64,), 32768)),         # rows in c * 32 + d order
    (1048576, 2097152, "level", ((32,), 65536)),         # Lk > N / 2: the 2-pass inner kernel; k fills the grid
    (1048576, 1572864, "level", ((32,), 65536)),         # ... and does not
    (2097152, 2097152, "level", ((16, 16), 16384)),      # two levels
]
BIG_N = 1048576      # from this fft size up: B = 2, H = 1, bf16 (fp16 on the 2M (64,) route and on 4M)


def _dtypes(L, fac):
    if 2 * L < BIG_N:
        return (BF, FP)
    return (BF, FP) if fac in (((64,), 32768), ((16, 16), 16384)) else (BF,)


def _rid(L, Lk):
    return f"L{L}" + ("" if Lk == L else f"-k{Lk}")


def _route_name(L, path, fac):
    return f"fft{2 * L}:" + (path if fac is None else "x".join(str(f) for f in fac[0]) + f"x{fac[1]}")


class _SparseRoute:
    """asserts that a call really ran the route its case names"""

    def __init__(self, monkeypatch, L, Lk, path, fac):
        from flashfftconv import bigfft, conv as C
        self.N, self.Lmax, self.path, self.fac, self.C = 2 * L, max(L, Lk), path, fac, C
        if fac is not None:
            assert bigfft.choose(self.N, self.Lmax, C._TorchOps) == fac, (bigfft.choose(self.N, self.Lmax, C._TorchOps), fac)
        self.chosen, self.half, self.rows = [], [], []
        choose, half, sparse = bigfft.choose, C._big_half, C._conv_sparse

        def rec_choose(N, Lmax, ops=None):
            r = choose(N, Lmax, ops)
            self.chosen.append((N, r))
            return r

        def rec_half(mod, B, Lmax, f):
            r = half(mod, B, Lmax, f)
            self.half.append((mod.seqlen, f, r))
            return r

        def rec_sparse(plan, u, kf, pregate, postgate, conj, rows):
            self.rows.append((plan.seqlen, rows))
            return sparse(plan, u, kf, pregate, postgate, conj, rows)
        monkeypatch.setattr(bigfft, "choose", rec_choose)
        monkeypatch.setattr(C, "_big_half", rec_half)
        monkeypatch.setattr(C, "_conv_sparse", rec_sparse)

    def sp_rows(self, keep):
        """rows per side the compute-skipping kernel must have been given for this keep; 0: the dense kernel"""
        r = -(-keep // (self.N // 32))
        return r if self.path == "sp" and 1 <= r <= 4 else 0

    def expect(self, conv, keep, forwards=1):
        """after `forwards` forward calls of the module's conv (a frequency-sparse module with that keep; keep None: a dense one)"""
        N, C = self.N, self.C
        assert conv.seqlen == N
        if self.path == "level":
            assert conv._big or conv._route_big(self.Lmax)
            assert self.chosen == [(N, self.fac)] * forwards, self.chosen
            assert self.half == [(N, self.fac, False)] * forwards, self.half
        else:
            assert not conv._big and not conv._route_big(self.Lmax) and not conv._folded and conv._plan_seqlen == N
            assert self.chosen == [] and self.half == [], (self.chosen, self.half)
            assert {"tile": N in (256, 512, 1024), "2pass": N == 2048 and N in C.MULTIPASS_SEQLENS, "dense": N in (4096, 8192),
                    "sp": N in (16384, 32768), "multipass": N in (65536, 131072) and N in C.MULTIPASS_SEQLENS}[self.path]
        r = self.sp_rows(keep) if keep is not None else 0
        assert self.rows == ([(N, r)] * forwards if r else []), (self.rows, r)
        self.chosen.clear(); self.half.clear(); self.rows.clear()


def _to_gpu(x, k, dout, dtype):
    """device tensors (x, dout rounded to the module dtype, k fp32) and the float64 host copies the oracle reads"""
    xg, dg = (torch.from_numpy(t).to("cuda").to(dtype) for t in (x, dout))
    kg = torch.from_numpy(k).to("cuda")
    return (xg, kg, dg), tuple(t.double().cpu().numpy() for t in (xg, kg, dg))


def _fwd_bwd(mod, xg, kg, dg):
    xl, kl = xg.clone().requires_grad_(True), kg.clone().requires_grad_(True)
    y = mod(xl, kl)
    dx, dk = torch.autograd.grad(y, (xl, kl), dg)
    assert dk.shape == kg.shape and dk.dtype == kg.dtype and dx.dtype == xg.dtype
    return y.detach(), dx, dk


def _errs(got, want):
    return {nm: _row_rel(g.float(), w) for nm, g, w in zip(SI.NAMES, got, want)}


def _line(part, L, Lk, path, fac, dtype, B, H, what, errs, tol):
    print(f"\nsparse_parity ({part}) {_route_name(L, path, fac)} L={L} Lk={Lk} B={B} H={H} {SI.DT_NAME[dtype]} {what}: "
          + "  ".join(f"{nm} {errs[nm]:.2e}" for nm in errs) + "   [gates " + " | ".join(f"{tol[nm]:.0e}" for nm in errs) + "]", end="")


def _check(errs, tol, what):
    for nm, v in errs.items():
        assert v < tol[nm], f"{what}: {nm} rel-L2 of the worst row {v:.3e} >= {tol[nm]:.1e}"


# ------------------------------------------------------------------------------------------------ (a) the mask's edge on a tone
_BH = ((1, 1), (2, 3), (3, 2), (2, 1), (3, 3), (1, 2))


def _tone_bins(L, path, fac):
    N = 2 * L
    if N >= BIG_N:
        P = math.prod(fac[0])
        return [3 * P - 1, N // 2 - P]          # below the 3rd multiple of the levels' stride (odd, low); ON the (M / 2 - 1)th, the highest below N / 2 - 3
    f = [3 if N < 2048 else 37, N // 2 - 3]
    if path == "sp":                            # keep = f0 + 1 exactly on and just past a row boundary: rows 1 | 2 and 4 | dense
        f += [N // 32 - 1, N // 32, 4 * N // 32 - 1, 4 * N // 32]
    if path == "level":                         # inner positions q - 1 | q of the last and the first inner row, q = 11
        P = math.prod(fac[0])
        f += [11 * P - 1, 11 * P]
    return f


def _tone_cases():
    out = []
    for L, Lk, path, fac in ROUTES:
        for dtype in _dtypes(L, fac):
            for i, f0 in enumerate(_tone_bins(L, path, fac)):
                B, H = (2, 1) if 2 * L >= BIG_N else _BH[(i + (dtype == FP)) % len(_BH)]
                out.append(pytest.param(L, Lk, path, fac, dtype, f0, B, H, id=f"{_rid(L, Lk)}-f{f0}-B{B}H{H}-{SI.DT_NAME[dtype]}"))
    return out


def _tone_setup(L, Lk, B, H, f0, dtype):
    """device inputs and the oracle's {keep: (out, dx, dk)} for keep = f0, f0 + 1, f0 + 2, asserted far enough apart -- before any GPU call"""
    x, k, dout = SI.tone_inputs(L, Lk, B, H, f0, seed=L + Lk + 7 * f0 + int(dtype == FP))
    dev, host = _to_gpu(x, k, dout, dtype)
    want = O.ref_freq_sparse_keeps(*host[:2], host[2], (f0, f0 + 1, f0 + 2))
    sep = SI.assert_separated(want, f0, dtype, k_fills_grid=Lk == 2 * L)
    return dev, want, sep


@pytest.mark.parametrize("L,Lk,path,fac,dtype,f0,B,H", _tone_cases())
def test_mask_edge_on_a_tone(L, Lk, path, fac, dtype, f0, B, H, monkeypatch):
    """N_partial = 2 f0, 2 f0 + 1 (odd: floor) and 2 f0 + 2, i.e. keep = f0, f0 and f0 + 1, each against the oracle of its keep: a mask one bin too
    wide, too narrow, or wrong on the mirror side (f >= N - keep for f > N - keep) misses at least one of them by most of a row"""
    from flashfftconv import FrequencySparseFFTConv
    t0 = time.time()
    dev, want, sep = _tone_setup(L, Lk, B, H, f0, dtype)
    t_ref = time.time() - t0
    route = _SparseRoute(monkeypatch, L, Lk, path, fac)
    tol = SI.gates(dtype)
    bad = []
    for n_partial in (2 * f0, 2 * f0 + 1, 2 * f0 + 2):
        keep = n_partial // 2
        mod = FrequencySparseFFTConv(n_partial).to("cuda")
        errs = _errs(_fwd_bwd(mod, *dev), want[keep])
        route.expect(mod._convs[(2 * L, dtype)], keep)
        _line("a", L, Lk, path, fac, dtype, B, H, f"f0={f0} N_partial={n_partial} keep={keep} rows={route.sp_rows(keep)}", errs, tol)
        bad += [f"N_partial = {n_partial}: {nm} {v:.3e} >= {tol[nm]:.1e}" for nm, v in errs.items() if not v < tol[nm]]
    print(f"   (separation {min(sep.values()):.2f}; oracle {t_ref:.1f} s, case {time.time() - t0:.1f} s)")
    assert not bad, "rel-L2 of the worst row: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ (e) proof that (a) bites
@pytest.mark.parametrize("L,Lk,path,fac,f0", [(256, 256, "tile", None, 3), (16384, 16384, "sp", None, 1023),
                                               (1048576, 1048576, "level", ((64,), 32768), 3 * 64 - 1)], ids=["L256", "L16384", "L1048576"])
def test_a_mask_one_bin_too_wide_fails_the_tone_comparison(L, Lk, path, fac, f0, monkeypatch):
    """correct kernels under a mask built for keep + 1: every comparison of (a) must then miss by at least 2.5 x its gate"""
    from flashfftconv import FrequencySparseFFTConv, FlashFFTConv, conv as C
    t0 = time.time()
    dtype, (B, H) = BF, (2, 1)
    dev, want, _ = _tone_setup(L, Lk, B, H, f0, dtype)

    def widened(fn):
        def wrong(mod, *args):
            true = mod._kf_keep
            mod._kf_keep = true + 1
            try:
                return fn(mod, *args)
            finally:
                mod._kf_keep = true
        return wrong
    monkeypatch.setattr(FlashFFTConv, "_kf_mask", widened(FlashFFTConv._kf_mask))
    monkeypatch.setattr(C, "_big_kf_mask", widened(C._big_kf_mask))
    route = _SparseRoute(monkeypatch, L, Lk, path, fac)
    tol = SI.gates(dtype)
    for n_partial in (2 * f0, 2 * f0 + 2):
        keep = n_partial // 2
        mod = FrequencySparseFFTConv(n_partial).to("cuda")
        errs = _errs(_fwd_bwd(mod, *dev), want[keep])
        route.expect(mod._convs[(2 * L, dtype)], keep)
        _line("e", L, Lk, path, fac, dtype, B, H, f"f0={f0} keep={keep}, mask built for {keep + 1}", errs, tol)
        for nm, v in errs.items():
            assert v >= 2.5 * tol[nm], f"keep = {keep} under a mask for {keep + 1}: {nm} misses by only {v:.3e} (< 2.5 x {tol[nm]:.1e})"
    print(f"   (case {time.time() - t0:.1f} s)")


# ------------------------------------------------------------------------------------------------ (b) white inputs
def _slab_count(conv, B, H, fac):
    """fp32 dk_f slabs of this call's backward: the inner plan's count for the pair-plane rows at an HBM-level size"""
    from flashfftconv import _lib
    if fac is None:
        return _lib.lib().ffc_dkf_slab_count(conv._get_plan(torch.device("cuda", torch.cuda.current_device())).handle, B, H)
    plan = conv._get_plan(torch.device("cuda", torch.cuda.current_device()), fac[1])
    return _lib.lib().ffc_dkf_slab_count(plan.handle, 2 * ((B + 1) // 2), H * math.prod(fac[0]))


def _white_cases():
    out = []
    for L, Lk, path, fac in ROUTES:
        if Lk not in (L, 2 * L):
            continue
        N = 2 * L
        # small and odd: 37, not 3 or 5.  On white inputs a kept bin's own energy |x_f|^2 scatters (exponentially) around the level that sets the rounding
        # noise of every bin, so that over a handful of bins the worst row's relative error measures that scatter: on the float64 oracle
        # sqrt(sum_f |k_f|^2 mean |x|^2 / sum_f |x_f k_f|^2) reached 4.8 at keep = 5 (fft 1M; measured out 2.8e-2, dx 3.8e-2 there, 5.8e-3 and
        # 1.2e-2 once divided by it).  Over 37 bins the factor stays within 1 +- 0.2; the lowest bins themselves are what (a) puts its tone on
        keeps = [37, N // 8 - 5, N // 3] + ([3 * N // 32 - 5] if path == "sp" else [])      # rows 1, 4, dense (+ 3)
        B, H = (2, 1) if N >= BIG_N else (3, 2)
        for dtype in _dtypes(L, fac):
            for keep in keeps:
                out.append(pytest.param(L, Lk, path, fac, dtype, keep, B, H, 1, id=f"{_rid(L, Lk)}-keep{keep}-{SI.DT_NAME[dtype]}"))
    # the smallest (B, H) with more than one fp32 dk_f slab (csrc/ffc_dev.h ffc_choose_chunks: a second chunk needs more pairs than a workgroup takes per
    # iteration -- 8 units / waves per unit, x G sequences per tile at the single-tile sizes): fft 1024 B = 17; fft 32768 B = 3; fft 524288 = 16 x 32768 B = 3,
    # whose two pairs are four pair-plane rows = two pairs of the inner 32768 plan
    for L, path, fac, B in ((512, "tile", None, 17), (16384, "sp", None, 3), (262144, "level", ((16,), 32768), 3)):
        for dtype in (BF, FP):
            out.append(pytest.param(L, L, path, fac, dtype, L // 4 - 5, B, 1, 2, id=f"L{L}-slabs-B{B}H1-{SI.DT_NAME[dtype]}"))
    return out


@pytest.mark.parametrize("L,Lk,path,fac,dtype,keep,B,H,min_slabs", _white_cases())
def test_white_inputs_graph_no_grad_eval(L, Lk, path, fac, dtype, keep, B, H, min_slabs, monkeypatch):
    """unit-scale x and dout, k = 0.1 randn without decay (every kept bin is live): the forward with a graph, under no_grad and in eval mode, and the backward"""
    from flashfftconv import FrequencySparseFFTConv
    t0 = time.time()
    dev, host = _to_gpu(*SI.white_inputs(L, Lk, B, H, seed=L + Lk + keep + int(dtype == FP)), dtype)
    want = O.ref_freq_sparse_conv(host[0], host[1], 2 * keep, host[2])
    t_ref = time.time() - t0
    route = _SparseRoute(monkeypatch, L, Lk, path, fac)
    tol = SI.gates(dtype)
    mod = FrequencySparseFFTConv(2 * keep + 1).to("cuda")
    errs = _errs(_fwd_bwd(mod, *dev), want)
    conv = mod._convs[(2 * L, dtype)]
    route.expect(conv, keep)
    nslab = _slab_count(conv, B, H, fac)
    assert nslab >= min_slabs, (nslab, min_slabs)
    with torch.no_grad():
        errs["out, no_grad"] = _row_rel(mod(dev[0], dev[1]).float(), want[0])
    mod.eval()
    y = mod(dev[0], dev[1].clone().requires_grad_(True))
    assert not conv.training
    errs["out, eval"] = _row_rel(y.detach().float(), want[0])
    route.expect(conv, keep, 2)
    tol = dict(tol, **{"out, no_grad": tol["out"], "out, eval": tol["out"]})
    _line("b", L, Lk, path, fac, dtype, B, H, f"keep={keep} rows={route.sp_rows(keep)} slabs={nslab}", errs, tol)
    print(f"   (oracle {t_ref:.1f} s, case {time.time() - t0:.1f} s)")
    _check(errs, tol, f"keep = {keep}")


# ------------------------------------------------------------------------------------------------ (c) edges
EDGE_L = [(512, "tile", None), (16384, "sp", None), (131072, "level", ((16,), 16384))]
EDGE_IDS = ["L512", "L16384", "L131072"]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("L,path,fac", EDGE_L, ids=EDGE_IDS)
def test_nothing_kept_is_exactly_zero(L, path, fac, dtype, monkeypatch):
    from flashfftconv import FrequencySparseFFTConv
    dev, _ = _to_gpu(*SI.white_inputs(L, L, 2, 2, seed=L), dtype)
    route = _SparseRoute(monkeypatch, L, L, path, fac)
    for n_partial in (0, 1):
        mod = FrequencySparseFFTConv(n_partial).to("cuda")
        got = _fwd_bwd(mod, *dev)
        route.expect(mod._convs[(2 * L, dtype)], 0)
        for nm, t in zip(SI.NAMES, got):
            assert bool(torch.isfinite(t).all()) and not bool(t.any()), f"N_partial = {n_partial}: {nm} has {int((t != 0).sum())} non-zero elements"


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("L,path,fac", EDGE_L, ids=EDGE_IDS)
def test_everything_kept_is_the_dense_convolution(L, path, fac, dtype, monkeypatch):
    """N_partial = N + 2 keeps all N / 2 + 1 rfft bins, Nyquist included: the oracle's full convolution, and FlashFFTConv's on the same inputs to REL / 4
    (its k_f comes from another call path: not bit-identical)"""
    from flashfftconv import FrequencySparseFFTConv, FlashFFTConv
    t0 = time.time()
    N, B, H = 2 * L, 2, 2
    dev, host = _to_gpu(*SI.white_inputs(L, L, B, H, seed=L + 1), dtype)
    want = O.ref_freq_sparse_conv(host[0], host[1], N + 2, host[2])
    full = (O.ref_fft_conv(host[0], host[1], N),) + tuple(O.ref_grads(host[0], host[1], host[2], N))
    for a, b in zip(want, full):      # (the oracle itself: a mask of ones)
        assert np.abs(a - b).max() < 1e-9
    route = _SparseRoute(monkeypatch, L, L, path, fac)
    tol = SI.gates(dtype)
    mod = FrequencySparseFFTConv(N + 2).to("cuda")
    got = _fwd_bwd(mod, *dev)
    route.expect(mod._convs[(N, dtype)], N // 2 + 1)
    errs = _errs(got, want)
    _line("c", L, L, path, fac, dtype, B, H, f"N_partial={N + 2} keep={N // 2 + 1}", errs, tol)
    dense = _fwd_bwd(FlashFFTConv(N, dtype=dtype).to("cuda"), *dev)
    agree = {nm: _row_rel(g.float(), d.double().cpu().numpy()) for nm, g, d in zip(SI.NAMES, got, dense)}
    quarter = {nm: SI.REL[dtype] / 4 for nm in SI.NAMES}
    _line("c", L, L, path, fac, dtype, B, H, "against FlashFFTConv", agree, quarter)
    print(f"   (case {time.time() - t0:.1f} s)")
    _check(errs, tol, "all bins kept")
    _check(agree, quarter, "against FlashFFTConv")


def test_one_module_caches_one_conv_per_size_and_dtype():
    from flashfftconv import FrequencySparseFFTConv
    keep = 37
    mod = FrequencySparseFFTConv(2 * keep).to("cuda")
    seen = {}
    for rnd in range(2):
        for L in (512, 16384):
            for dtype in (BF, FP):
                dev, host = _to_gpu(*SI.white_inputs(L, L, 2, 2, seed=L + rnd), dtype)
                got = _fwd_bwd(mod, *dev)
                conv = mod._convs[(2 * L, dtype)]
                assert seen.setdefault((2 * L, dtype), conv) is conv and conv.seqlen == 2 * L and conv.dtype == dtype and conv._kf_keep == keep
                _check(_errs(got, O.ref_freq_sparse_conv(host[0], host[1], 2 * keep, host[2])), SI.gates(dtype), f"L = {L}, {SI.DT_NAME[dtype]}, call {rnd}")
    assert set(mod._convs) == {(1024, BF), (1024, FP), (32768, BF), (32768, FP)}


def test_unsupported_inputs_raise():
    from flashfftconv import FrequencySparseFFTConv, PartialFFTConv
    for mod in (FrequencySparseFFTConv(64), PartialFFTConv(64)):
        with pytest.raises(NotImplementedError):
            mod(torch.randn(1, 1, 1000, device="cuda").to(BF), torch.randn(1, 1000, device="cuda"))
        with pytest.raises(RuntimeError):
            mod(torch.randn(1, 1, 512, device="cuda"), torch.randn(1, 512, device="cuda"))
        assert not mod._convs


# ------------------------------------------------------------------------------------------------ (d) PartialFFTConv
PARTIAL = [(256, "tile", None), (1024, "2pass", None), (16384, "sp", None), (32768, "multipass", None), (524288, "level", ((32,), 32768))]


def _partial_cases():
    out = [pytest.param(L, path, fac, dtype, torch.float32, id=f"L{L}-{SI.DT_NAME[dtype]}") for L, path, fac in PARTIAL for dtype in (BF, FP)]
    # a k that is itself bf16: once per family of call paths (one C-ABI call, fused size with k_f in front, HBM levels)
    return out + [pytest.param(L, path, fac, BF, BF, id=f"L{L}-bf16-kbf16") for L, path, fac in (PARTIAL[0], PARTIAL[2], PARTIAL[4])]


@pytest.mark.parametrize("L,path,fac,dtype,k_dtype", _partial_cases())
def test_partial_conv_against_the_oracle(L, path, fac, dtype, k_dtype, monkeypatch):
    """y = conv(x, k[..., :P]) at fft size 2 L for P = 1, 7, L - 1, L and a value above Lk; the module slices k[..., :P] itself, a non-contiguous view for P < Lk and H > 1; dk has k's
    shape and dtype with exact zeros beyond P.  Above fft 32768 P = 1 fits half the fft size: at fft 65536 the fitted 32768-point module must run."""
    from flashfftconv import PartialFFTConv
    t0 = time.time()
    N = 2 * L
    B, H = (2, 1) if N >= BIG_N else (3, 2)
    x, k, dout = SI.white_inputs(L, L, B, H, seed=3 * L + int(dtype == FP))
    (xg, kg, dg), host = _to_gpu(x, k, SI.tie_to(dout, x), dtype)
    kg = kg.to(k_dtype)
    taps = (1, 7, L - 1, L, L + 9)
    want = O.ref_partial_keeps(host[0], kg.double().cpu().numpy(), host[2], taps)
    t_ref = time.time() - t0
    route = _SparseRoute(monkeypatch, L, L, path, fac)
    tol = SI.gates(dtype)
    bad = []
    for P in taps:
        mod = PartialFFTConv(P).to("cuda")
        got = _fwd_bwd(mod, xg, kg, dg)
        conv = mod._convs[(N, dtype)]
        n_run = conv._fit_seqlen(L, min(P, L))
        if P == 1 and N > 32768:
            assert n_run == N // 2 and list(conv._fitted) == [N // 2] and conv._fitted[N // 2].seqlen == N // 2
            route.chosen.clear(); route.half.clear()
            assert route.rows == []
        else:
            assert n_run == N and not conv._fitted
            route.expect(conv, None)
        assert not bool(got[2][..., P:].any()), f"P = {P}: dk beyond the taps has {int((got[2][..., P:] != 0).sum())} non-zero elements"
        errs = _errs(got, want[P])
        _line("d", L, L, path, fac, dtype, B, H, f"P={P} k {str(k_dtype)[6:]} fft {n_run}", errs, tol)
        bad += [f"P = {P}: {nm} {v:.3e} >= {tol[nm]:.1e}" for nm, v in errs.items() if not v < tol[nm]]
    print(f"   (oracle {t_ref:.1f} s, case {time.time() - t0:.1f} s)")
    assert not bad, "rel-L2 of the worst row: " + "; ".join(bad)
