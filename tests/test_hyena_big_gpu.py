"""The fused Hyena / M2 operator on the HBM-level routes (fft >= 262144; flashfftconv/hyena.py _GatedSlicesBigFn): x1, x2, v are read as slices of uc
(B, 3D, L) and du, dpregate, dpostgate are written as slices of one d(uc), through the batch pitches of the level kernels (ffc_outer_pass*_strided).

One case per route, each asserting its route by what bigfft.choose and conv._big_half answered (as tests/test_sparse_gpu.py does).  Filters are as
long as L, so no smaller fft size fits.  Every case checks
 1. IN PLACE: every first-level forward call of _TorchOps.outer reads its input / gate inside uc's storage (or the incoming gradient dy), at the
    slice's offset and with uc's batch stride; every last-level inverse call of the backward writes a slice of the tensor returned as uc.grad; and no
    Tensor.contiguous() call copies anything.  (Without the feature the operator copies the three slices: this check fails.)
 2. BIT IDENTITY with the same module called on contiguous copies of the slices: y, uc.grad against the concatenation of the three gradients, dk
    (and dk_res) -- same kernels, same arithmetic, only addresses differ.
 3. for one case per dtype, the float64 oracle per (b, h) row with the gates and the input scaling of tests/test_half_rows_gpu.py (unit-scale
    inputs, k = 0.1 * randn; REL of the suite, x 1.5 gated, dk max(REL, 1e-2))."""
import os
import numpy as np
import pytest
import torch

from oracle import ref_fft_conv as O
from test_half_rows_gpu import _row_rel, _gates, NAMES

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float16

# id, B, D, L, fft size, (factors, inner size), half rows, dtype, fit_fft, options
CASES = [
    ("262144-B3", 3, 2, 131072, 262144, ((16,), 16384), False, BF, True, {"oracle": True}),
    ("262144-oddL", 2, 2, 100003, 262144, ((16,), 16384), False, FP, True, {"oracle": True}),      # element-wise path, unaligned slices
    ("1M-half", 1, 2, 524288, 1048576, ((32,), 32768), True, BF, True, {}),
    ("2M-64", 2, 1, 1048576, 2097152, ((64,), 32768), False, FP, True, {}),
    ("2M-32x65536", 2, 1, 1048584, 2097152, ((32,), 65536), False, BF, True, {}),
    ("4M-128-half", 1, 2, 1048576, 4194304, ((128,), 32768), True, BF, False, {}),                 # fit_fft off: the rows would fit 2097152 points
    ("4M-16x16", 2, 1, 1500000, 4194304, ((16, 16), 16384), False, FP, True, {}),
    ("2M-64-per-pass", 3, 1, 1048576, 2097152, ((64,), 32768), False, BF, True, {"env": {"FFC_BIG_ONE_LAUNCH": "0"}}),
    ("262144-k_res", 3, 2, 131072, 262144, ((16,), 16384), False, FP, True, {"k_res": True}),
    ("262144-eval-no_grad", 2, 2, 100003, 262144, ((16,), 16384), False, BF, True, {"eval": True}),
]


class _Spy:
    """records the route (bigfft.choose, conv._big_half), the long-side tensors of every level call (_TorchOps.outer) and every Tensor.contiguous()
    that copies"""

    def __init__(self, monkeypatch):
        from flashfftconv import bigfft, conv as C
        self.chosen, self.half, self.outer, self.copies = [], [], [], []
        choose, half, outer, contiguous = bigfft.choose, C._big_half, C._TorchOps.outer, torch.Tensor.contiguous

        def rec_choose(N, Lmax, ops=None):
            r = choose(N, Lmax, ops)
            self.chosen.append(r)
            return r

        def rec_half(mod, B, Lmax, f):
            r = half(mod, B, Lmax, f)
            self.half.append(r)
            return r

        def rec_outer(ops, dt, n0, fwd, inp, out, gate, bv, npair, Hin, mi, Llong, scale, lf32=None):
            desc = lambda t: None if t is None else (t.data_ptr(), t.stride(0), t.element_size())
            self.outer.append({"fwd": fwd, "Hin": Hin, "Llong": Llong, "lf32": lf32, "in": desc(inp), "out": desc(out), "gate": desc(gate)})
            return outer(ops, dt, n0, fwd, inp, out, gate, bv, npair, Hin, mi, Llong, scale, lf32)

        def rec_contiguous(t, *a, **kw):
            if not t.is_contiguous():
                self.copies.append(tuple(t.shape))
            return contiguous(t, *a, **kw)
        monkeypatch.setattr(bigfft, "choose", rec_choose)
        monkeypatch.setattr(C, "_big_half", rec_half)
        monkeypatch.setattr(C._TorchOps, "outer", rec_outer)
        monkeypatch.setattr(torch.Tensor, "contiguous", rec_contiguous)

    def clear(self):
        for l in (self.chosen, self.half, self.outer, self.copies):
            l.clear()

    def long_side(self, fwd, D, L, lo=0, hi=None):
        """the level calls lo .. hi that touch caller tensors: first forward level / last inverse level of the 16-bit rows (not the fp32 filter / dk rows)"""
        return [c for c in self.outer[lo:hi] if c["fwd"] == fwd and c["Hin"] == D and c["Llong"] == L and c["lf32"] is None]


def _slice_of(desc, t, D, L):
    """index j of the channel slice of t (B, 3D, L) that a recorded long-side tensor is (its pointer, and t's batch stride); None: not a slice of t"""
    if desc is None:
        return None
    ptr, stride0, es = desc
    off = ptr - t.data_ptr()
    if off < 0 or off % (D * L * es) or off // (D * L * es) > 2:
        return None
    return off // (D * L * es) if (t.shape[0] == 1 or stride0 == 3 * D * L) else None


def _outside(desc, t):
    """a recorded tensor that does not touch t's storage (the incoming gradient dy, an output of its own)"""
    return desc is not None and not (t.data_ptr() <= desc[0] < t.data_ptr() + t.numel() * t.element_size())


@pytest.mark.parametrize("cid,B,D,L,N,fac,half,dtype,fit,opt", CASES, ids=[c[0] for c in CASES])
def test_level_routes_read_and_write_the_slices_in_place(cid, B, D, L, N, fac, half, dtype, fit, opt, monkeypatch):
    from flashfftconv import FlashFFTConv, gated_conv_from_slices, conv as C
    torch.manual_seed(N + L + B)
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    conv.fit_fft = fit
    assert conv._fit_seqlen(L, L) == N
    evalmode, with_res = opt.get("eval", False), opt.get("k_res", False)
    if evalmode:
        conv.eval()
    uc = torch.randn(B, 3 * D, L, device="cuda").to(dtype)
    dy = torch.randn(B, D, L, device="cuda").to(dtype)
    k = torch.randn(D, L, device="cuda") * 0.1
    k_res = torch.randn(D, L, device="cuda") * 0.1 if with_res else None
    nres = 1 if with_res else 0
    env = opt.get("env", {})
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    C.reload_env()
    try:
        if env:
            assert C._ONE_LAUNCH_LEVEL is False
        spy = _Spy(monkeypatch)
        # ---- the operator: slices in place
        ul = uc.clone().requires_grad_(not evalmode)
        kl = k.clone().requires_grad_(not evalmode)
        krl = None if k_res is None else k_res.clone().requires_grad_(not evalmode)
        if evalmode:
            with torch.no_grad():
                y = gated_conv_from_slices(conv, ul, kl, krl)
            grads = ()
        else:
            y = gated_conv_from_slices(conv, ul, kl, krl)
            nfwd = len(spy.outer)
            grads = torch.autograd.grad(y, [ul, kl] + ([] if krl is None else [krl]), dy)
        assert spy.chosen and all(r == fac for r in spy.chosen), (spy.chosen, fac)
        assert spy.half and all(r == half for r in spy.half), (spy.half, half)
        assert spy.copies == [], f"contiguous() copied tensors of shape {spy.copies}"
        # 1. in place.  forward: conv(x1 * v, k) reads v (slice 2) gated by x1 (slice 0) [+ conv(v, k_res): v alone]; the last level writes y gated by x2 (slice 1)
        nfwd = len(spy.outer) if evalmode else nfwd
        first = spy.long_side(True, D, L, 0, nfwd)
        assert [(_slice_of(c["in"], ul, D, L), _slice_of(c["gate"], ul, D, L)) for c in first] == [(2, 0)] + [(2, None)] * nres, first
        last = spy.long_side(False, D, L, 0, nfwd)
        assert [_slice_of(c["gate"], ul, D, L) for c in last] == [1] + [None] * nres and all(_outside(c["out"], ul) for c in last), last
        if not with_res:
            assert last[0]["out"][0] == y.data_ptr()
        if not evalmode:
            duc = grads[0]
            assert duc.shape == ul.shape and duc.is_contiguous()
            # backward, first levels: dy gated by x2 (slice 1) [, v gated by x1 again where nothing was kept] [, dy and v for k_res]: whatever is not dy is a slice of uc
            first = spy.long_side(True, D, L, nfwd)
            for c in first:
                assert _outside(c["in"], ul) or _slice_of(c["in"], ul, D, L) == 2, c
                assert c["gate"] is None or _slice_of(c["gate"], ul, D, L) == (1 if _outside(c["in"], ul) else 0), c
            assert sum(1 for c in first if _outside(c["in"], ul) and c["gate"] is not None) == 1, first
            # backward, last levels: du -> slice 2 (gate x1), dpregate -> slice 0 (gate v), dpostgate -> slice 1 (gate dy) of uc.grad [, dv of k_res: a tensor of its own]
            last = spy.long_side(False, D, L, nfwd)
            assert len(last) == 3 + nres, last
            assert [_slice_of(c["out"], duc, D, L) for c in last[:3]] == [2, 0, 1], last
            assert [_slice_of(c["gate"], ul, D, L) for c in last[:2]] == [0, 2] and _outside(last[2]["gate"], ul), last
        in_place = (y,) + tuple(grads)
        # ---- the same module on contiguous copies of the slices
        spy.clear()
        monkeypatch.undo()
        leaves = [t.contiguous().requires_grad_(not evalmode) for t in uc.split(D, dim=1)]      # x1, x2, v
        kc = k.clone().requires_grad_(not evalmode)
        krc = None if k_res is None else k_res.clone().requires_grad_(not evalmode)
        with torch.set_grad_enabled(not evalmode):
            x1, x2, v = leaves
            yc = conv(v, kc, x1, x2) if krc is None else conv(v, kc, x1, x2, residual=conv(v, krc))
        ref = (yc,)
        if not evalmode:
            g = torch.autograd.grad(yc, leaves + [kc] + ([] if krc is None else [krc]), dy)
            ref += (torch.cat(g[:3], dim=1),) + tuple(g[3:])
        # 2. bit identity
        for nm, a, b in zip(("y", "uc.grad", "dk", "dk_res"), in_place, ref):
            assert a.shape == b.shape and a.dtype == b.dtype, nm
            assert torch.equal(a, b), f"{nm}: {int((a != b).sum())} of {a.numel()} elements differ from the run on contiguous copies"
        # 3. the float64 oracle, per (b, h) row
        if opt.get("oracle"):
            h = [t.double().cpu().numpy() for t in (uc[:, 2 * D:], k, dy, uc[:, :D], uc[:, D:2 * D])]      # v, k, dy, x1, x2
            want = (O.ref_fft_conv_gated(h[0], h[1], h[3], h[4], N),) + tuple(O.ref_grads(h[0], h[1], h[2], N, h[3], h[4]))
            duc = in_place[1]
            got = (in_place[0], duc[:, 2 * D:], in_place[2], duc[:, :D], duc[:, D:2 * D])
            tol = _gates(dtype, True)
            errs = {nm: _row_rel(a.contiguous(), w) for nm, a, w in zip(NAMES, got, want)}
            print(f"\nhyena_big {cid}: " + "  ".join(f"{nm} {e:.2e}" for nm, e in errs.items()))
            for nm, e in errs.items():
                assert e < tol[nm], f"{nm}: rel-L2 of the worst (b, h) row {e:.3e} >= {tol[nm]:.1e}"
    finally:
        for n, v_ in old.items():
            if v_ is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v_
        C.reload_env()
