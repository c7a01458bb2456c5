"""Every fused fft size (256 .. 32768 in one launch, 65536 / 131072 in two / four passes) through FlashFFTConv, checked per (b, h) row and per
element against the numpy float64 oracle on the CPU (tests/rowcheck.py: tied heads, per row, per element), at unit scale with a filter that
does not decay, both dtypes, plain and gated (random unit-scale gates), one residual case per size.

Each case runs forward + backward with the spectra kept, the same recomputing them, and the forward under no_grad, and applies the three
assertions to every result (a result that is bit-equal to one already checked passes by identity).

Lengths per size: N / 2 (the half form where there is an outer digit), N / 2 + 8 (the first length past the half boundary; at 65536 / 131072 that
boundary is 16384: 16384 and 16392 as well), N, N / 2 - 3 (ragged: the element-wise row paths; its gated case has a 37-tap filter), and at fft
32768 L = 1032, where whole store instructions of phase C have no active lane.

Two widths per (size, length), told apart by the number of fp32 dk_f slabs (csrc/ffc_dev.h ffc_choose_chunks), which is asserted:
  narrow  H = 3, an odd batch (a lone last row) large enough for more than one chunk: the pairs are spread over the workgroups, k -> k_f and
          dk_f -> dk are launches of their own and dk_f is summed from several slabs.  B = 5 does that where a workgroup takes one or two pairs
          per iteration (fft >= 16384); below, the smallest odd batch with a second chunk: 9 at fft 8192, 17 at 4096 / 2048 / 1024 and on the
          HBM-level route of fft 131072 beyond L = 65536, 33 at 512, 65 at 256.  The oracle sees all three heads.
  wide    H = twice the workgroup slots of the card (four workgroups per CU and 8 more at the single-tile sizes, whose kernels are persistent
          with two workgroups per CU; two per CU above), tiled from 8 representative heads: one chunk, one slab, every workgroup owns all pairs
          of its head(s) and its pair loop takes a back edge on the way to each row the oracle sees -- 9 pairs at fft 4096 (8 per iteration),
          5 at 8192 (4), 3 at 16384 (2), 3 above (1).  The loop's steady state, the rotated prefetch, the in-launch k -> k_f and the dk tail
          all run here.
fft 32768: the wide plain cases at L = 16384 and 8200 also under tuning flags 512 (the kernels with the run-time arms) and 256 (full-height
phase C), each against the oracle on its own; and the input gate alone through the C entry points (the form with a gate and plain output rows).

The gates are the suite's own and none is tuned to what these kernels give; profiles/fused_rows_parity.txt holds the measured figures."""
import collections
import math
import time

import pytest
import torch

import rowcheck as RC
from test_flashfftconv_gpu import REL, rel

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072]
BF, FP = torch.bfloat16, torch.float16
DT_NAME = {BF: "bf16", FP: "fp16"}
WIDE_B = {4096: 17, 8192: 9}        # odd, two iterations of the pair loop; every other size: 5
_ORACLE = collections.OrderedDict()   # (N, L, Lk, B, heads, dtype, gated, residual) -> rowcheck.Want, at most _ORACLE_BYTES of them
_ORACLE_BYTES = 1 << 30


def lengths(N):
    return [N // 2, N // 2 + 8, N, N // 2 - 3] + ([16384, 16392] if N >= 65536 else []) + ([1032] if N == 32768 else [])


def _slabs(conv, N, B, H, Lmax):
    """fp32 dk_f slabs of this call's backward; on the HBM-level route (fft 131072 beyond L = 65536) the inner plan's count for the pair-plane rows"""
    from flashfftconv import _lib, bigfft, conv as C
    dev = torch.device("cuda", torch.cuda.current_device())
    if conv._route_big(Lmax):
        fac = bigfft.choose(N, Lmax, C._TorchOps)
        return _lib.lib().ffc_dkf_slab_count(conv._get_plan(dev, fac[1]).handle, 2 * ((B + 1) // 2), H * math.prod(fac[0]))
    return _lib.lib().ffc_dkf_slab_count(conv._get_plan(dev).handle, B, H)


def _shape(conv, N, width, Lmax):
    """(B, H) of the case and the assertion that it runs the route its width names"""
    if width == "narrow":
        B, H = 5, 3
        while _slabs(conv, N, B, H, Lmax) <= 1 and B < 65:
            B += 2
        assert _slabs(conv, N, B, H, Lmax) > 1, (N, B, H)
        return B, H
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, H = WIDE_B.get(N, 5), (4 * cus + 8 if N <= 2048 else 2 * cus)
    assert _slabs(conv, N, B, H, Lmax) == 1, (N, B, H)
    return B, H


def _inputs(N, L, Lk, B, heads, dtype, gated, residual):
    """the representative heads' inputs, on the GPU: (u, k, dout, pregate, postgate, residual), the last three None where absent"""
    g = torch.Generator(device="cuda").manual_seed(N * 7 + L * 1009 + Lk * 31 + B * 3 + heads + 2 * int(gated) + int(dtype == FP) + 4 * int(residual))
    mk = lambda: torch.randn(B, heads, L, device="cuda", generator=g).to(dtype)
    u, dout = mk(), mk()
    k = torch.randn(heads, Lk, device="cuda", generator=g) * 0.1
    pre, post = (mk(), mk()) if gated else (None, None)
    return u, k, dout, pre, post, (mk() if residual else None)


def _want(key, rep):
    """the float64 oracle on the representative heads, once per case shape"""
    if key in _ORACLE:
        _ORACLE.move_to_end(key)
        return _ORACLE[key], 0.0
    t0 = time.time()
    u, k, dout, pre, post, res = (None if t is None else t.double().cpu().numpy() for t in rep)
    want = RC.oracle(u, k, dout, key[0], pre, post, res)
    _ORACLE[key] = want
    while len(_ORACLE) > 1 and sum(w.nbytes() for w in _ORACLE.values()) > _ORACLE_BYTES:
        _ORACLE.popitem(last=False)
    return want, time.time() - t0


class _Checked:
    """applies the three assertions to every result of a case; a tensor bit-equal to one that passed under the same name has passed them too"""

    def __init__(self, want, pi, dtype, gated):
        self.want, self.pi, self.dtype, self.gated = want, pi, dtype, gated
        self.seen, self.reports = {}, {}

    def __call__(self, what, got):
        fresh = {nm: t for nm, t in got.items() if not any(torch.equal(t, s) for s in self.seen.get(nm, ()))}
        rep = RC.check(fresh, self.want, self.pi, self.dtype, self.gated)
        self.reports[what] = rep
        rep.assert_ok(what)
        for nm, t in fresh.items():
            self.seen.setdefault(nm, []).append(t)
        return rep

    def worst(self):
        out = RC.Report()
        for rep in self.reports.values():
            for nm in rep.row:
                out.row[nm], out.elem[nm] = max(out.row.get(nm, 0.0), rep.row[nm]), max(out.elem.get(nm, 0.0), rep.elem[nm])
        return out


def run_case(N, L, width, dtype, gated, residual=False, tag=""):
    from flashfftconv import FlashFFTConv
    t0 = time.time()
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    conv.fit_fft = False              # fft 65536 / 131072 at L = 16384 would otherwise run fft 32768
    Lk = 37 if (gated and L == N // 2 - 3) else L
    B, H = _shape(conv, N, width, L)
    pi = RC.head_map(H, seed=N + L)
    heads = min(H, RC.P)
    rep = _inputs(N, L, Lk, B, heads, dtype, gated, residual)
    want, t_ref = _want((N, L, Lk, B, heads, dtype, gated, residual), rep)
    u, k, dout, pre, post, res = (None if t is None else RC.tile(t, pi, 0 if t.dim() == 2 else 1) for t in rep)
    fwd = lambda lv: conv(lv[0], lv[1], lv[2] if gated else None, lv[3] if gated else None, res)
    checked = _Checked(want, pi, dtype, gated)
    names = ("du", "dk") + (("dpregate", "dpostgate") if gated else ())
    ys = {}
    for what, save in (("spectra kept", True), ("recomputed", False)):
        conv.save_spectrum = save
        leaves = [t.detach().requires_grad_(True) for t in (u, k) + ((pre, post) if gated else ())]
        y = fwd(leaves)
        grads = torch.autograd.grad(y, leaves, dout)
        ys[what] = y.detach()
        checked(what, dict(zip(("y",) + names, (ys[what],) + tuple(grads))))
        del y, grads, leaves
    with torch.no_grad():
        y_n = fwd((u, k, pre, post))
    checked("no_grad", {"y": y_n})
    for what, y in ys.items():
        # without a graph no spectra are stored (another kernel variant): the same output bit for bit where an outer digit exists, to
        # last-bit steps at fft <= 2048 (tests/test_flashfftconv_gpu.py run_case)
        if N >= 4096:
            assert torch.equal(y_n, y), f"forward under no_grad against '{what}': {int((y_n != y).sum())} elements differ"
        else:
            assert rel(y_n, y) < REL[dtype] / 4, f"forward under no_grad against '{what}': rel {rel(y_n, y):.3e}"
    torch.cuda.synchronize()
    print(f"\nfused_rows N={N} L={L} Lk={Lk} {width} B={B} H={H} {DT_NAME[dtype]} {'gated' if gated else 'plain'}{' residual' if residual else ''}{tag}: "
          f"{checked.worst().line()}  (worst row rel-L2 / worst element |err| / bound; oracle {t_ref:.1f} s, case {time.time() - t0:.1f} s)")


MATRIX = [pytest.param(N, L, width, dtype, gated, id=f"{N}-L{L}-{width}-{DT_NAME[dtype]}-{'gated' if gated else 'plain'}")
          for N in SIZES for L in lengths(N) for width in ("narrow", "wide") for dtype in (BF, FP) for gated in (False, True)]


@pytest.mark.parametrize("N,L,width,dtype,gated", MATRIX)
def test_rows_and_elements(N, L, width, dtype, gated):
    run_case(N, L, width, dtype, gated)


@pytest.mark.parametrize("N,dtype", [(N, (BF, FP)[i % 2]) for i, N in enumerate(SIZES)], ids=[f"{N}-{('bf16', 'fp16')[i % 2]}" for i, N in enumerate(SIZES)])
def test_residual(N, dtype):
    """y = postgate * conv(u * pregate, k) + residual, added in the kernel's output epilogue: the oracle's y plus the residual in float64; wide, gated, L = N / 2"""
    run_case(N, N // 2, "wide", dtype, True, residual=True)


@pytest.mark.parametrize("flags", [512, 256])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("L", [16384, 8200])
def test_fft32768_tuning_flags(L, dtype, flags, monkeypatch):
    """the kernels with the run-time arms (512) and full-height phase C (256) in the looping regime, each against the oracle on its own"""
    from flashfftconv import FlashFFTConv, conv as C
    FlashFFTConv(32768, dtype=dtype).to("cuda")._get_plan(torch.device("cuda", torch.cuda.current_device()))
    monkeypatch.setenv("FFC_FLAGS", str(flags)); C.reload_env()      # (tuning flags are read when a plan is built or reloaded)
    try:
        run_case(32768, L, "wide", dtype, False, tag=f" FFC_FLAGS={flags}")
    finally:
        monkeypatch.delenv("FFC_FLAGS"); C.reload_env()


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_fft32768_input_gate_alone(dtype, save):
    """a random input gate alone through the C entry points (forward: pregate, backward: postgate; the output rows stay plain), wide:
    y = conv(u * pregate, k); du and dk are those of the plain call on dout * postgate.  The noise of each row is that of a plain row; the
    gates are the gated ones (x 1.5: a rounded product in front of the transform)"""
    from flashfftconv import FlashFFTConv, conv as C
    from oracle import ref_fft_conv as O
    from test_plain_rows_gpu import raw_step
    N, L = 32768, 16384
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    B, H = _shape(conv, N, "wide", L)
    pi = RC.head_map(H, seed=N + L + 1)
    rep = _inputs(N, L, L, B, RC.P, dtype, True, False)
    u, k, dout, pre, post = (t.double().cpu().numpy() for t in rep[:5])
    y = O.ref_fft_conv(u * pre, k, N)
    du, dk = O.ref_grads(u, k, dout * post, N)
    want = RC.Want({"y": y, "du": du, "dk": dk}, {"y": RC.rms(y), "du": RC.rms(du), "dk": RC.rms(dk)})
    tu, tk, tdout, tpre, tpost = (RC.tile(t, pi, 0 if t.dim() == 2 else 1) for t in rep[:5])
    plan = conv._get_plan(tu.device)
    kf = C._kernel_fft(plan, tk)
    y_g, _, _ = raw_step(plan, kf, tu, tdout, save, pre=tpre)
    _, du_g, dk_g = raw_step(plan, kf, tu, tdout, save, post=tpost)
    r = RC.check({"y": y_g, "du": du_g, "dk": dk_g}, want, pi, dtype, True)
    print(f"\nfused_rows N={N} L={L} wide B={B} H={H} {DT_NAME[dtype]} input gate alone, {'spectra kept' if save else 'recomputed'}: {r.line()}")
    r.assert_ok("input gate alone")
