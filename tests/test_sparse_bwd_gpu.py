"""Frequency-sparse backward on the GPU: ffc_conv_bwd_sparse + ffc_kernel_ifft_grad_sp directly (NaN-filled workspace) and through FrequencySparseFFTConv,
per (b, h) row against the float64 definition with the masked k_f, evaluated on the inputs as rounded to the module dtype.  Inputs: the tone recipe of
tests/sparse_inputs.py, the tone on the last kept bin.  Gates: those of tests/test_sparse_gpu.py (sparse_inputs.gates; the gate gradients take the
gate of out / dx).  B = 3: the last pair is half empty; H = 3: several dk_f slabs (tests/test_fused_rows_gpu.py)."""
import ctypes
import numpy as np
import pytest
import torch

from oracle import ref_fft_conv as O
import sparse_inputs as SI
from test_half_rows_gpu import _row_rel

pytestmark = pytest.mark.gpu
B, H = 3, 3
KEEPS = [lambda N: N // 32, lambda N: N // 32 + 1, lambda N: 3 * N // 32 + 5, lambda N: 4 * N // 32]      # rows 1, 2, 4 (edge inside the row), 4 (full)
DTS = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]


def _setup(N, keep, dtype, gated):
    """device inputs (x, k fp32, dout, pregate, postgate) and the oracle's {out, dx, dk, dpre, dpost}"""
    L = N // 2
    x, k, dout = SI.tone_inputs(L, L, B, H, keep - 1, seed=N + keep + int(gated))
    rng = np.random.default_rng(keep)
    gates = [rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(2)] if gated else [None, None]
    dev = [None if t is None else torch.from_numpy(t).to("cuda").to(dtype) for t in (x, dout, *gates)]
    kg = torch.from_numpy(k).to("cuda")
    xh, dh, g1, g2 = (None if t is None else t.double().cpu().numpy() for t in dev)
    rnd = lambda a: O.round_to(a, SI.DT_NAME[dtype])
    f = np.arange(N)
    live = (f < keep) | (f > N - keep)
    kf = np.fft.fft(k.astype(np.float64), n=N) * live
    v, dc = (rnd(xh * g1), rnd(dh * g2)) if gated else (xh, dh)
    vf, df = np.fft.fft(v, n=N), np.fft.fft(dc, n=N)
    conv, dv = np.fft.ifft(vf * kf, n=N).real[..., :L], np.fft.ifft(df * np.conj(kf), n=N).real[..., :L]
    want = {"out": conv * g2 if gated else conv, "dx": dv * g1 if gated else dv, "dk": np.fft.ifft((df * np.conj(vf)).sum(0) * live).real[:, :L]}
    if gated:
        want.update(dpre=dv * xh, dpost=rnd(conv) * dh)
    return (dev[0], kg, dev[1], dev[2], dev[3]), want


def _check(got, want, dtype, what):
    tol = dict(SI.gates(dtype), dpre=SI.REL[dtype], dpost=SI.REL[dtype])
    errs = {nm: _row_rel(got[nm].float(), want[nm]) for nm in got}
    print(f"\nsparse_bwd {what}: " + "  ".join(f"{nm} {e:.2e}" for nm, e in errs.items()), end="")
    for nm, e in errs.items():
        assert e < tol[nm], f"{what}: {nm} rel-L2 of the worst row {e:.3e} >= {tol[nm]:.1e}"


def _conv(N, keep, dtype):
    from flashfftconv import FrequencySparseFFTConv
    mod = FrequencySparseFFTConv(2 * keep).to("cuda")
    return mod._conv_for(torch.empty(1, 1, N // 2, dtype=dtype, device="cuda"), keep=keep)


def _module_run(N, keep, dtype, x, k, dout, g1, g2):
    """FrequencySparseFFTConv's public forward; gated: its FlashFFTConv (the public forward takes no gates)"""
    from flashfftconv import FrequencySparseFFTConv
    conv = FrequencySparseFFTConv(2 * keep).to("cuda") if g1 is None else _conv(N, keep, dtype)
    leaves = [t.clone().requires_grad_(True) for t in (x, k) + ((g1, g2) if g1 is not None else ())]
    y = conv(leaves[0], leaves[1], *leaves[2:])
    grads = torch.autograd.grad(y, leaves, dout)
    return dict(zip(("out", "dx", "dk", "dpre", "dpost"), (y.detach(),) + grads))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("N", [16384, 32768])
def test_c_abi_on_a_nan_workspace(N, dtype, gated):
    from flashfftconv import conv as C, _lib
    keep, rows, L = 3 * N // 32 + 5, 4, N // 2
    (x, k, dout, g1, g2), want = _setup(N, keep, dtype, gated)
    cv = _conv(N, keep, dtype)
    plan = cv._get_plan(x.device)
    kf = C._kernel_fft(plan, k)
    kf.mul_(cv._kf_mask(plan, kf.dtype)[None, :, None])
    ws = torch.full((C._ws_bytes(plan, B, H) // 4,), float("nan"), device="cuda")
    du, dpre, dpost = (torch.empty_like(x) if (gated or i == 0) else None for i in range(3))
    lib, P = _lib.lib(), _lib.ptr
    _lib.check(lib.ffc_conv_bwd_sparse(plan.handle, P(dout), P(x), P(kf), P(g1), P(g2), P(du), P(dpre), P(dpost), P(ws), None, B, H, L, rows,
                                       _lib.stream_ptr()), "ffc_conv_bwd_sparse")
    dk = torch.full((H, L), float("nan"), device="cuda")
    _lib.check(lib.ffc_kernel_ifft_grad_sp(plan.handle, P(ws), P(cv._kf_mask(plan, torch.float32)), rows, B, H, L, P(dk), _lib.stream_ptr()),
               "ffc_kernel_ifft_grad_sp")
    nslab = lib.ffc_dkf_slab_count(plan.handle, B, H)
    slabs = ws[: nslab * H * plan.kf_elems * 2].view(nslab, H, plan.kf_elems // 1024, 8, 256)      # [slab][head][tile][spectrum row][...]
    assert bool(torch.isfinite(slabs[:, :, :, [0, 7]]).all()) and bool(torch.isnan(slabs[:, :, :, 1:7]).all()), "live rows written, dead rows untouched"
    assert bool(torch.isfinite(dk).all())
    got = dict(dx=du, dk=dk, **({"dpre": dpre, "dpost": dpost} if gated else {}))
    _check(got, want, dtype, f"C-ABI fft{N} {SI.DT_NAME[dtype]} gated={gated} slabs={nslab}")


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("ki", range(5), ids=["rows1", "rows2", "rows4-edge", "rows4", "dense"])
@pytest.mark.parametrize("N", [16384, 32768])
def test_module_takes_the_sparse_backward(N, ki, dtype, gated, monkeypatch):
    from flashfftconv import conv as C
    keep = KEEPS[ki](N) if ki < 4 else 4 * N // 32 + 1
    dev, want = _setup(N, keep, dtype, gated)
    calls, real = [], C._bwd_sparse
    monkeypatch.setattr(C, "_bwd_sparse", lambda plan, *a: (calls.append((plan.seqlen, a[5])), real(plan, *a))[1])
    got = _module_run(N, keep, dtype, *dev)
    rows = -(-keep // (N // 32))
    assert calls == ([(N, rows)] if ki < 4 else []), calls
    _check(got, want, dtype, f"module fft{N} keep={keep} {SI.DT_NAME[dtype]} gated={gated}")


@pytest.mark.parametrize("N", [16384, 32768])
def test_against_the_dense_backward_in_one_process(N, monkeypatch):
    from flashfftconv import conv as C
    keep, dtype = 3 * N // 32 + 5, torch.bfloat16
    dev, want = _setup(N, keep, dtype, True)
    got = {}
    try:
        for flag in ("0", "1"):
            monkeypatch.setenv("FFC_SPARSE_BWD", flag)
            C.reload_env()
            got[flag] = _module_run(N, keep, dtype, *dev)
            _check(got[flag], want, dtype, f"FFC_SPARSE_BWD={flag} fft{N}")
    finally:
        monkeypatch.delenv("FFC_SPARSE_BWD")
        C.reload_env()
    dist = {nm: float((got["1"][nm].double() - got["0"][nm].double()).norm() / got["0"][nm].double().norm()) for nm in ("dx", "dk")}
    print(f"\nsparse_bwd A/B fft{N}: relative distance sparse - dense  dx {dist['dx']:.2e}  dk {dist['dk']:.2e}", end="")


def test_refusals_leave_du_untouched():
    from flashfftconv import conv as C, _lib
    lib, P = _lib.lib(), _lib.ptr

    def call(N, rows, zin=False):
        L = N // 2
        plan = C.get_plan(N, torch.bfloat16, "cuda")
        x = torch.randn(B, H, L, device="cuda").to(torch.bfloat16)
        kf = torch.zeros(H, plan.kf_elems, 2, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(C._ws_bytes(plan, B, H), dtype=torch.uint8, device="cuda")
        du = torch.full_like(x, 7.0)
        rc = lib.ffc_conv_bwd_sparse(plan.handle, P(x), P(x), P(kf), None, None, P(du), None, None, P(ws), P(ws) if zin else None, B, H, L, rows,
                                     _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and lib.ffc_last_error() and bool((du == 7.0).all()), (N, rows, zin, rc)
    call(8192, 2); call(16384, 0); call(16384, 5); call(32768, 2, zin=True)
