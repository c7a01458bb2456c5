"""Half-height phase C of fft 32768 at L <= N/2 (csrc/ffc_body.h Body::outer_inv_half) on the GPU: forward + backward through the module,
spectrum-saving and recomputing, both dtypes -- against the torch.fft oracle, against the earlier stages (tuning flag 256), and the two sinks
against each other (plain rows take the direct store; all-ones gates and a zero residual take E + rows_out and must give the same bits)."""
import pytest
import torch

from oracle.torch_ref import ref_fft_conv
from tests.test_flashfftconv_gpu import rel, stable, REL

pytestmark = pytest.mark.gpu
N = 32768
# (B, H, L): all 16 rows live; odd batch (missing partner row); a partly filled row; last chunk short; one row and one chunk; exactly 15 rows
SHAPES = [(2, 2, 16384), (3, 2, 16384), (2, 3, 8200), (2, 2, 16376), (2, 2, 1032), (4, 1, 15360)]
_REF = {}


def inputs(B, H, L, dtype):
    g = torch.Generator(device="cuda").manual_seed(B * 100003 + H * 1009 + L)
    u = torch.randn(B, H, L, device="cuda", generator=g).to(dtype)
    k = torch.randn(H, L, device="cuda", generator=g) * torch.exp(-0.01 * torch.arange(L, device="cuda")) / 4
    dout = torch.randn(B, H, L, device="cuda", generator=g).to(dtype)
    return u, k, dout


def reference(B, H, L, dtype):
    """y, du, dk of the torch.fft oracle, computed once per shape and dtype"""
    key = (B, H, L, dtype)
    if key not in _REF:
        u, k, dout = inputs(B, H, L, dtype)
        uc, kc = u.clone().requires_grad_(True), k.clone().requires_grad_(True)

        def run():
            y = ref_fft_conv(uc, kc, n=N)
            return (y.detach(),) + tuple(torch.autograd.grad(y, (uc, kc), dout))
        _REF[key] = stable(run, "fft 32768 reference")
    return _REF[key]


def run_module(B, H, L, dtype, save, gates=False, residual=False):
    from flashfftconv import FlashFFTConv
    u, k, dout = inputs(B, H, L, dtype)
    u.requires_grad_(True); k.requires_grad_(True)
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    conv.save_spectrum = save
    ones = torch.ones_like(u) if gates else None
    res = torch.zeros_like(u) if residual else None
    y = conv(u, k, ones, ones, res) if (gates or residual) else conv(u, k)
    du, dk = torch.autograd.grad(y, (u, k), dout)
    torch.cuda.synchronize()
    return y.detach(), du, dk


def check_against_oracle(got, ref, dtype):
    for name, a, b, tol in zip(("y", "du", "dk"), got, ref, (REL[dtype], REL[dtype], max(REL[dtype], 1e-2))):
        e = rel(a, b)
        print(f"{name} rel-L2 {e:.3e} (gate {tol:.1e})")
        assert e < tol, f"{name} rel-L2 {e:.3e}"


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_against_oracle_and_between_sinks(B, H, L, save, dtype, monkeypatch):
    from flashfftconv import conv as C
    ref = reference(B, H, L, dtype)
    plain = run_module(B, H, L, dtype, save)
    check_against_oracle(plain, ref, dtype)
    # the same call through E + rows_out: all-ones gates (a product with 1.0 is exact), a zero residual (so is a sum with 0)
    gated = run_module(B, H, L, dtype, save, gates=True)
    resid = run_module(B, H, L, dtype, save, residual=True)
    for name, a, b, c in zip(("y", "du"), plain, gated, resid):
        assert torch.equal(a, b), f"{name}: plain != unit gates, {int((a != b).sum())} elements"
        assert torch.equal(a, c), f"{name}: plain != zero residual, {int((a != c).sum())} elements"
    # the earlier stages (tuning flag 256, read when a plan is built): same result to the dtype's tolerance
    monkeypatch.setenv("FFC_FLAGS", "256"); C.reload_env()
    try:
        old = run_module(B, H, L, dtype, save)
    finally:
        monkeypatch.delenv("FFC_FLAGS"); C.reload_env()
    check_against_oracle(old, ref, dtype)
    for name, a, b, tol in zip(("y", "du", "dk"), plain, old, (REL[dtype], REL[dtype], max(REL[dtype], 1e-2))):
        assert rel(a, b) < tol, f"{name}: default vs flag 256 rel-L2 {rel(a, b):.3e}"


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
def test_ragged_length_falls_back(save):
    """L % 8 != 0: element-wise rows, which the direct store does not take"""
    B, H, L, dtype = 2, 2, 8198, torch.bfloat16
    check_against_oracle(run_module(B, H, L, dtype, save), reference(B, H, L, dtype), dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_batch_strided_rows(dtype):
    """u and y as channel slices of wider (B, C, L) tensors (batch stride C * L): the direct store honours the output's batch stride and
    leaves the neighbouring channels alone; same bits as the contiguous call"""
    from flashfftconv import FlashFFTConv, conv as C, _lib
    lib, P, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr
    B, H, L, Cw = 3, 2, 8200, 5
    u, k, _ = inputs(B, H, L, dtype)
    plan = FlashFFTConv(N, dtype=dtype).cuda()._get_plan(u.device)
    kf = C._kernel_fft(plan, k)
    y0 = torch.full_like(u, 7.0)
    _lib.check(lib.ffc_conv_fwd(plan.handle, P(u), P(kf), None, None, P(y0), B, H, L, 0, sp()), "fwd")
    wide_u = torch.full((B, Cw, L), float("nan"), dtype=dtype, device="cuda"); wide_y = torch.full((B, Cw, L), 5.0, dtype=dtype, device="cuda")
    wide_u[:, 1:1 + H] = u
    us, ys = wide_u[:, 1:1 + H], wide_y[:, 2:2 + H]
    _lib.check(lib.ffc_conv_fwd_strided(plan.handle, P(us), P(kf), None, None, P(ys), B, H, L, 0, Cw * L, 0, 0, Cw * L, sp()), "fwd strided")
    torch.cuda.synchronize()
    assert torch.equal(ys, y0)
    assert bool((wide_y[:, :2] == 5.0).all()) and bool((wide_y[:, 2 + H:] == 5.0).all()), "the strided store touched another channel"
    yr, _, _ = reference(B, H, L, dtype)
    assert rel(y0, yr) < REL[dtype]
