"""Plain-row kernels of fft 32768 at L <= N/2 (csrc/ffc_route.h plain_rows_ok: the direct-store kernels without the gate, side-product and
element-wise arms on the input side) on the GPU: the default route against tuning flag 512 (the kernels with the run-time arms) bit for
bit and against the torch.fft oracle, and the calls that must fall back to the general kernels -- a ragged length, an input gate, a
misaligned base -- plus batch-strided rows.  Nothing arithmetic differs between the variants, so equality of the bits is the gate."""
import pytest
import torch

from tests.test_flashfftconv_gpu import rel, REL
from tests.test_phase_c_half_gpu import N, SHAPES, inputs, reference, run_module, check_against_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,L", SHAPES)
@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_default_bit_identical_to_flag_512(B, H, L, save, dtype, monkeypatch):
    from flashfftconv import conv as C
    new = run_module(B, H, L, dtype, save)
    check_against_oracle(new, reference(B, H, L, dtype), dtype)
    monkeypatch.setenv("FFC_FLAGS", "512"); C.reload_env()      # (tuning flags are read when a plan is built or reloaded)
    try:
        old = run_module(B, H, L, dtype, save)
    finally:
        monkeypatch.delenv("FFC_FLAGS"); C.reload_env()
    for name, a, b in zip(("y", "du", "dk"), new, old):
        assert torch.equal(a, b), f"{name}: default != flag 512, {int((a != b).sum())} elements"


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
def test_ragged_length_falls_back(save):
    """L % 8 != 0: element-wise rows, the general kernels"""
    B, H, L, dtype = 2, 2, 8198, torch.bfloat16
    check_against_oracle(run_module(B, H, L, dtype, save), reference(B, H, L, dtype), dtype)


def raw_step(plan, kf, u, dout, save, y=None, du=None, pre=None, post=None, sb_u=0, sb_y=0, sb_dout=0, sb_du=0):
    """forward (+ spectra) and fused backward through the C ABI: y, du into the given tensors (batch strides in elements, 0 = contiguous),
    pre: the forward's input gate alone, post: the backward's input gate alone; returns (y, du, dk)"""
    from flashfftconv import _lib
    lib, P, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr
    B, H, L = u.shape
    y = torch.empty(B, H, L, dtype=u.dtype, device="cuda") if y is None else y
    du = torch.empty(B, H, L, dtype=u.dtype, device="cuda") if du is None else du
    z = torch.empty(lib.ffc_spectrum_bytes(plan.handle, B, H), dtype=torch.uint8, device="cuda") if save else None
    if save:
        _lib.check(lib.ffc_conv_fwd_z(plan.handle, P(u), P(kf), P(pre), None, P(y), P(z), None, B, H, L, sb_u, 0, 0, sb_y, sp()), "fwd_z")
    else:
        _lib.check(lib.ffc_conv_fwd_strided(plan.handle, P(u), P(kf), P(pre), None, P(y), B, H, L, 0, sb_u, 0, 0, sb_y, sp()), "fwd")
    ws = torch.empty(lib.ffc_dkf_workspace_bytes(plan.handle, B, H), dtype=torch.uint8, device="cuda")
    if save:
        _lib.check(lib.ffc_conv_bwd_z(plan.handle, P(dout), P(u), P(kf), None, P(post), P(du), None, None, P(ws), P(z), B, H, L,
                                      sb_dout, sb_u, 0, 0, sb_du, 0, 0, sp()), "bwd_z")
    else:
        _lib.check(lib.ffc_conv_bwd_gated_strided(plan.handle, P(dout), P(u), P(kf), None, P(post), P(du), None, None, P(ws), B, H, L,
                                                  sb_dout, sb_u, 0, 0, sb_du, 0, 0, sp()), "bwd")
    dk = torch.empty(H, L, dtype=torch.float32, device="cuda")
    _lib.check(lib.ffc_kernel_ifft_grad(plan.handle, P(ws), B, H, L, P(dk), sp()), "ifft_grad")
    torch.cuda.synchronize()
    return y, du, dk


def setup(B, H, L, dtype):
    from flashfftconv import FlashFFTConv, conv as C
    u, k, dout = inputs(B, H, L, dtype)
    plan = FlashFFTConv(N, dtype=dtype).cuda()._get_plan(u.device)
    return plan, C._kernel_fft(plan, k), u, dout


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_input_gate_alone_and_misaligned_base_fall_back(save, dtype):
    """an all-ones input gate alone (forward: pregate, backward: postgate; the output rows stay plain) takes the direct-store kernels with
    the run-time arms, a base that is not 16-byte aligned the element-wise rows: a product with 1.0 is exact and the rows carry the same
    values, so both give the bits of the plain call"""
    B, H, L = 3, 2, 8200
    plan, kf, u, dout = setup(B, H, L, dtype)
    plain = raw_step(plan, kf, u, dout, save)
    ref = reference(B, H, L, dtype)
    assert rel(plain[0], ref[0]) < REL[dtype] and rel(plain[1], ref[1]) < REL[dtype] and rel(plain[2], ref[2]) < max(REL[dtype], 1e-2)
    ones = torch.ones_like(u)
    y_g, _, _ = raw_step(plan, kf, u, dout, save, pre=ones)
    assert torch.equal(y_g, plain[0]), "forward with an all-ones pregate alone"
    _, du_g, dk_g = raw_step(plan, kf, u, dout, save, post=ones)
    assert torch.equal(du_g, plain[1]) and torch.equal(dk_g, plain[2]), "backward with an all-ones postgate alone"

    def shifted(t):      # the same values in a view that starts one element (2 bytes) into its storage
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2
        return v
    y_m, du_m, dk_m = raw_step(plan, kf, shifted(u), shifted(dout), save)
    assert torch.equal(y_m, plain[0]) and torch.equal(du_m, plain[1]) and torch.equal(dk_m, plain[2]), "misaligned u / dout"


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_batch_strided_rows(save, dtype):
    """u, dout, y and du as channel slices of wider (B, 5, L) tensors (batch stride 5 L), the inputs' other channels NaN: the plain-row
    kernels keep the batch strides as run-time values -- same bits as the contiguous call, the outputs' neighbouring channels untouched"""
    B, H, L, Cw = 3, 2, 8200, 5
    plan, kf, u, dout = setup(B, H, L, dtype)
    y0, du0, dk0 = raw_step(plan, kf, u, dout, save)
    wide = {n: torch.full((B, Cw, L), v, dtype=dtype, device="cuda") for n, v in (("u", float("nan")), ("dout", float("nan")), ("y", 5.0), ("du", 3.0))}
    wide["u"][:, 1:1 + H] = u
    wide["dout"][:, 3:3 + H] = dout
    ys, dus = wide["y"][:, 2:2 + H], wide["du"][:, 0:H]
    _, _, dk1 = raw_step(plan, kf, wide["u"][:, 1:1 + H], wide["dout"][:, 3:3 + H], save, y=ys, du=dus,
                         sb_u=Cw * L, sb_y=Cw * L, sb_dout=Cw * L, sb_du=Cw * L)
    assert torch.equal(ys, y0) and torch.equal(dus, du0) and torch.equal(dk1, dk0)
    assert bool((wide["y"][:, :2] == 5.0).all()) and bool((wide["y"][:, 2 + H:] == 5.0).all()), "the strided y store touched another channel"
    assert bool((wide["du"][:, H:] == 3.0).all()), "the strided du store touched another channel"
