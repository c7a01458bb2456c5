"""The residual input of the convolution's output epilogue on the GPU: ffc_conv_fwd_res (C-ABI), FlashFFTConv(..., residual=r) and the
M2 residual long convolution of the fused operator, FlashHyenaOp / FlashHyenaMixer(..., k_res):

    y = postgate * conv(u * pregate, k) + residual          fp32 product and sum, ONE rounding to the module dtype
    y = x2 * conv(x1 * v, k) + conv(v, k_res)               (reference examples/bert/monarch_mixer_sequence_mixer_flashfftconv.py:151-175)

The store sites and their routes are those of tests/test_residual_sim.py (same kernels' body on the CPU simulator)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle.torch_ref import ref_fft_conv

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 3e-2, torch.float16: 8e-3}      # the relative-norm gates of tests/test_hyena_gpu.py


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def fc64(u, k, n):
    """float64 oracle: ifft(fft(u, n) * fft(k, n)).real[..., :L]"""
    L = u.shape[-1]
    return torch.fft.ifft(torch.fft.fft(u.double(), n=n) * torch.fft.fft(k.double(), n=n), n=n).real[..., :L]


def bits(t):
    return t.contiguous().view(torch.int16)


# (fft size, L, H): B = 3 everywhere -- the last pair is half empty
ROUTES = [
    (256, 256, 2), (1024, 1024, 2), (1024, 999, 2),      # single tile: rows_out_g, and rows_out's element-wise arm
    (2048, 1024, 3),                                       # merged store
    (2048, 2048, 2),                                       # per-pass store: rows_out_rp_t, addend on the last pass
    (2048, 1001, 2),                                       # ... its element-wise arm
    (4096, 4096, 3),                                       # one wave per unit
    (16384, 8192, 2), (16384, 16384, 2),                   # HALF / full rows: rows_out_g
    (16384, 8189, 2),                                      # not 16-byte: rows_out instead of rows_out_g
    (32768, 16384, 2),                                     # HALF on the 32-point outer digit
    (65536, 32768, 2), (65536, 65536, 2), (65536, 65533, 2),      # 2 passes: one row block, two row blocks, element-wise
    (131072, 131072, 2),                                   # 4 passes
]


def _inputs(B, H, L, dtype, seed, n=4):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(B, H, L, device="cuda", generator=g).to(dtype) for _ in range(n)]


# ---------------------------------------------------------------- C-ABI
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,L,H", ROUTES)
def test_abi_addend_is_one_rounding_after_the_gate(N, L, H, dtype, gated):
    from flashfftconv import _lib
    from flashfftconv.conv import get_plan, _kernel_fft
    B = 3
    lib = _lib.lib()
    plan = get_plan(N, dtype, "cuda")
    u, g1, g2, r = _inputs(B, H, L, dtype, N + L)
    k = torch.randn(H, min(L, N), device="cuda") * 0.1
    kf = _kernel_fft(plan, k)
    pre, post = (g1, g2) if gated else (None, None)

    def run(add):
        y = torch.zeros_like(u)
        yraw = torch.zeros_like(u)
        z = torch.zeros(lib.ffc_spectrum_bytes(plan.handle, B, H), dtype=torch.uint8, device="cuda")
        _lib.check(lib.ffc_conv_fwd_res(plan.handle, _lib.ptr(u), _lib.ptr(kf), _lib.ptr(pre), _lib.ptr(post), _lib.ptr(add), _lib.ptr(y),
                                        _lib.ptr(z), _lib.ptr(yraw), B, H, L, 0, 0, 0, 0, 0, 0, _lib.stream_ptr()), "ffc_conv_fwd_res")
        torch.cuda.synchronize()
        return y, z, yraw

    y, z, yraw = run(r)
    assert yraw.abs().sum() > 0, "y_raw was not written"
    want = ((yraw.float() * post.float() if gated else yraw.float()) + r.float()).to(dtype)
    assert torch.equal(bits(y), bits(want))
    y0, z0, yraw0 = run(None)
    assert torch.equal(bits(yraw), bits(yraw0)), "y_raw must not see the addend"
    assert torch.equal(z, z0)


def test_abi_strides_and_overlap():
    """addend and y as channel slices of wider tensors; an addend that overlaps y is refused without a launch"""
    from flashfftconv import _lib
    from flashfftconv.conv import get_plan, _kernel_fft
    lib = _lib.lib()
    for N, L in ((1024, 1024), (16384, 8192), (65536, 32768)):
        dtype, B, H = torch.bfloat16, 3, 2
        plan = get_plan(N, dtype, "cuda")
        u, g1, g2, r = _inputs(B, H, L, dtype, N)
        kf = _kernel_fft(plan, torch.randn(H, L, device="cuda") * 0.1)
        wide_r = torch.full((B, H + 2, L), float("nan"), dtype=dtype, device="cuda")
        wide_r[:, 1:1 + H] = r
        wide_y = torch.full((B, H + 1, L), 7.0, dtype=dtype, device="cuda")
        yraw = torch.zeros_like(u)
        z = torch.zeros(lib.ffc_spectrum_bytes(plan.handle, B, H), dtype=torch.uint8, device="cuda")
        add_ptr = ctypes.c_void_p(wide_r.data_ptr() + L * 2)
        _lib.check(lib.ffc_conv_fwd_res(plan.handle, _lib.ptr(u), _lib.ptr(kf), _lib.ptr(g1), _lib.ptr(g2), add_ptr, _lib.ptr(wide_y),
                                        _lib.ptr(z), _lib.ptr(yraw), B, H, L, 0, 0, 0, 0, (H + 2) * L, (H + 1) * L, _lib.stream_ptr()),
                   "ffc_conv_fwd_res")
        torch.cuda.synchronize()
        want = (yraw.float() * g2.float() + r.float()).to(dtype)
        assert torch.equal(bits(wide_y[:, :H]), bits(want))
        assert (wide_y[:, H:] == 7.0).all()
        y = r.clone()
        rc = lib.ffc_conv_fwd_res(plan.handle, _lib.ptr(u), _lib.ptr(kf), None, None, _lib.ptr(y), _lib.ptr(y), None, None, B, H, L, 0,
                                  0, 0, 0, 0, 0, _lib.stream_ptr())
        assert rc != 0 and b"overlap" in lib.ffc_last_error()
        torch.cuda.synchronize()
        assert torch.equal(bits(y), bits(r)), "a refused call must not run"


# ---------------------------------------------------------------- module, eval / no_grad
@pytest.fixture
def separate_kfft():
    """tuning flag 64 for the test: k -> k_f as the stand-alone kernel in EVERY call, so that a call with a residual and the same call
    without one multiply by the same k_f bits (see test_module_training)"""
    import os
    from flashfftconv import conv as C
    os.environ["FFC_FLAGS"] = "64"; C.reload_env()
    try:
        yield
    finally:
        os.environ.pop("FFC_FLAGS"); C.reload_env()


MODULE_ROUTES = [(256, 256, 2), (1024, 999, 2), (2048, 1024, 3), (2048, 2048, 2), (4096, 4096, 3), (16384, 8192, 2), (16384, 8189, 2),
                 (32768, 16384, 2), (65536, 65536, 2), (131072, 65536, 2)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,L,H", MODULE_ROUTES)
def test_module_eval(N, L, H, dtype, separate_kfft):
    from flashfftconv import FlashFFTConv
    B = 3
    conv = FlashFFTConv(N, dtype=dtype).cuda().eval()
    conv.fit_fft = False
    u, g1, g2, r = _inputs(B, H, L, dtype, 3 * N + L)
    k = torch.randn(H, L, device="cuda") * 0.1
    with torch.no_grad():
        y = conv(u, k, residual=r)
        assert torch.equal(bits(y), bits((conv(u, k).float() + r.float()).to(dtype)))
        yg = conv(u, k, g1, g2, residual=r)
    want = g2.double() * fc64(u.double() * g1.double(), k, N) + r.double()
    print(f"gated + residual, fft {N} L {L} {dtype}: rel {rel(yg, want):.3e} (gate {TOL[dtype]:.0e})")
    assert rel(yg, want) < TOL[dtype]


# ---------------------------------------------------------------- module, training
@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N,L,H", [(1024, 1024, 2), (2048, 1024, 3), (4096, 2048, 3), (16384, 8192, 2), (32768, 16384, 2), (65536, 32768, 2)])
def test_module_training(N, L, H, dtype, save, separate_kfft):
    """y within the gates; d residual == dout and du, dk, dpregate, dpostgate bit for bit those of the same call without a residual
    (a y_raw stored after the add, or an addend that reached the backward, would show in dpostgate / du).

    Both calls run with tuning flag 64 (k -> k_f as the stand-alone kernel): without a residual the module's one-call forward transforms
    the filter inside the convolution launch at fft 8192 ... 32768, with one it runs ffc_kernel_fft first, and the two kernels may land
    single k_f values on neighbouring values (tests/test_spectrum_gpu.py::test_one_launch_per_direction_equals_the_separate_kernels) --
    first run of this test, without the flag: every case bit-equal except fft 16384 fp16 without kept spectra, du 5.6e-5 apart in
    relative norm.  With the same k_f kernel in both calls every difference left is the residual's."""
    from flashfftconv import FlashFFTConv
    B = 3
    conv = FlashFFTConv(N, dtype=dtype).cuda().train()
    conv.fit_fft = False
    conv.save_spectrum = "always" if save else False
    u, g1, g2, r, dout = _inputs(B, H, L, dtype, 5 * N + L, 5)
    k = torch.randn(H, L, device="cuda") * 0.1

    def step(gated, res):
        leaves = [t.clone().requires_grad_(True) for t in ((u, k, g1, g2) if gated else (u, k))]
        rr = r.clone().requires_grad_(True) if res else None
        y = conv(*leaves, residual=rr) if res else conv(*leaves)
        g = torch.autograd.grad(y, leaves + ([rr] if res else []), dout)
        return y, g

    for gated in (False, True):
        y, g = step(gated, True)
        y0, g0 = step(gated, False)
        conv_out = fc64(u.double() * g1.double(), k, N) * g2.double() if gated else fc64(u, k, N)
        print(f"training fft {N} L {L} {dtype} gated {gated} save {save}: y rel {rel(y, conv_out + r.double()):.3e}")
        assert rel(y, conv_out + r.double()) < TOL[dtype]
        assert torch.equal(bits(g[-1]), bits(dout)), "d residual must be dout"
        for a, b, name in zip(g[:-1], g0, ("du", "dk", "dpregate", "dpostgate")):
            same = torch.equal(a, b)
            print(f"  {name}: bit-equal {same}, rel {rel(a, b):.3e}")
            assert same, f"{name} differs from the call without a residual"


# ---------------------------------------------------------------- routes without a fused epilogue: composition
def test_big_size_composes():
    from flashfftconv import FlashFFTConv
    N, B, H, L, dtype = 262144, 1, 2, 131080, torch.bfloat16
    conv = FlashFFTConv(N, dtype=dtype).cuda().eval()
    assert conv._residual_composes(L)
    u, r = _inputs(B, H, L, dtype, 9, 2)
    k = torch.randn(H, L, device="cuda") * 0.05
    with torch.no_grad():
        assert torch.equal(bits(conv(u, k, residual=r)), bits(conv(u, k) + r))
    ur, rr = u.clone().requires_grad_(True), r.clone().requires_grad_(True)
    conv.train()
    dout = torch.randn_like(u)
    (dr,) = torch.autograd.grad(conv(ur, k, residual=rr), [rr], dout)
    assert torch.equal(bits(dr), bits(dout))


def test_frequency_sparse_kernel_composes():
    from flashfftconv import FrequencySparseFFTConv
    B, H, L, dtype = 3, 2, 8192, torch.bfloat16
    m = FrequencySparseFFTConv(1024).cuda().eval()      # fft 16384, 512 kept bins: one spectrum row per side, the compute-skipping kernel
    x, r = _inputs(B, H, L, dtype, 10, 2)
    k = torch.randn(H, L, device="cuda") * 0.05
    with torch.no_grad():
        y0 = m(x, k)
        assert m._conv_for(x, keep=512)._residual_composes(L)
        assert torch.equal(bits(m(x, k, residual=r)), bits(y0 + r))


# ---------------------------------------------------------------- the fused operator with k_res
@pytest.mark.parametrize("B,D,L,fft,dtype", [(2, 40, 512, 1024, torch.bfloat16), (2, 64, 1024, 2048, torch.bfloat16),
                                             (3, 96, 2048, 4096, torch.bfloat16), (2, 128, 8192, 16384, torch.float16),
                                             (2, 32, 32768, 65536, torch.bfloat16), (1, 16, 131072, 262144, torch.bfloat16),
                                             (2, 16, 8192, 131072, torch.bfloat16)])      # the last: fft size fitted to the rows
def test_hyena_op_with_k_res(B, D, L, fft, dtype):
    from flashfftconv import FlashHyenaOp
    torch.manual_seed(11)
    sf = nn.Conv1d(3 * D, 3 * D, 3, padding=1, groups=3 * D).cuda()
    with torch.no_grad():
        sf.weight.copy_(sf.weight.to(dtype).float()); sf.bias.copy_(sf.bias.to(dtype).float())
    op = FlashHyenaOp(D, fft, sf.weight.detach(), sf.bias.detach(), dtype=dtype, device="cuda").cuda()
    u = torch.randn(B, 3 * D, L, device="cuda").to(dtype)
    k = torch.randn(D, L, device="cuda") * 0.05
    k2 = torch.randn(D, L, device="cuda") * 0.05
    dy = torch.randn(B, D, L, device="cuda").to(dtype)

    uf, kf_, k2f = u.clone().requires_grad_(True), k.clone().requires_grad_(True), k2.clone().requires_grad_(True)
    y = op(uf, kf_, k2f)
    gy = torch.autograd.grad(y, [uf, kf_, k2f, op.short_filter.weights, op.short_filter.bias], dy)

    # fp32 oracle of the reference composition fc(x1 * v, k) * x2 + fc(v, k_res)
    uo, ko, k2o = u.float().requires_grad_(True), k.clone().requires_grad_(True), k2.clone().requires_grad_(True)
    uc = sf(uo)[..., :L]
    x1, x2, v = uc.split(D, dim=1)
    yo = ref_fft_conv((x1 * v).to(dtype), ko, n=fft).float() * x2 + ref_fft_conv(v.to(dtype), k2o, n=fft).float()
    go = torch.autograd.grad(yo, [uo, ko, k2o, sf.weight, sf.bias], dy.float())
    tol = TOL[dtype] * (2.0 if fft >= 262144 else 1.0)
    got = (y, gy[0], gy[1], gy[2], gy[3], gy[4])
    ref = (yo, go[0], go[1], go[2], go[3].squeeze(1), go[4])
    for a, b, name in zip(got, ref, ("y", "du", "dk", "dk_res", "dw", "dbias")):
        print(f"hyena k_res fft {fft} L {L} {dtype} {name}: rel {rel(a, b):.3e} (gate {tol:.0e})")
    for a, b, name in zip(got, ref, ("y", "du", "dk", "dk_res", "dw", "dbias")):
        assert rel(a, b) < tol, f"{name} {rel(a, b):.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mixer_with_k_res(dtype):
    from flashfftconv import FlashHyenaMixer, FlashFFTConv, FlashDepthWiseConv1d
    torch.manual_seed(5)
    B, L, D, fft = 2, 2048, 64, 4096
    inp = torch.nn.Linear(D, 3 * D).cuda().to(dtype); outp = torch.nn.Linear(D, D).cuda().to(dtype)
    sf = torch.nn.Conv1d(3 * D, 3 * D, 3, padding=2, groups=3 * D).cuda()
    k = (torch.randn(D, L, device="cuda") * 0.02).requires_grad_(True)
    k2 = (torch.randn(D, L, device="cuda") * 0.02).requires_grad_(True)
    u = (torch.randn(B, L, D, device="cuda") * 0.5).to(dtype).requires_grad_(True)
    mixer = FlashHyenaMixer(D, fft, inp, outp, sf.weight.detach(), sf.bias.detach(), dtype=dtype, device="cuda").cuda()
    short = FlashDepthWiseConv1d(3 * D, 3, padding=1, weights=sf.weight.detach(), bias=sf.bias.detach(), dtype=dtype).cuda()
    conv = FlashFFTConv(fft, dtype=dtype).cuda()

    def reference(u, k, k2):      # monarch_mixer_sequence_mixer_flashfftconv.py:124-175 with residual_long_conv, on this package's drop-in modules
        x = inp.weight @ u.transpose(-1, -2)
        uc = short(x)[..., :L]
        x1, x2, v = uc.split(D, dim=1)
        y = conv((x1 * v).contiguous(), k) * x2
        y = y + conv(v.contiguous(), k2)
        return outp(y.transpose(-1, -2))
    y = mixer(u, k, k2); yr = reference(u, k, k2)
    tol = 2e-2 if dtype == torch.bfloat16 else 4e-3
    relf = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    assert relf(y, yr) < tol, relf(y, yr)
    dy = torch.randn_like(y) * 0.1
    g = torch.autograd.grad(y, [u, k, k2, inp.weight, outp.weight, outp.bias], dy)
    gr = torch.autograd.grad(yr, [u, k, k2, inp.weight, outp.weight, outp.bias], dy)
    for a, b, n in zip(g, gr, ("du", "dk", "dk_res", "d in_proj.weight", "d out_proj.weight", "d out_proj.bias")):
        assert relf(a, b) < 2 * tol, f"{n}: {relf(a, b):.3e}"


def test_operator_kf_cache_has_two_slots():
    from flashfftconv import FlashHyenaOp
    from flashfftconv.conv import _kf_key
    D, L = 32, 2048
    w = torch.randn(3 * D, 3, device="cuda"); b = torch.randn(3 * D, device="cuda")
    op = FlashHyenaOp(D, 4096, w, b, dtype=torch.bfloat16, device="cuda").cuda().eval()
    op.flashfftconv.cache_kf = True
    u = torch.randn(2, 3 * D, L, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(D, L, device="cuda") * 0.1
    k2 = torch.randn(D, L, device="cuda") * 0.1
    with torch.no_grad():
        y1 = op(u, k, k2)
        c, c2 = op.flashfftconv._kf_cache, op.flashfftconv._kf_cache_res
        y2 = op(u, k, k2)
        # both filters were served from their own slot: neither evicted the other
        assert op.flashfftconv._kf_cache is c and op.flashfftconv._kf_cache_res is c2
        assert c[0] == _kf_key(k) and c2[0] == _kf_key(k2)
        assert torch.equal(bits(y1), bits(y2))
        k2.mul_(2.0)
        y3 = op(u, k, k2)
        assert not torch.equal(bits(y3), bits(y2)), "k_res changed in place: its cached k_f is stale"
        op.flashfftconv.cache_kf = False
        assert torch.equal(bits(y3), bits(op(u, k, k2)))


def test_errors():
    from flashfftconv import FlashFFTConv, FlashHyenaOp
    conv = FlashFFTConv(1024, dtype=torch.bfloat16).cuda()
    u = torch.randn(2, 4, 512, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(4, 512, device="cuda")
    with pytest.raises(RuntimeError):
        conv(u, k, residual=u[:, :2])                       # shape
    with pytest.raises(RuntimeError):
        conv(u, k, residual=u.to(torch.float16))            # dtype
    with pytest.raises(RuntimeError):
        conv(u, k, residual=u.cpu())                        # device
    big = FlashFFTConv(262144, dtype=torch.bfloat16).cuda()
    big.fit_fft = False
    with pytest.raises(RuntimeError):
        big(u, k, residual=u[:, :2])                        # the composed routes check too
    D, L = 16, 512
    op = FlashHyenaOp(D, 1024, torch.randn(3 * D, 3, device="cuda"), torch.randn(3 * D, device="cuda"), dtype=torch.bfloat16,
                      device="cuda").cuda()
    x = torch.randn(2, 3 * D, L, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        op(x, torch.randn(D, L, device="cuda"), torch.randn(D + 1, L, device="cuda"))      # k_res with the wrong head count
