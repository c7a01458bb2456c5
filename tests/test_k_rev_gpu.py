"""Bidirectional filters on the GPU: FlashFFTConv(u, k, ..., k_rev=kr), FlashHyenaOp / FlashHyenaMixer(..., k_rev=, k_res_rev=).

The call with (k, kr) is the call on the fft-size row

    k_full = pad(k, (0, N - Lk)) + pad(flip(kr), (N - Lr, 0))

(reference examples/bert/monarch_mixer_sequence_mixer_flashfftconv.py:141-170).  On the fused routes the k -> k_f kernel reads both tensors and the
dk_f -> dk kernel writes both gradients; every result is compared BIT FOR BIT with the same module called on the torch-composed k_full, whose
gradient dk_full is sliced: dk = dk_full[:, :Lk], dk_rev = flip(dk_full[:, N - Lr:]).  One case per dtype goes to the float64 oracle
(tests/rowcheck.py) to anchor the formula itself.  The routes that compose (HBM levels, folded fft 2048, frequency-sparse) are checked against
their own call on k_full.  The same kernels' body runs on the CPU simulator in tests/test_k_rev_sim.py."""
import os, re, subprocess, sys

import pytest
import torch

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
DT_NAME = {BF: "bf16", FP: "fp16"}
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def k_full_of(k, kr, N):
    pad = torch.nn.functional.pad
    return pad(k, (0, N - k.shape[-1])) + pad(kr.flip(-1), (N - kr.shape[-1], 0))


def inputs(N, B, H, L, Lk, Lr, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda: torch.randn(B, H, L, device="cuda", generator=g).to(dtype)
    u, dout, pre, post, res = mk(), mk(), mk(), mk(), mk()
    k = torch.randn(H, Lk, device="cuda", generator=g) * 0.1
    kr = torch.randn(H, Lr, device="cuda", generator=g) * 0.1
    return u, dout, pre, post, res, k, kr


def step(conv, u, dout, filt, pre=None, post=None, res=None):
    """forward + backward; filt = (k, kr) or (k_full,) -> (y, du, [dpre, dpost,] d(filter tensors)...)"""
    leaves = [t.detach().requires_grad_(True) for t in (u,) + ((pre, post) if pre is not None else ()) + tuple(filt)]
    nf = len(filt)
    f = leaves[-nf:]
    gates = leaves[1:3] if pre is not None else [None, None]
    y = conv(leaves[0], f[0], gates[0], gates[1], res) if nf == 1 else conv(leaves[0], f[0], gates[0], gates[1], res, k_rev=f[1])
    grads = torch.autograd.grad(y, leaves, dout)
    return (y.detach(),) + tuple(grads)


def compare(conv, N, u, dout, k, kr, pre=None, post=None, res=None, what=""):
    """the k_rev call against the call on the composed row, every result bit for bit"""
    Lk, Lr = k.shape[-1], kr.shape[-1]
    got = step(conv, u, dout, (k, kr), pre, post, res)
    ref = step(conv, u, dout, (k_full_of(k, kr, N),), pre, post, res)
    names = ["y", "du"] + (["dpregate", "dpostgate"] if pre is not None else [])
    for i, nm in enumerate(names):
        assert same(got[i], ref[i]), f"{what} {nm}: {int((got[i] != ref[i]).sum())} elements differ"
    dk, dkr, dkf = got[-2], got[-1], ref[-1]
    assert dk.dtype == torch.float32 and dkr.dtype == torch.float32
    assert same(dk, dkf[:, :Lk]), f"{what} dk: {int((dk != dkf[:, :Lk]).sum())} elements differ"
    want_r = dkf[:, N - Lr:].flip(-1)
    assert same(dkr, want_r), f"{what} dk_rev: {int((dkr != want_r).sum())} elements differ"


FUSED = [256, 1024, 2048, 4096, 32768, 65536]


@pytest.mark.parametrize("save", [True, False], ids=["saved", "recompute"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", FUSED)
def test_module_fused_routes_match_the_composed_row(N, dtype, gated, save):
    from flashfftconv import FlashFFTConv
    B, H, L = 3, 3, N // 2
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    conv.save_spectrum = save
    assert not conv._k_rev_composes()
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, dtype, N + 3 * int(gated))
    g = (pre, post) if gated else (None, None)
    compare(conv, N, u, dout, k, kr, *g, what=f"N={N}")


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", FUSED)
def test_module_with_a_residual(N, dtype):
    from flashfftconv import FlashFFTConv
    B, H, L = 3, 3, N // 2
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, dtype, N + 11)
    compare(conv, N, u, dout, k, kr, pre, post, res, what=f"N={N} residual")


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", FUSED)
def test_module_odd_lengths(N, dtype):
    """Lk, Lr odd: the per-element loads and stores"""
    from flashfftconv import FlashFFTConv
    B, H, L = 3, 3, N // 2
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L - 3, L - 5, dtype, N + 5)
    compare(conv, N, u, dout, k, kr, what=f"N={N} odd")


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_module_overlapping_taps_add(dtype):
    from flashfftconv import FlashFFTConv
    N, B, H, L = 1024, 3, 3, 512
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, 768, 512, dtype, 77)
    compare(conv, N, u, dout, k, kr, pre, post, what="overlap")


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_oracle_on_the_composed_row(dtype):
    """the formula itself: y, du, both gate gradients and dk_full = [dk | flip(dk_rev)] against the float64 oracle on k_full, per row and per
    element with the gates of tests/test_fused_rows_gpu.py (rowcheck.gates; random unit-scale input gates)"""
    import rowcheck as RC
    from flashfftconv import FlashFFTConv
    N, B, H, L = 4096, 3, 3, 2048
    conv = FlashFFTConv(N, dtype=dtype).to("cuda")
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, dtype, 4096 + int(dtype == FP))
    kfull = k_full_of(k, kr, N)
    want = RC.oracle(*(t.double().cpu().numpy() for t in (u, kfull, dout)), N, pre.double().cpu().numpy(), post.double().cpu().numpy())
    y, du, dpre, dpost, dk, dkr = step(conv, u, dout, (k, kr), pre, post)
    got = {"y": y, "du": du, "dk": torch.cat((dk, dkr.flip(-1)), dim=-1), "dpregate": dpre, "dpostgate": dpost}
    rep = RC.check(got, want, RC.head_map(H), dtype, True)
    print(f"\nk_rev oracle N={N} {DT_NAME[dtype]}: {rep.line()}")
    rep.assert_ok("k_rev against the float64 oracle")


# ---------------------------------------------------------------- routes that compose
def composed_case(conv, N, B, H, L, dtype, seed):
    assert conv._k_rev_composes()
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, dtype, seed)
    compare(conv, N, u, dout, k, kr, what=f"composed N={N}")


def test_composed_hbm_level():
    from flashfftconv import FlashFFTConv
    composed_case(FlashFFTConv(262144, dtype=BF).to("cuda"), 262144, 1, 2, 131072, BF, 1)


def test_composed_frequency_sparse():
    from flashfftconv import FlashFFTConv
    conv = FlashFFTConv(4096, dtype=BF).to("cuda")
    conv._kf_keep = 512
    composed_case(conv, 4096, 3, 3, 2048, BF, 2)


def test_composed_folded_2048():
    """fft 2048 on the folded 4096 plan (FFC_MULTIPASS without 2048 is read at import: a child process)"""
    env = dict(os.environ, FFC_MULTIPASS="65536,131072")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "folded"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "k_rev folded ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------- eval, cache
def test_eval_cache_key_covers_both_tensors():
    from flashfftconv import FlashFFTConv
    N, B, H, L = 4096, 2, 3, 2048
    conv = FlashFFTConv(N, dtype=BF).to("cuda").eval()
    conv.cache_kf = True
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, BF, 9)
    with torch.no_grad():
        y0 = conv(u, k, k_rev=kr)
        assert same(y0, conv(u, k_full_of(k, kr, N)))
        y1 = conv(u, k, k_rev=kr)
        assert same(y0, y1)
        kr.mul_(-1.0)                        # k_rev alone changes, in place
        y2 = conv(u, k, k_rev=kr)
        assert not same(y2, y0), "a stale k_f served a changed k_rev"
        assert same(y2, conv(u, k_full_of(k, kr, N)))
        y3 = conv(u, k)                      # and the one-tensor call does not take the pair's k_f
        assert same(y3, conv(u, torch.nn.functional.pad(k, (0, N - L))))


# ---------------------------------------------------------------- operator
def make_op(D, fft, dtype, mixer):
    from flashfftconv import FlashHyenaOp, FlashHyenaMixer
    g = torch.Generator(device="cuda").manual_seed(D + fft)
    w = torch.randn(3 * D, 1, 3, device="cuda", generator=g) * 0.5
    b = torch.randn(3 * D, device="cuda", generator=g) * 0.1
    if not mixer:
        return FlashHyenaOp(D, fft, w, b, dtype=dtype, device="cuda").to("cuda")
    torch.manual_seed(D + fft)
    inp, outp = torch.nn.Linear(D, 3 * D).to("cuda", dtype), torch.nn.Linear(D, D).to("cuda", dtype)
    return FlashHyenaMixer(D, fft, inp, outp, w, b, dtype=dtype, device="cuda").to("cuda")


@pytest.mark.parametrize("mixer", [False, True], ids=["op", "mixer"])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,D,L,fft", [(2, 40, 512, 1024), (2, 64, 2048, 4096)])
def test_operator_matches_composed_filters(B, D, L, fft, dtype, mixer):
    op = make_op(D, fft, dtype, mixer)
    g = torch.Generator(device="cuda").manual_seed(B + D + L)
    x = (torch.randn(B, L, D, device="cuda", generator=g) if mixer else torch.randn(B, 3 * D, L, device="cuda", generator=g)).to(dtype)
    filt = [torch.randn(D, L, device="cuda", generator=g) * 0.1 for _ in range(4)]      # k, k_rev, k_res, k_res_rev
    out = None

    def run(fused):
        nonlocal out
        op.zero_grad(set_to_none=True)
        xs = x.detach().requires_grad_(True)
        f = [t.detach().requires_grad_(True) for t in filt]
        if fused:
            y = op(xs, f[0], f[2], k_rev=f[1], k_res_rev=f[3])
        else:
            y = op(xs, k_full_of(f[0], f[1], fft), k_full_of(f[2], f[3], fft))
        if out is None:
            out = torch.randn(y.shape, device="cuda", generator=g).to(dtype)
        y.backward(out)
        # (a parameter the operator does not read has no gradient on either side: the mixer drops the in-projection bias)
        return [y.detach(), xs.grad] + [t.grad for t in f] + [None if p.grad is None else p.grad.clone() for p in op.parameters()]

    got, ref = run(True), run(False)
    assert len(got) == len(ref) and all(t is not None for t in got[:6]) and sum(t is not None for t in got[6:]) >= 2
    for i, (a, b) in enumerate(zip(got, ref)):
        assert (a is None) == (b is None), f"result {i}: a gradient on one side only"
        assert a is None or same(a, b), f"result {i}: {int((a != b).sum())} elements differ"


# ---------------------------------------------------------------- launches
def kernels_of(fn):
    from torch.profiler import profile, ProfilerActivity
    fn(); torch.cuda.synchronize()             # plans, caches
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn(); torch.cuda.synchronize()
    names = []
    for e in p.events():
        nm = e.name
        if nm.startswith(("Memcpy", "Memset", "hip", "cuda")):
            continue
        m = re.search(r"([A-Za-z0-9_]*kernel[A-Za-z0-9_]*)", nm)
        names.append(re.sub(r"^(_Z)?\d*", "", m.group(1)) if m else nm)
    return names


def test_launches_of_the_fused_call():
    """no pad, flip or add kernel on the filter: the module's forward is the two-tensor k -> k_f kernel and the convolution kernel"""
    from flashfftconv import FlashFFTConv
    N, B, H, L = 4096, 2, 3, 2048
    conv = FlashFFTConv(N, dtype=BF).to("cuda").eval()
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, BF, 13)
    with torch.no_grad():
        fused = kernels_of(lambda: conv(u, k, k_rev=kr))
        composed = kernels_of(lambda: conv(u, k_full_of(k, kr, N)))
    print(f"\nk_rev launches: fused {fused}; composed {composed}")
    assert fused == ["kfft_bi_kernel", "conv_kernel"], fused
    assert len(composed) > len(fused), composed


def test_launches_of_the_fused_operator():
    """one k -> k_f kernel per filter, and fewer launches than the operator on torch-composed filters"""
    B, D, L, fft = 2, 64, 2048, 4096
    op = make_op(D, fft, BF, False).eval()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, 3 * D, L, device="cuda", generator=g).to(BF)
    f = [torch.randn(D, L, device="cuda", generator=g) * 0.1 for _ in range(4)]
    with torch.no_grad():
        fused = kernels_of(lambda: op(x, f[0], f[2], k_rev=f[1], k_res_rev=f[3]))
        composed = kernels_of(lambda: op(x, k_full_of(f[0], f[1], fft), k_full_of(f[2], f[3], fft)))
    print(f"\nk_rev operator launches: fused {fused}; composed {composed}")
    assert [n for n in fused if "kfft" in n] == ["kfft_bi_kernel", "kfft_bi_kernel"], fused
    assert not [n for n in fused if "elementwise" in n or "pad" in n or "flip" in n], fused
    assert len(composed) > len(fused), composed


# ---------------------------------------------------------------- errors
def test_errors():
    from flashfftconv import FlashFFTConv
    N, B, H, L = 1024, 2, 3, 512
    conv = FlashFFTConv(N, dtype=BF).to("cuda")
    u, dout, pre, post, res, k, kr = inputs(N, B, H, L, L, L, BF, 3)
    with pytest.raises(RuntimeError):
        conv(u, k, k_rev=kr[:2])                                   # wrong H
    with pytest.raises(RuntimeError):
        conv(u, k, k_rev=torch.zeros(H, N + 1, device="cuda"))     # Lr > seqlen
    with pytest.raises(RuntimeError):
        conv(u, k, k_rev=kr.cpu())                                 # CPU tensor
    with pytest.raises(RuntimeError):
        conv(u, k, k_rev=kr[0])                                    # 1-D


if __name__ == "__main__" and sys.argv[1:] == ["folded"]:
    ROOT = os.path.dirname(HERE)
    for p in (os.path.join(ROOT, "flash-fft-conv_amd"), HERE, ROOT):
        sys.path.insert(0, p)
    from flashfftconv import FlashFFTConv
    mod = FlashFFTConv(2048, dtype=BF).to("cuda")
    assert mod._folded, "FFC_MULTIPASS without 2048 must select the folded plan"
    composed_case(mod, 2048, 3, 3, 1024, BF, 4)
    print("k_rev folded ok")
