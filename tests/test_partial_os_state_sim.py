"""The history form of the gated blocked-row kernels on the CPU wave simulator (conv_os_h_kernel, dkf_os_h_kernel; fft 4096, S = 2048).
A row of 4 S is cut into chunks of 2 S and every chunk is fed the tail of the previous chunk's x * pregate as its history: every pair of
planes then holds the same two windows as in the gated call on the whole row, so y is compared bit for bit with it.  The dk_f sums added
over the chunks go against the float64 oracle (tests/rowcheck.py), block -1 of the input-gradient launch against the float64 correlation of
dout * postgate with k, and the blocks >= 0 of that launch against the oracle's dx and dpregate of the last chunk."""
import ctypes
import numpy as np
import pytest
import torch

import rowcheck as RC
import simlib as S_

N, S, B, H, L, P = 4096, 2048, 3, 2, 4 * 2048, 2048
VP, I = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    lb = S_.lib()
    lb.ffcsim_conv_fwd_os_gated.argtypes = [I, I] + [VP] * 8 + [I] * 5
    lb.ffcsim_conv_fwd_os_hist.argtypes = [I, I] + [VP] * 10 + [I] * 5
    lb.ffcsim_conv_bwd_dkf_os_hist.argtypes = [I, I] + [VP] * 6 + [I] * 3
    return lb


@pytest.mark.parametrize("DT", [S_.DT_BF16, S_.DT_F16], ids=["bf16", "fp16"])
def test_chunks_with_a_history_on_the_simulator(lib, DT):
    tdt = torch.bfloat16 if DT == S_.DT_BF16 else torch.float16
    rng = np.random.default_rng(DT)
    x, pre, post, res, dout = (S_.to_bits(rng.standard_normal((B, H, L)).astype(np.float32), DT) for _ in range(5))
    k = (0.1 * rng.standard_normal((H, P))).astype(np.float32)
    f64 = lambda bits: S_.from_bits(bits, DT).astype(np.float64)
    t = lambda bits: torch.from_numpy(S_.from_bits(bits, DT)).to(tdt)
    want = RC.oracle(f64(x), k.astype(np.float64), f64(dout), 1 << (L + P).bit_length(), f64(pre), f64(post), f64(res))
    p, kf = S_.p, S_.sim_kernel_fft(N, DT, k)
    whole = np.zeros_like(x)
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(x), p(kf), p(pre), p(post), p(res), p(whole), None, None, B, H, L, 0, 1) == 0
    # (the product of two 16-bit values is exact in fp32: one rounding, as at the kernel's LDS write)
    xg = S_.to_bits(S_.from_bits(x, DT) * S_.from_bits(pre, DT), DT)
    y, dk, hist = np.zeros_like(x), np.zeros((H, P), np.float32), None
    for c0 in (0, 2 * S):
        cut = lambda a: np.ascontiguousarray(a[..., c0:c0 + 2 * S])
        xc, prec, postc, resc, dc, yc = (cut(a) for a in (x, pre, post, res, dout, y))
        assert lib.ffcsim_conv_fwd_os_hist(N, DT, p(xc), p(kf), p(prec), p(postc), p(resc), p(yc), None, None, p(hist), None, B, H, 2 * S, 0, 1) == 0
        y[..., c0:c0 + 2 * S] = yc
        ws = np.full(lib.ffcsim_upw(N) * H * S_.plan_info(N, DT)[0] * 2048, np.nan, np.float32)
        nslab = lib.ffcsim_conv_bwd_dkf_os_hist(N, DT, p(dc), p(xc), p(prec), p(postc), p(hist), p(ws), B, H, 2 * S)
        dkc = np.full((H, P), np.nan, np.float32)
        assert nslab == 1 and lib.ffcsim_kernel_ifft_grad(N, DT, p(ws), nslab, H, P, p(dkc)) == 0
        dk += dkc
        hist = np.ascontiguousarray(xg[..., c0 + S:c0 + 2 * S])
    assert np.array_equal(y, whole), "chunks with a history differ from the call on the whole row"
    rep = RC.check({"y": t(y), "dk": torch.from_numpy(dk)}, want, RC.head_map(H), tdt, gated=True)
    # input-gradient launch of the last chunk with its block -1: dstate[n] = sum_s k[s] (dout * postgate)[n - S + s]; the blocks >= 0 are
    # the whole row's dx and dpregate there (nothing follows the last chunk; the blocks pair up differently, so no bit identity)
    dx, dpre, dst = np.zeros_like(xc), np.zeros_like(xc), np.zeros((B, H, S), np.uint16)
    assert lib.ffcsim_conv_fwd_os_hist(N, DT, p(dc), p(kf), p(postc), p(prec), None, p(dx), p(xc), p(dpre), None, p(dst), B, H, 2 * S, 1, 0) == 0
    last = lambda part: {nm: part[nm][..., 2 * S:] for nm in ("du", "dpregate")}
    rep1 = RC.check({"du": t(dx), "dpregate": t(dpre)}, RC.Want(last(want.want), last(want.scale)), RC.head_map(H), tdt, gated=True)
    g = f64(dc) * f64(postc)
    corr = np.stack([[np.concatenate((np.zeros(S), np.convolve(g[b, h], k[h, ::-1].astype(np.float64))))[P - 1:P - 1 + S] for h in range(H)] for b in range(B)])
    rep2 = RC.check({"du": t(dst)}, RC.Want({"du": corr}, {"du": RC.rms(corr)}), RC.head_map(H), tdt, gated=True)
    print(f"\npartial_os_state_sim {tdt}: {rep.line()}  last chunk {rep1.line()}  dstate {rep2.line()}", end="")
    for r, what in ((rep, "chunked y and dk"), (rep1, "dx and dpregate next to block -1"), (rep2, "dstate")):
        r.assert_ok(what)


def test_history_form_refusals(lib):
    """a history needs the wrapped window, a state gradient the natural-order one, and neither may overlap another tensor of the launch"""
    DT, p = S_.DT_BF16, S_.p
    x, y, h, dh = (np.zeros((1, 1, S), np.uint16) for _ in range(4))
    kf = S_.sim_kernel_fft(N, DT, np.ones((1, 4), np.float32))
    call = lambda hist, dhist, wrap, out=y: lib.ffcsim_conv_fwd_os_hist(N, DT, p(x), p(kf), None, None, None, p(out), None, None, p(hist), p(dhist), 1, 1, S, 0, wrap)
    assert call(h, None, 1) == 0 and call(None, dh, 0) == 0
    assert call(h, None, 0) == -8 and call(None, dh, 1) == -8
    assert call(h, None, 1, out=h) == -3 and call(None, x, 0) == -3
