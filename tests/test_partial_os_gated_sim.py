"""The gated blocked-row kernels on the CPU wave simulator (conv_os_g_kernel, dkf_os_g_kernel; fft 4096, S = 2048, bf16): the forward
y = postgate * conv(x * pregate, k) + residual, the input-gradient launch (dx and dpregate), the dpostgate launch and the gated dk_f launch
+ inverse, per row and per element against the float64 oracle (tests/rowcheck.py).  L and P as tests/test_partial_os_sim.py: S + 1 (one
sample in the second block), 3 S - 5 (element-wise arm, ragged last block, B * nblk odd) and 2 S (16-byte path with its clamped loads)."""
import ctypes
import numpy as np
import pytest
import torch

import rowcheck as RC
import simlib as S_

N, S, DT, B, H = 4096, 2048, S_.DT_BF16, 3, 2
VP, I = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    L = S_.lib()
    L.ffcsim_conv_fwd_os_gated.argtypes = [I, I] + [VP] * 8 + [I] * 5
    L.ffcsim_conv_bwd_dkf_os_gated.argtypes = [I, I] + [VP] * 5 + [I] * 3
    return L


def _t(bits):
    return torch.from_numpy(S_.from_bits(bits, DT)).to(torch.bfloat16)


@pytest.mark.parametrize("L,P", [(S + 1, S), (3 * S - 5, S // 2 + 1), (2 * S, 7)], ids=["S+1", "3S-5", "2S"])
def test_gated_blocked_rows_on_the_simulator(lib, L, P):
    rng = np.random.default_rng(L + P)
    x, pre, post, res, dout = (S_.to_bits(rng.standard_normal((B, H, L)).astype(np.float32), DT) for _ in range(5))
    k = (0.1 * rng.standard_normal((H, P))).astype(np.float32)
    f64 = lambda bits: S_.from_bits(bits, DT).astype(np.float64)
    want = RC.oracle(f64(x), k.astype(np.float64), f64(dout), 1 << (L + P).bit_length(), f64(pre), f64(post), f64(res))
    p, kf = S_.p, S_.sim_kernel_fft(N, DT, k)
    y, dx, dpre, dpost = (np.zeros_like(x) for _ in range(4))
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(x), p(kf), p(pre), p(post), p(res), p(y), None, None, B, H, L, 0, 1) == 0
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(dout), p(kf), p(post), p(pre), None, p(dx), p(x), p(dpre), B, H, L, 1, 0) == 0
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(x), p(kf), p(pre), p(dout), None, p(dpost), None, None, B, H, L, 0, 1) == 0
    ws = np.full(lib.ffcsim_upw(N) * H * S_.plan_info(N, DT)[0] * 2048, np.nan, np.float32)
    nslab = lib.ffcsim_conv_bwd_dkf_os_gated(N, DT, p(dout), p(x), p(pre), p(post), p(ws), B, H, L)
    assert nslab == 1
    dk = np.full((H, P), np.nan, np.float32)
    assert lib.ffcsim_kernel_ifft_grad(N, DT, p(ws), nslab, H, P, p(dk)) == 0
    got = {"y": _t(y), "du": _t(dx), "dk": torch.from_numpy(dk), "dpregate": _t(dpre), "dpostgate": _t(dpost)}
    rep = RC.check(got, want, RC.head_map(H), torch.bfloat16, gated=True)
    print(f"\npartial_os_gated_sim L={L} P={P}: {rep.line()}", end="")
    rep.assert_ok(f"L = {L}, P = {P}")


def test_outputs_that_overlap_an_input_are_refused(lib):
    """a block is its successor's history: y on x, the second output on y, and a second output without its gate"""
    x, g = (np.zeros((1, 1, S + 8), np.uint16) for _ in range(2))
    kf, p = S_.sim_kernel_fft(N, DT, np.ones((1, 4), np.float32)), S_.p
    y = np.zeros_like(x)
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(x), p(kf), p(g), None, None, p(x), None, None, 1, 1, S + 8, 0, 1) == -3
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(x), p(kf), None, None, None, p(y), p(g), p(y), 1, 1, S + 8, 0, 1) == -3
    assert lib.ffcsim_conv_fwd_os_gated(N, DT, p(x), p(kf), None, None, None, p(y), None, p(g), 1, 1, S + 8, 0, 1) == -8
