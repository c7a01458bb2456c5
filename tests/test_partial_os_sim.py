"""The blocked-row (overlap-save) kernels on the CPU wave simulator: conv_os_kernel forward and input gradient, dkf_os_kernel + the dk
inverse, fft 4096 (S = 2048), against the float64 linear convolution.  L = S + 1: one sample in the second block, 16-byte path off
(L % 8 != 0); L = 3 S - 5: a block before the ragged one and an odd number of blocks (the last pair has one plane); L = 2 S: the
16-byte path with its clamped loads."""
import numpy as np
import pytest

from oracle import ref_fft_conv as O
import simlib as S_

N, S, DT = 4096, 2048, S_.DT_BF16


def _rel(got, want):
    got, want = (np.asarray(t, np.float64).reshape(-1, want.shape[-1]) for t in (got, want))
    return float((np.linalg.norm(got - want, axis=-1) / np.linalg.norm(want, axis=-1)).max())


@pytest.mark.parametrize("L,P", [(S + 1, S), (3 * S - 5, S // 2 + 1), (2 * S, 7)], ids=["S+1", "3S-5", "2S"])
def test_blocked_rows_on_the_simulator(L, P):
    B, H = 1, 2
    rng = np.random.default_rng(L + P)
    xb, db = (S_.to_bits(rng.standard_normal((B, H, L)).astype(np.float32), DT) for _ in range(2))
    k = (0.1 * rng.standard_normal((H, P))).astype(np.float32)
    want = O.ref_partial_keeps(S_.from_bits(xb, DT), k, S_.from_bits(db, DT), [P])[P]
    lib, kf = S_.lib(), S_.sim_kernel_fft(N, DT, k)
    y, dx = np.zeros_like(xb), np.zeros_like(xb)
    assert lib.ffcsim_conv_fwd_os(N, DT, S_.p(xb), S_.p(kf), S_.p(y), B, H, L, 0, 1) == 0
    assert lib.ffcsim_conv_fwd_os(N, DT, S_.p(db), S_.p(kf), S_.p(dx), B, H, L, 1, 0) == 0
    nt = S_.plan_info(N, DT)[0]
    ws = np.full(lib.ffcsim_upw(N) * H * nt * 2048, np.nan, np.float32)
    nslab = lib.ffcsim_conv_bwd_dkf_os(N, DT, S_.p(db), S_.p(xb), S_.p(ws), B, H, L)
    assert nslab == 1
    dk = np.full((H, P), np.nan, np.float32)
    assert lib.ffcsim_kernel_ifft_grad(N, DT, S_.p(ws), nslab, H, P, S_.p(dk)) == 0
    errs = {"out": _rel(S_.from_bits(y, DT), want[0]), "dx": _rel(S_.from_bits(dx, DT), want[1]), "dk": _rel(dk, want[2])}
    print(f"\npartial_os_sim L={L} P={P}: " + "  ".join(f"{nm} {v:.2e}" for nm, v in errs.items()), end="")
    for nm, tol in (("out", 2e-2), ("dx", 2e-2), ("dk", 2e-2)):      # the suite's bf16 gate (tests/test_flashfftconv_gpu.py REL)
        assert errs[nm] < tol, (nm, errs[nm])


def test_other_sizes_are_refused():
    """no outer digit, no history half: fft 1024 has no blocked form (-8: the library has no kernel for the call)"""
    z = np.zeros((1, 1, 1024), np.uint16)
    kf = S_.sim_kernel_fft(1024, DT, np.ones((1, 4), np.float32))
    assert S_.lib().ffcsim_conv_fwd_os(1024, DT, S_.p(z), S_.p(kf), S_.p(z.copy()), 1, 1, 1024, 0, 1) == -8


def test_module_copies_and_refuses_what_it_cannot_run():
    """host side of PartialFFTConv(overlap_save=True): deep copy and pickle, CPU tensors, and a row so long that a 32-bit index one window
    past its end would wrap (the library and the simulator refuse the same: -2)"""
    import copy, pickle
    import torch
    from flashfftconv import PartialFFTConv
    mod = PartialFFTConv(64, overlap_save=True)
    assert copy.deepcopy(mod).overlap_save and pickle.loads(pickle.dumps(mod)).N_partial == 64
    assert not PartialFFTConv(64).overlap_save
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        mod(torch.zeros(1, 2, 5000, dtype=torch.bfloat16), torch.zeros(2, 64))
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        mod(torch.empty(1, 1, 2 ** 31 - 4096, dtype=torch.bfloat16, device="meta"), torch.empty(1, 64, device="meta"))
    assert S_.lib().ffcsim_conv_fwd_os(N, DT, None, None, None, 1, 1, 2 ** 31 - 4096, 0, 1) == -2
