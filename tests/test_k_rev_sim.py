"""Bidirectional filters on the CPU wave simulator: the two-tensor forms of the k -> k_f and dk_f -> dk kernels (Modes::kfft / Modes::dkifft on
KfBiArgs / DkBiArgs) against the one-tensor kernels on the dense row

    k_full[h, n] = (n < Lk ? k[h, n] : 0) + (N-1-n < Lr ? kr[h, N-1-n] : 0)

bit for bit: k_f of (k, kr) is k_f of k_full, and (dk, dk_rev) are the slices dk_full[:, :Lk] and flip(dk_full)[:, :Lr] of the dense inverse."""
import functools
import os, sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simlib as S

SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072)
SINGLE_TILE_G = {256: 4, 512: 2, 1024: 1, 2048: 1}      # heads per tile (Geo::G)
SENTINEL = np.float32(-12345.75)
PAD = 16


def heads(N):
    """the last tile / workgroup partly filled: G + 1 heads at the single-tile sizes, UPW + 1 elsewhere, at most 2 at 65536 / 131072"""
    if N in SINGLE_TILE_G:
        return SINGLE_TILE_G[N] + 1
    return min(S.lib().ffcsim_upw(N) + 1, 2) if N >= 65536 else S.lib().ffcsim_upw(N) + 1


def cases(N):
    return (("half", N // 2, N // 2),                 # the caller's case
            ("odd", N // 2 - 3, N // 2 - 5),          # per-element path
            ("k4", 4, N - 4),
            ("lr1", N // 2, 1),
            ("lk1", 1, N // 2),
            ("overlap4", 3 * N // 4, N // 2),         # Lk + Lr > N, both % 4 == 0
            ("overlap_odd", 3 * N // 4 + 1, N // 2 + 3),
            ("lr_full", N // 2, N))


def k_full_of(k, kr, N):
    H, Lk = k.shape
    Lr = kr.shape[1]
    a = np.zeros((H, N), np.float32)
    b = np.zeros((H, N), np.float32)
    a[:, :Lk] = k
    b[:, N - Lr:] = kr[:, ::-1]
    return a + b          # fp32 sum, as the kernel's


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def kernel_fft_bi(N, dt, k, kr):
    H, Lk = k.shape
    nt = S.plan_info(N, dt)[0]
    kf = np.zeros((H, nt * 1024, 2), np.uint16)
    rc = S.lib().ffcsim_kernel_fft_bi(N, dt, S.p(k), Lk, S.p(kr), kr.shape[1], H, S.p(kf))
    assert rc == 0, rc
    return kf


@pytest.mark.parametrize("dt", [S.DT_BF16, S.DT_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("N", SIZES)
def test_kernel_fft_bi_is_kernel_fft_of_the_dense_row(N, dt):
    H = heads(N)
    for name, Lk, Lr in cases(N):
        rng = np.random.default_rng(N + 7 * Lk + Lr)
        k = rng.standard_normal((H, Lk)).astype(np.float32)
        kr = rng.standard_normal((H, Lr)).astype(np.float32)
        want = S.sim_kernel_fft(N, dt, k_full_of(k, kr, N))
        got = kernel_fft_bi(N, dt, k, kr)
        assert np.array_equal(got, want), (N, name, int((got != want).sum()))


@functools.lru_cache(maxsize=None)
def slabs_and_dense(N, nslab):
    """seeded fp32 dk_f slabs [nslab][H (x passes)][kf_elems][2] and the dense inverse of their sum, dk_full (H, N); shared, read-only"""
    H = heads(N)
    nt = S.plan_info(N, S.DT_BF16)[0]
    rng = np.random.default_rng(1000 + N + nslab)
    ws = rng.standard_normal(nslab * H * nt * 2048).astype(np.float32)
    full = np.full((H, N), np.nan, np.float32)
    rc = S.lib().ffcsim_kernel_ifft_grad(N, S.DT_BF16, S.p(ws), nslab, H, N, S.p(full))
    assert rc == 0, rc
    assert not np.isnan(full).any()
    ws.setflags(write=False); full.setflags(write=False)
    return ws, full


@pytest.mark.parametrize("nslab", [1, 2])
@pytest.mark.parametrize("N", SIZES)
def test_kernel_ifft_grad_bi_is_the_two_slices_of_the_dense_inverse(N, nslab):
    H = heads(N)
    ws, full = slabs_and_dense(N, nslab)
    for name, Lk, Lr in cases(N):
        dk = np.full(H * Lk + PAD, SENTINEL, np.float32)
        dkr = np.full(H * Lr + PAD, SENTINEL, np.float32)
        rc = S.lib().ffcsim_kernel_ifft_grad_bi(N, S.DT_BF16, S.p(ws), nslab, H, Lk, S.p(dk), Lr, S.p(dkr))
        assert rc == 0, rc
        assert np.array_equal(bits(dk[:H * Lk].reshape(H, Lk)), bits(full[:, :Lk])), (N, name, "dk")
        assert np.array_equal(bits(dkr[:H * Lr].reshape(H, Lr)), bits(full[:, ::-1][:, :Lr])), (N, name, "dk_rev")
        assert (dk[H * Lk:] == SENTINEL).all() and (dkr[H * Lr:] == SENTINEL).all(), (N, name, "wrote behind its rows")


def test_null_or_oversized_tensors_are_refused():
    N, H = 1024, 2
    k = np.zeros((H, 8), np.float32)
    kf = np.zeros((H, 1024, 2), np.uint16)
    assert S.lib().ffcsim_kernel_fft_bi(N, S.DT_BF16, S.p(k), 8, None, 8, H, S.p(kf)) != 0
    big = np.zeros((H, N + 4), np.float32)
    assert S.lib().ffcsim_kernel_fft_bi(N, S.DT_BF16, S.p(k), 8, S.p(big), N + 4, H, S.p(kf)) != 0
