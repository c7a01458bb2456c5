"""The inputs of tests/test_sparse_gpu.py, checked without a GPU: the tone recipe (tests/sparse_inputs.py) stays within the magnitudes the suite
already runs and keeps the oracle's results for neighbouring mask edges far apart -- an edit of the recipe that made the GPU test vacuous fails
here -- and the oracle helpers that share transforms between several keeps return what the one-keep functions return."""
import numpy as np
import pytest
import torch

from oracle import ref_fft_conv as O
import sparse_inputs as SI


@pytest.mark.parametrize("L,Lk,f0s", [(128, 128, (3, 125)), (8192, 8192, (37, 511, 512, 8189)), (131072, 131072, (37, 3 * 16 - 1, 131069)),
                                       (65536, 131072, (3, 11 * 32, 65533)), (65536, 98304, (3, 11 * 32 - 1, 65533))])
def test_tone_recipe_peak_and_separation(L, Lk, f0s):
    N, B, H = 2 * L, 2, 2
    for f0 in f0s:
        x, k, dout = SI.tone_inputs(L, Lk, B, H, f0, seed=L + f0)
        for t, s in ((x, 1.0), (dout, 1.0), (k, 0.1)):
            for row in t.reshape(-1, t.shape[-1]):
                p = SI.peak_over_white_rms(row, N, s)
                assert 3.0 <= p <= 5.0, f"f0 = {f0}: largest bin {p:.2f} x the rms bin of a white row of that length"
        # dk sums the batch: its terms must not cancel (sparse_inputs: one phase offset between x and dout for all b), or dk's relative error measures the cancellation
        terms = np.stack([O.ref_freq_sparse_conv(x[b:b + 1], k, 2 * f0 + 2, dout[b:b + 1])[2] for b in range(B)])
        whole = O.ref_freq_sparse_conv(x, k, 2 * f0 + 2, dout)[2]
        cancel = np.sqrt((np.linalg.norm(terms, axis=-1) ** 2).sum(0)) / np.linalg.norm(whole, axis=-1)
        assert cancel.max() < 1.0, f"f0 = {f0}: sqrt(sum_b |dk_b|^2) / |dk| = {cancel.max():.2f} on the worst head"
        for dtype in (torch.bfloat16, torch.float16):
            nm = SI.DT_NAME[dtype]
            want = O.ref_freq_sparse_keeps(O.round_to(x, nm), k, O.round_to(dout, nm), (f0, f0 + 1, f0 + 2))
            SI.assert_separated(want, f0, dtype, k_fills_grid=Lk == N)


@pytest.mark.parametrize("L,Lk", [(64, 64), (512, 1024), (4096, 1000)])
def test_shared_transform_oracles_match_the_one_keep_oracles(L, Lk):
    rng = np.random.default_rng(L + Lk)
    x, dout = (rng.standard_normal((3, 2, L)) for _ in range(2))
    k = rng.standard_normal((2, Lk))
    keeps = (0, 1, 2, 3, 9, L // 3, L // 3 + 1, L - 1, L, L + 1, L + 7)      # L + 1 bins: all of them, Nyquist included
    got = O.ref_freq_sparse_keeps(x, k, dout, keeps)
    for keep in keeps:
        for a, b in zip(got[keep], O.ref_freq_sparse_conv(x, k, 2 * keep, dout)):
            assert a.shape == b.shape and np.abs(a - b).max() < 1e-11 * max(np.abs(b).max(), 1.0), keep
    taps = (1, 7, Lk - 1, Lk, Lk + 5)
    got = O.ref_partial_keeps(x, k, dout, taps)
    for P in taps:
        y = O.ref_partial_conv(x, k, P)
        dx, dk = O.ref_grads(x, k[..., :P], dout, 2 * L)
        assert np.abs(got[P][0] - y).max() < 1e-11 and np.abs(got[P][1] - dx).max() < 1e-11
        assert got[P][2].shape == k.shape and np.abs(got[P][2][..., :P] - dk).max() < 1e-10 and not got[P][2][..., P:].any()
