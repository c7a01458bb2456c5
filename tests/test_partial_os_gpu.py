"""PartialFFTConv(P, overlap_save=True): rows cut into blocks of S samples on the fused kernel of fft size N' = 2 S (ffc_conv_fwd_os,
ffc_conv_bwd_dkf_os).  Forward, dx and dk against the float64 linear convolution (oracle.ref_partial_keeps), worst row against the suite's
gates (sparse_inputs.gates).  Per N': the smallest and the largest P that select it; L = S + 1 (one sample in the second block), 3 S - 5
(element-wise arm, a block before the ragged one; B * nblk odd: the last pair has one plane) and 4 S (16-byte path)."""
import pytest
import torch

from oracle import ref_fft_conv as O
import sparse_inputs as SI
from test_sparse_gpu import _to_gpu, _fwd_bwd, _errs, _check, BF, FP

pytestmark = pytest.mark.gpu


def _run(monkeypatch, P_list, L, Lk, B, H, dtype, k_dtype=torch.float32, route=True):
    """one module per P on shared inputs and one oracle call; the forward / dx launches (fft size, conj, wrap) and the dk_f launch (fft size)
    of every module are recorded"""
    from flashfftconv import PartialFFTConv, sparse_conv as SC
    x, k, dout = SI.white_inputs(L, Lk, B, H, seed=L + 7 * Lk + B + int(dtype == FP))
    (xg, kg, dg), host = _to_gpu(x, k, SI.tie_to(dout, x), dtype)
    kg = kg.to(k_dtype)
    want = O.ref_partial_keeps(host[0], kg.double().cpu().numpy(), host[2], P_list)
    calls, conv_os, dkf_os = [], SC._conv_os, SC._dkf_os
    monkeypatch.setattr(SC, "_conv_os", lambda plan, t, kf, conj, wrap: (calls.append((plan.seqlen, conj, wrap)), conv_os(plan, t, kf, conj, wrap))[1])
    monkeypatch.setattr(SC, "_dkf_os", lambda plan, dy, t: (calls.append(plan.seqlen), dkf_os(plan, dy, t))[1])
    for P in P_list:
        calls.clear()
        mod = PartialFFTConv(P, overlap_save=True).to("cuda")
        got = _fwd_bwd(mod, xg, kg, dg)
        n = SC.os_fft_size(min(P, Lk))
        assert calls == ([(n, False, True), (n, True, False), n] if route else []), (P, calls)
        assert bool(mod._convs) != route
        assert not bool(got[2][..., P:].any()), f"P = {P}: dk beyond the taps is not zero"
        errs = _errs(got, want[P])
        print(f"\npartial_os L={L} P={P} B={B} H={H} {SI.DT_NAME[dtype]}: " + "  ".join(f"{nm} {v:.2e}" for nm, v in errs.items()), end="")
        _check(errs, SI.gates(dtype), f"L = {L}, P = {P}")


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,H", [(1, 3), (3, 2)])
@pytest.mark.parametrize("Lform", ["S+1", "3S-5", "4S"])
@pytest.mark.parametrize("N", [4096, 8192, 16384, 32768])
def test_blocked_route_against_the_oracle(N, Lform, B, H, dtype, monkeypatch):
    S = N // 2
    L = {"S+1": S + 1, "3S-5": 3 * S - 5, "4S": 4 * S}[Lform]
    taps = [S // 2 + 1, S] + ([1] if (N, Lform, B) == (4096, "3S-5", 3) else [])
    _run(monkeypatch, taps, L, S + 9, B, H, dtype)


def test_bf16_filter(monkeypatch):
    _run(monkeypatch, [1500], 3 * 2048 - 5, 1509, 3, 2, BF, k_dtype=BF)


def test_one_block_of_an_unsupported_length(monkeypatch):
    """L = 1000: 2 L is no fft size, today's route raises; here one block of fft 4096"""
    _run(monkeypatch, [64], 1000, 100, 3, 2, BF)


def test_long_filter_keeps_the_2L_route(monkeypatch):
    """more than 16384 taps: no block size with an outer digit holds them, fft size 2 L = 65536 as without the flag"""
    _run(monkeypatch, [16400], 32768, 16409, 1, 1, BF, route=False)

