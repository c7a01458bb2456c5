"""PartialFFTConv(P, overlap_save=True) with gates and a residual: y = postgate * conv(x * pregate, k[:, :P]) + residual on the gated blocked
kernels (ffc_conv_fwd_os_gated, ffc_conv_bwd_dkf_os_gated).  y, dx, dk, dpregate and dpostgate per row and per element against the float64
oracle (tests/rowcheck.py; fft size >= L + P: nothing wraps).  Per N': L = S + 1 (one sample in the second block), 3 S - 5 (element-wise arm,
a ragged last block, B * nblk odd) and 4 S (16-byte path); P = S and S / 2 + 1."""
import pytest
import torch

import rowcheck as RC
import sparse_inputs as SI
from test_sparse_gpu import BF, FP

pytestmark = pytest.mark.gpu
NAMES = ("x", "dout", "pre", "post", "res")


def _inputs(L, Lk, B, H, dtype, seed):
    """white rows on the representative heads (gates and residual drawn as x is), every other head a copy of its representative's"""
    nrep = min(H, RC.P)
    x, k, dout = SI.white_inputs(L, Lk, B, nrep, seed)
    pre, _, post = SI.white_inputs(L, 1, B, nrep, seed + 1)
    res = SI.white_inputs(L, 1, B, nrep, seed + 2)[0]
    pi = RC.head_map(H)
    d = {nm: RC.tile(torch.from_numpy(t).to("cuda").to(dtype), pi, 1) for nm, t in zip(NAMES, (x, SI.tie_to(dout, x), pre, post, res))}
    d["k"] = RC.tile(torch.from_numpy(k).to("cuda"), pi, 0)
    return d, pi


def _want(d, P, pre=True, post=True, res=True):
    """the oracle on the representative heads; a gate that the call leaves out is all ones"""
    nrep = min(d["x"].shape[1], RC.P)
    h = {nm: d[nm][:, :nrep].double().cpu().numpy() for nm in NAMES}
    k = d["k"][:nrep, :P].double().cpu().numpy()
    gates = () if not (pre or post) else tuple(h[nm] if on else h[nm] * 0 + 1 for nm, on in (("pre", pre), ("post", post)))
    return RC.oracle(h["x"], k, h["dout"], 1 << (h["x"].shape[-1] + P).bit_length(), *gates, residual=h["res"] if res else None)


def _step(mod, d, pre=True, post=True, res=True, only_k=False):
    leaf = lambda t, on=True: t.clone().requires_grad_(not only_k) if on else None
    x, k = leaf(d["x"]), d["k"].clone().requires_grad_(True)
    g = {"pregate": leaf(d["pre"], pre), "postgate": leaf(d["post"], post), "residual": leaf(d["res"], res)}
    y = mod(x, k, **g)
    y.backward(d["dout"])
    got = {"y": y.detach(), "du": x.grad, "dk": k.grad, "dpregate": pre and g["pregate"].grad, "dpostgate": post and g["postgate"].grad}
    return {nm: t for nm, t in got.items() if torch.is_tensor(t)}, g


def _check(got, want, pi, P, dtype, gated, what):
    assert not bool(got["dk"][:, P:].any()), f"{what}: dk beyond the taps is not zero"
    rep = RC.check(dict(got, dk=got["dk"][:, :P]), want, pi, dtype, gated=gated)
    print(f"\npartial_os_gated {what}: {rep.line()}", end="")
    rep.assert_ok(what)


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Lform", ["S+1", "3S-5", "4S"])
@pytest.mark.parametrize("N", [4096, 8192, 16384, 32768])
def test_gated_blocked_route_against_the_oracle(N, Lform, dtype):
    from flashfftconv import PartialFFTConv
    S = N // 2
    L = {"S+1": S + 1, "3S-5": 3 * S - 5, "4S": 4 * S}[Lform]
    d, pi = _inputs(L, S + 9, 3, 2, dtype, seed=L + int(dtype == FP))
    for P in (S // 2 + 1, S):
        got, _ = _step(PartialFFTConv(P, overlap_save=True).to("cuda"), d)
        assert set(got) == set(RC.NAMES)
        _check(got, _want(d, P), pi, P, dtype, True, f"N'={N} L={L} P={P} {SI.DT_NAME[dtype]}")


@pytest.fixture
def launches(monkeypatch):
    """(conj, wrap, gate2 given) of every ffc_conv_fwd_os_gated call and "dkf" for every ffc_conv_bwd_dkf_os_gated call of the module"""
    from flashfftconv import sparse_conv as SC
    calls, conv, dkf = [], SC._conv_os_gated, SC._dkf_os_gated
    monkeypatch.setattr(SC, "_conv_os_gated", lambda plan, x, kf, conj, wrap, *g: (calls.append((conj, wrap, len(g) > 3 and g[3] is not None)), conv(plan, x, kf, conj, wrap, *g))[1])
    monkeypatch.setattr(SC, "_dkf_os_gated", lambda *a: (calls.append("dkf"), dkf(*a))[1])
    return calls


@pytest.mark.parametrize("pre,post,res", [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1)], ids=["pregate", "postgate", "both", "residual"])
def test_each_operand_on_its_own(pre, post, res, launches):
    """H = 11: three heads beyond the representatives (tied-head check).  A gate that is absent gets no gradient launch: no second output
    without a pregate, no dpostgate launch without a postgate; the residual's gradient is the incoming one."""
    from flashfftconv import PartialFFTConv
    S, P = 2048, 1025
    d, pi = _inputs(3 * S - 5, S + 9, 3, 11, BF, seed=11)
    got, g = _step(PartialFFTConv(P, overlap_save=True).to("cuda"), d, pre, post, res)
    assert launches == [(False, True, False), (True, False, bool(pre))] + [(False, True, False)] * post + ["dkf"]
    assert ("dpregate" in got, "dpostgate" in got) == (bool(pre), bool(post))
    if res:
        assert torch.equal(g["residual"].grad, d["dout"])
    _check(got, _want(d, P, pre, post, res), pi, P, BF, bool(pre or post), f"pre={pre} post={post} res={res}")


def test_only_k_requires_grad(launches):
    from flashfftconv import PartialFFTConv
    S, P = 2048, 1025
    d, _ = _inputs(3 * S - 5, S + 9, 3, 2, BF, seed=12)
    mod = PartialFFTConv(P, overlap_save=True).to("cuda")
    full, _ = _step(mod, d)
    launches.clear()
    got, _ = _step(mod, d, only_k=True)
    assert launches == [(False, True, False), "dkf"] and set(got) == {"y", "dk"}
    assert torch.equal(got["dk"], full["dk"]) and torch.equal(got["y"], full["y"])
