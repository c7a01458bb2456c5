"""PartialFFTConv(P, overlap_save=True)(.., state=, return_state=): a row fed in chunks that carry S = N' / 2 samples of x * pregate from call
to call (ffc_conv_fwd_os_hist, ffc_conv_bwd_dkf_os_hist) against the float64 oracle on the WHOLE row (tests/rowcheck.py), with the inputs,
gates and bounds of tests/test_partial_os_gated_gpu.py.  Chunks of S / 2 + 3 (shorter than a state: the new state keeps part of the old
one), S + 1 (one sample in a second block), 2 S - 5 (element-wise arm, ragged last block) and S / 2 + 8: a multiple of 8, so the last chunk
runs every launch (forward, input gradient with block -1, dpostgate, dk_f) on the 16-byte arm behind a history.  That makes L = 4 S + 7;
with L = 4 S + 3 the remainder would be S / 2 + 4 and no chunk would leave the element-wise arm.  One backward over all chunks, so every
gradient passes through every state."""
import numpy as np
import pytest
import torch

import rowcheck as RC
import sparse_inputs as SI
from test_sparse_gpu import BF, FP

pytestmark = pytest.mark.gpu
B, H, NAMES = 3, 2, ("x", "dout", "pre", "post", "res")


def _inputs(L, Lk, dtype, seed):
    """white x, dout (tied to x), gates and residual as tests/test_partial_os_gated_gpu.py draws them; H <= rowcheck.P: every head is checked"""
    x, k, dout = SI.white_inputs(L, Lk, B, H, seed)
    pre, _, post = SI.white_inputs(L, 1, B, H, seed + 1)
    res = SI.white_inputs(L, 1, B, H, seed + 2)[0]
    d = {nm: torch.from_numpy(t).to("cuda").to(dtype) for nm, t in zip(NAMES, (x, SI.tie_to(dout, x), pre, post, res))}
    return dict(d, k=torch.from_numpy(k).to("cuda")), RC.head_map(H)


def _check(got, d, pi, P, dtype, gated, what):
    """got against the oracle on the whole row (fft size >= L + P: nothing wraps), per row and per element"""
    h = {nm: d[nm].double().cpu().numpy() for nm in NAMES}
    want = RC.oracle(h["x"], d["k"][:, :P].double().cpu().numpy(), h["dout"], 1 << (h["x"].shape[-1] + P).bit_length(),
                     *((h["pre"], h["post"]) if gated else ()), residual=h["res"] if gated else None)
    assert not bool(got["dk"][:, P:].any()), f"{what}: dk beyond the taps is not zero"
    rep = RC.check(dict(got, dk=got["dk"][:, :P]), want, pi, dtype, gated=gated)
    print(f"\npartial_os_state {what}: {rep.line()}", end="")
    rep.assert_ok(what)


def _chunked(mod, d, cuts, gated, state=None):
    """the row of d through mod in chunks that end at `cuts`, the state threaded through -> (got as _check takes it, last state)"""
    leaf = lambda t: t.clone().requires_grad_(True)
    x, k = leaf(d["x"]), leaf(d["k"])
    g = {nm: leaf(d[key]) for nm, key in (("pregate", "pre"), ("postgate", "post"), ("residual", "res"))} if gated else {}
    ys, a = [], 0
    for b in cuts:
        y, state = mod(x[..., a:b], k, **{nm: t[..., a:b] for nm, t in g.items()}, state=state, return_state=True)
        ys.append(y)
        a = b
    torch.autograd.backward(ys, [d["dout"][..., a:b] for a, b in zip((0,) + tuple(cuts), cuts)])
    got = {"y": torch.cat(ys, -1).detach(), "du": x.grad, "dk": k.grad}
    if gated:
        got.update(dpregate=g["pregate"].grad, dpostgate=g["postgate"].grad)
    return got, state


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", [4096, 8192, 16384, 32768])
def test_chunks_with_a_state_against_the_oracle_on_the_whole_row(N, dtype, gated):
    from flashfftconv import PartialFFTConv
    S, L = N // 2, 2 * N + 7
    cuts = (S // 2 + 3, 3 * S // 2 + 4, 7 * S // 2 - 1, L)
    d, pi = _inputs(L, S + 9, dtype, seed=L + int(dtype == FP))
    for P in (S // 2 + 1, S):
        mod = PartialFFTConv(P, overlap_save=True).to("cuda")
        assert mod.state_len == S
        got, state = _chunked(mod, d, cuts, gated)
        assert torch.equal(state, (d["x"] * d["pre"] if gated else d["x"])[..., -S:])
        _check(got, d, pi, P, dtype, gated, f"N'={N} P={P} {SI.DT_NAME[dtype]} gated={gated}")


@pytest.fixture
def launches(monkeypatch):
    """the name of every launcher call of the module; for _conv_os_hist (name, conj, wrap, a state gradient came back)"""
    from flashfftconv import sparse_conv as SC
    calls = []

    def spy(nm, fn):
        def run(*a, **kw):
            out = fn(*a, **kw)
            calls.append((nm, a[3], a[4], out[2] is not None) if nm == "_conv_os_hist" else nm)
            return out
        monkeypatch.setattr(SC, nm, run)
    for nm in ("_conv_os", "_dkf_os", "_conv_os_gated", "_dkf_os_gated", "_conv_os_hist", "_dkf_os_hist"):
        spy(nm, getattr(SC, nm))
    return calls


def test_state_gradient_on_its_own(launches):
    """one chunk of S + 1 samples behind a random state: state.grad[n] = sum_s k[s] (dout * postgate)[n - S + s] in float64; without a
    gradient for the state the input-gradient launch runs no block -1"""
    from flashfftconv import PartialFFTConv
    S, P = 2048, 1025
    d, pi = _inputs(S + 1, S + 9, BF, seed=21)
    mod = PartialFFTConv(P, overlap_save=True).to("cuda")
    state = torch.randn(B, H, S, device="cuda").to(BF)
    for want_grad in (True, False):
        launches.clear()
        st, x, k = state.clone().requires_grad_(want_grad), d["x"].clone().requires_grad_(True), d["k"].clone().requires_grad_(True)
        mod(x, k, d["pre"], d["post"], state=st).backward(d["dout"])
        assert launches == [("_conv_os_hist", False, True, False), ("_conv_os_hist", True, False, want_grad), "_dkf_os_hist"]
    g = (d["dout"].double() * d["post"].double()).cpu().numpy()
    kk = d["k"][:, :P].double().cpu().numpy()
    corr = np.stack([[np.concatenate((np.zeros(S), np.convolve(g[b, h], kk[h, ::-1])))[P - 1:P - 1 + S] for h in range(H)] for b in range(B)])
    launches.clear()
    st = state.clone().requires_grad_(True)
    mod(d["x"], d["k"], d["pre"], d["post"], state=st).backward(d["dout"])
    assert launches[1:] == [("_conv_os_hist", True, False, True)]      # nothing but the state wants a gradient
    rep = RC.check({"du": st.grad}, RC.Want({"du": corr}, {"du": RC.rms(corr)}), pi, BF, gated=True)
    print(f"\npartial_os_state dstate: {rep.line()}", end="")
    rep.assert_ok("state.grad")


@pytest.mark.parametrize("N", [4096, 32768])
def test_chunks_are_bit_identical_to_the_single_call(N):
    """L = 4 S in chunks of 2 S: every pair of planes holds the same two windows as in the call on the whole row"""
    from flashfftconv import PartialFFTConv
    S = N // 2
    d, _ = _inputs(4 * S, S, BF, seed=N)
    mod = PartialFFTConv(S, overlap_save=True).to("cuda")
    with torch.no_grad():
        whole = mod(d["x"], d["k"], pregate=d["pre"])
        y0, state = mod(d["x"][..., :2 * S], d["k"], pregate=d["pre"][..., :2 * S], return_state=True)
        y1 = mod(d["x"][..., 2 * S:], d["k"], pregate=d["pre"][..., 2 * S:], state=state)
    assert torch.equal(torch.cat((y0, y1), -1), whole)


def test_default_call_makes_the_launches_it_made(launches):
    from flashfftconv import PartialFFTConv
    d, _ = _inputs(3 * 2048 - 5, 1025, BF, seed=5)
    mod = PartialFFTConv(1025, overlap_save=True).to("cuda")
    x, k = d["x"].clone().requires_grad_(True), d["k"].clone().requires_grad_(True)
    mod(x, k).backward(d["dout"])
    mod(x, k, d["pre"], d["post"], d["res"]).backward(d["dout"])
    assert launches == ["_conv_os", "_conv_os", "_dkf_os", "_conv_os_gated", "_conv_os_gated", "_dkf_os_gated"]


def test_refusals():
    from flashfftconv import PartialFFTConv
    x, k = torch.zeros(B, H, 3000, dtype=BF, device="cuda"), torch.zeros(H, 64, device="cuda")
    ok = torch.zeros(B, H, 2048, dtype=BF, device="cuda")
    for kw in ({"state": ok}, {"return_state": True}):
        with pytest.raises(RuntimeError, match="overlap_save=True"):
            PartialFFTConv(64)(x, k, **kw)
    mod = PartialFFTConv(64, overlap_save=True).to("cuda")
    bad = (ok[..., :-8], ok[:2], ok.to(FP), ok.cpu(), torch.zeros(B, H, 4096, dtype=BF, device="cuda")[..., ::2])
    for state in bad:
        with pytest.raises(RuntimeError, match="state"):
            mod(x, k, state=state)
