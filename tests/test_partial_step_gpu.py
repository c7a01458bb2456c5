"""PartialFFTConv(P, overlap_save="direct"): stateful pieces of 1 .. 64 samples on the direct step kernels (ffc_partial_step_fwd / _bwd),
behind a prompt prefilled on the blocked route, against the float64 oracle on the WHOLE row with the inputs, checker and bounds of
tests/test_partial_os_state_gpu.py.  Pieces S + 5 (blocked), then 1, 7, 8, 64, 3 (direct: one sample, odd, one tile, the longest step with
8 tiles, a ragged last one); one backward over all pieces, so every gradient crosses every state and the boundary of the two routes."""
import numpy as np
import pytest
import torch

import rowcheck as RC
import sparse_inputs as SI
import test_partial_os_state_gpu as T
from test_sparse_gpu import BF, FP

pytestmark = pytest.mark.gpu
STEPS = (1, 7, 8, 64, 3)
OS = ("_conv_os", "_dkf_os", "_conv_os_gated", "_dkf_os_gated", "_conv_os_hist", "_dkf_os_hist")


@pytest.fixture
def calls(monkeypatch):
    """the name of every launcher call of the module, the step launchers included"""
    from flashfftconv import sparse_conv as SC
    seen = []

    def spy(nm, fn):
        def run(*a, **kw):
            seen.append(nm)
            return fn(*a, **kw)
        monkeypatch.setattr(SC, nm, run)
    for nm in OS + ("_step_fwd", "_step_bwd"):
        spy(nm, getattr(SC, nm))
    return seen


def _cuts(S):
    return tuple(np.cumsum((S + 5,) + STEPS).tolist())


# P: one tap, fewer taps than lanes, a ragged chunk, taps = S, the step to S = 4096; then the largest chunk (64 taps per lane), taps set by
# k's length, and B = 8: the smallest batch that the host splits at H = 2 (two slices of 4 rows, ffc_partial_step_split)
CASES = [(P, P + 9, 3, dt, g) for P in (1, 3, 1025, 2048, 2049) for dt in (BF, FP) for g in (False, True)]
CASES += [(16384, 16384, 3, BF, True), (2048, 700, 3, BF, True), (1025, 1034, 8, FP, True)]


@pytest.mark.parametrize("P,Lk,nb,dtype,gated", CASES, ids=lambda v: SI.DT_NAME.get(v, str(v)))
def test_prefill_then_steps_against_the_oracle_on_the_whole_row(P, Lk, nb, dtype, gated, calls, monkeypatch):
    from flashfftconv import PartialFFTConv
    monkeypatch.setattr(T, "B", nb)
    mod = PartialFFTConv(P, overlap_save="direct").to("cuda")
    S = mod.state_len
    cuts = _cuts(S)
    # seed base 2, chosen on the float64 oracle alone: the one tap of a gated P = 1 call is a sum of B L products of random sign (the gates
    # remove the mean that sparse_inputs.tie_to gives the ungated call) and with base 0 head 1 draws |dk| = 0.001 sqrt(B L), below the
    # rounding of the bf16 inputs themselves on either route; with base 2 every dk row of P = 1, 3 has rms >= 0.2 sqrt(B L)
    d, pi = T._inputs(cuts[-1], Lk, dtype, seed=2 + P + nb + int(dtype == FP))
    got, state = T._chunked(mod, d, cuts, gated)
    # the prefill's launches and nothing else of the blocked route: every short piece was one step launch each way
    assert [c for c in calls if c in OS] == (["_conv_os_gated"] * 3 + ["_dkf_os_gated"] if gated else ["_conv_os", "_conv_os", "_dkf_os"])
    assert calls.count("_step_fwd") == len(STEPS) and calls.count("_step_bwd") == len(STEPS)
    assert torch.equal(state, (d["x"] * d["pre"] if gated else d["x"])[..., -S:])
    T._check(got, d, pi, min(P, Lk), dtype, gated, f"direct P={P} Lk={Lk} B={nb} {SI.DT_NAME[dtype]} gated={gated}")


@pytest.mark.parametrize("P", [3, 2049])
def test_state_after_every_step(P, calls):
    from flashfftconv import PartialFFTConv
    mod = PartialFFTConv(P, overlap_save="direct").to("cuda")
    S = mod.state_len
    d, _ = T._inputs(sum(STEPS), P + 9, BF, seed=P)
    state, a = torch.randn(T.B, T.H, S, device="cuda").to(BF), 0
    with torch.no_grad():
        x0, p0 = d["x"][..., :7], d["pre"][..., :7]
        none, zero = mod(x0, d["k"], p0, return_state=True), mod(x0, d["k"], p0, state=torch.zeros_like(state), return_state=True)
        assert torch.equal(none[0], zero[0]) and torch.equal(none[1], zero[1])
        for n in STEPS:
            x, pre, old = d["x"][..., a:a + n], d["pre"][..., a:a + n], state.clone()
            _, new = mod(x, d["k"], pre, d["post"][..., a:a + n], state=state, return_state=True)
            assert torch.equal(state, old)
            assert torch.equal(new, torch.cat((state, x * pre), -1)[..., -S:])
            state, a = new, a + n
    assert calls == ["_step_fwd"] * (2 + len(STEPS))


def test_state_gradient_on_its_own(calls):
    """one step of 64 samples behind a random state, nothing but the state wants a gradient: state.grad[i] = sum_t k[S + t - i] (dout * postgate)[t]
    in float64 (the formula of tests/test_partial_os_state_gpu.py) plus the gradient fed into new_state, shifted by L"""
    from flashfftconv import PartialFFTConv
    S, P, L = 2048, 1025, 64
    d, pi = T._inputs(L, S + 9, BF, seed=22)
    mod = PartialFFTConv(P, overlap_save="direct").to("cuda")
    st = torch.randn(T.B, T.H, S, device="cuda").to(BF).requires_grad_(True)
    dnew = torch.randn(T.B, T.H, S, device="cuda").to(BF)
    y, new = mod(d["x"], d["k"], d["pre"], d["post"], state=st, return_state=True)
    torch.autograd.backward([y, new], [d["dout"], dnew])
    assert calls == ["_step_fwd", "_step_bwd"]
    g = (d["dout"].double() * d["post"].double()).cpu().numpy()
    kk = d["k"][:, :P].double().cpu().numpy()
    corr = np.stack([[np.concatenate((np.zeros(S), np.convolve(g[b, h], kk[h, ::-1])))[P - 1:P - 1 + S] for h in range(T.H)] for b in range(T.B)])
    corr[..., L:] += dnew.double().cpu().numpy()[..., :S - L]
    rep = RC.check({"du": st.grad}, RC.Want({"du": corr}, {"du": RC.rms(corr)}), pi, BF, gated=True)
    print(f"\npartial_step dstate: {rep.line()}", end="")
    rep.assert_ok("state.grad")


def test_routing_edge_and_refusals(calls):
    from flashfftconv import PartialFFTConv, sparse_conv as SC
    S = 2048
    d, _ = T._inputs(3 * S - 5, 1025, BF, seed=6)
    x, k = d["x"], d["k"]
    state = torch.randn(T.B, T.H, S, device="cuda").to(BF)
    direct, blocked = PartialFFTConv(1025, overlap_save="direct").to("cuda"), PartialFFTConv(1025, overlap_save=True).to("cuda")
    with torch.no_grad():
        for mod, n, kw, want in ((direct, 64, {"state": state}, ["_step_fwd"]), (direct, 65, {"state": state}, ["_conv_os_hist"]),
                                 (blocked, 1, {"state": state}, ["_conv_os_hist"]), (direct, 3 * S - 5, {}, ["_conv_os"])):
            calls.clear()
            mod(x[..., :n], k, **kw)
            assert calls == want, (n, kw.keys())
        shifted = torch.zeros(state.numel() + 8, dtype=BF, device="cuda")[1:1 + state.numel()].view_as(state)
        for run in (lambda: direct(x[..., :4], k, state=shifted), lambda: direct(x[..., :0], k, state=state),
                    lambda: SC._step_fwd(x[..., :4].contiguous(), k, 1025, S, state=state, new_state=state)):
            with pytest.raises(RuntimeError):
                run()
