"""The checker of tests/rowcheck.py on the CPU: the float64 oracle rounded once to the module dtype stands in for a correct kernel and must pass
the three assertions (tied heads, per row, per element) without exception; each corruption below must fail the assertion that is there for
it.  The first two -- one sample replaced by its neighbour, the last 8 samples of one row zeroed -- PASS the suite's whole-tensor gate
(rel < REL[dtype], asserted here): that is why the per-element bound exists.

Shape: B = 3, 16 heads tiled from 8, L = 4096 at fft 8192, unit-scale inputs and gates, a 37-tap filter that does not decay.  With so short
a filter the rows of y are stationary, so that the 8 zeroed samples carry 8 / 4096 of their row's energy: sqrt(8 / (48 * 4096)) = 0.64 % of
the 48-row tensor in the mean, 0.2 .. 0.4 % on the row with the weakest tail, which is the one taken -- below the fp16 gate of 0.5 % even
on a tensor this small (on the 2048 rows of a training step it is 0.1 %)."""
import numpy as np
import pytest
import torch

import rowcheck as RC
from test_flashfftconv_gpu import REL, rel

B, H, L, LK, N = 3, 16, 4096, 37, 8192
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
_CASES = {}


def _case(dtype, gated):
    """inputs on the 8 representative heads, the oracle, and the stand-in result over all 16 heads (never modified: corruptions work on clones)"""
    key = (dtype, gated)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7 + int(gated) + 2 * int(dtype == torch.float16))
        u, dout, pre, post = (torch.randn(B, RC.P, L, generator=g).to(dtype).double().numpy() for _ in range(4))
        k = (torch.randn(RC.P, LK, generator=g) * 0.1).double().numpy()
        want = RC.oracle(u, k, dout, N, *((pre, post) if gated else ()))
        pi = RC.head_map(H, seed=3)
        good = {nm: RC.tile(torch.from_numpy(w).to(torch.float32 if nm == "dk" else dtype), pi, 0 if nm == "dk" else 1) for nm, w in want.want.items()}
        _CASES[key] = (want, pi, good)
    return _CASES[key]


def _corrupted(good, name, fn):
    got = dict(good)
    got[name] = good[name].clone()
    fn(got[name])
    return got


def test_head_map():
    pi = RC.head_map(1032, seed=5)
    assert list(pi[:8]) == list(range(8)) and pi.min() == 0 and pi.max() == 7
    assert not np.array_equal(pi, np.arange(1032) % 8)
    assert np.array_equal(pi, RC.head_map(1032, seed=5)) and not np.array_equal(pi, RC.head_map(1032, seed=6))
    assert min(np.bincount(pi, minlength=8)) > 1032 // 16                       # every representative carries its share of the heads
    assert len({(int(pi[h]), int(pi[h + 1])) for h in range(8, 1031)}) > 32       # neighbours do not repeat a pattern
    assert list(RC.head_map(3)) == [0, 1, 2]


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32], ids=IDS + ["fp32"])
def test_ulp_is_the_step_to_the_next_number(dtype):
    ints = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}[dtype]
    x = torch.tensor([1.0, 1.5, 1.999, 2.0, 0.75, 3e-3, 6.2e-5, 6.0e-5, 1e-7, 100.0, 40000.0], dtype=torch.float64).to(dtype)
    nxt = (x.view(ints) + 1).view(dtype)
    assert np.array_equal(RC.ulp(x.double().numpy(), dtype), (nxt.double() - x.double()).numpy())
    assert RC.ulp(np.zeros(1), torch.float16)[0] == 2.0 ** -24 and np.array_equal(RC.ulp(-x.double().numpy(), dtype), RC.ulp(x.double().numpy(), dtype))


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_rounded_oracle_passes(dtype, gated):
    want, pi, good = _case(dtype, gated)
    assert set(good) == set(RC.NAMES if gated else RC.NAMES[:3])
    rep = RC.check(good, want, pi, dtype, gated)
    print(rep.line())
    rep.assert_ok("oracle rounded once")
    tol = RC.gates(dtype, gated)
    for nm in good:
        assert rep.row[nm] < tol[nm] / 4 and rep.elem[nm] <= 1.0


def test_the_gated_oracle_parts():
    """c and dv as ref_grads(parts=True) returns them are the rows the gated results are built from"""
    from oracle import ref_fft_conv as O
    g = np.random.RandomState(0)
    u, pre, post, dout = (g.randn(2, 3, 100) for _ in range(4))
    k = g.randn(3, 60)
    du, dk, dpre, dpost, dv, c = O.ref_grads(u, k, dout, 256, pre, post, parts=True)
    assert np.array_equal(c, O.ref_fft_conv(u * pre, k, 256)) and np.array_equal(c * post, O.ref_fft_conv_gated(u, k, pre, post, 256))
    assert np.array_equal(du, dv * pre) and np.array_equal(dpre, dv * u) and np.array_equal(dpost, dout * c)
    assert np.array_equal(dv, O.ref_grads(u * pre, k, dout * post, 256)[0])
    assert len(O.ref_grads(u, k, dout, 256, pre, post)) == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_sample_replaced_by_its_neighbour(dtype):
    want, pi, good = _case(dtype, False)
    b, h = 1, 3
    row = want.want["y"][b, h]
    step, rms = np.abs(np.diff(row)), np.sqrt(np.mean(row * row))
    t = int(np.argmax((step >= rms) & (step <= 1.5 * rms)))      # an ordinary pair of neighbours: 1 .. 1.5 rms apart
    assert rms <= step[t] <= 1.5 * rms

    def fn(y):
        y[b, h, t] = y[b, h, t + 1]
    got = _corrupted(good, "y", fn)
    old = rel(got["y"], RC.tile(torch.from_numpy(want.want["y"]), pi, 1))
    print(f"whole-tensor rel {old:.3e} (gate {REL[dtype]:.0e})")
    assert old < REL[dtype], "the whole-tensor gate was expected to pass this"
    rep = RC.check(got, want, pi, dtype, False)
    assert "element" in rep.kinds("y") and not rep.kinds("du") and not rep.kinds("dk"), rep.failures
    assert f"first at (b, h, t) = ({b}, {h}, {t})" in [m for k, nm, m in rep.failures if k == "element"][0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_last_samples_of_a_row_zeroed(dtype):
    want, pi, good = _case(dtype, False)
    tail = (want.want["y"][..., -8:] ** 2).sum(-1)               # (B, 8): the row with the weakest tail
    b, h = (int(v) for v in np.unravel_index(int(np.argmin(tail)), tail.shape))

    def fn(y):
        y[b, h, -8:] = 0
    got = _corrupted(good, "y", fn)
    old = rel(got["y"], RC.tile(torch.from_numpy(want.want["y"]), pi, 1))
    print(f"whole-tensor rel {old:.3e} (gate {REL[dtype]:.0e})")
    assert old < REL[dtype], "the whole-tensor gate was expected to pass this"
    rep = RC.check(got, want, pi, dtype, False)
    assert "element" in rep.kinds("y") and not rep.kinds("du") and not rep.kinds("dk"), rep.failures


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_rows_of_a_head_swapped(dtype):
    want, pi, good = _case(dtype, True)
    for nm in ("y", "du", "dpregate", "dpostgate"):
        def fn(t):
            t[[0, 1], 5] = t[[1, 0], 5]
        rep = RC.check(_corrupted(good, nm, fn), want, pi, dtype, True)
        assert "row" in rep.kinds(nm) and rep.kinds() == rep.kinds(nm), rep.failures


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_tied_head_with_another_heads_rows(dtype):
    want, pi, good = _case(dtype, False)
    h = 11
    other = int((pi[h] + 1) % RC.P)
    for nm in ("y", "du", "dk"):
        def fn(t):
            if nm == "dk":
                t[h] = t[other]
            else:
                t[:, h] = t[:, other]
        rep = RC.check(_corrupted(good, nm, fn), want, pi, dtype, False)
        assert [(k, n) for k, n, _ in rep.failures] == [("tied", nm)], rep.failures      # (the representative heads themselves are intact)
        assert "1 of 16 heads" in rep.failures[0][2] and f"head {h} carries representative {int(pi[h])}" in rep.failures[0][2]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_tied_head_one_ulp_off(dtype):
    want, pi, good = _case(dtype, False)

    def fn(y):
        y.view(torch.int16)[2, 13, 777] += 1
    rep = RC.check(_corrupted(good, "y", fn), want, pi, dtype, False)
    assert [(k, n) for k, n, _ in rep.failures] == [("tied", "y")], rep.failures
    assert "in 1 elements; first at (b, h, t) = (2, 13, 777)" in rep.failures[0][2]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_dk_row_scaled(dtype):
    want, pi, good = _case(dtype, False)

    def fn(dk):
        dk[2] *= 1.05
    rep = RC.check(_corrupted(good, "dk", fn), want, pi, dtype, False)
    assert "row" in rep.kinds("dk") and rep.kinds() == rep.kinds("dk"), rep.failures
    assert "at row h = 2" in [m for k, nm, m in rep.failures if k == "row"][0]
