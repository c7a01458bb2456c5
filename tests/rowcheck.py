"""Per-row and per-element parity of a convolution result against the numpy float64 oracle (oracle/ref_fft_conv.py), for calls with many heads.

The whole-tensor relative L2 gates of the suite dilute what goes wrong in one place: one wrong sample in a row of 16384 is 0.8 % of that row
and far less of a tensor, one wrong (b, h) row among 2048 is 2.2 % of it.  Here the oracle is evaluated on a few REPRESENTATIVE heads (all
batch rows), the inputs of every other head are a copy of one representative's (head_map, tile), and three things are asserted per result
tensor (y, du, dk, dpregate, dpostgate):

  tied     head h of the result is bit-equal to the head of its representative: identical inputs through the same kernel instantiation give
           identical bits (k_f per head, the dk_f slabs of a head summed in a fixed order), so a mix-up of rows, a stale prefetch or a wait
           that is one short shows in every head the oracle does not see -- unless it mixes two heads of one representative (one in eight)
  row      on the representative heads, the worst relative L2 error over the (b, h) rows (dk: the h rows) stays below the suite's own gates
           (tests/test_flashfftconv_gpu.py REL; x 1.5 gated; dk max(REL, 1e-2))
  element  on the same rows |got_i - want_i| <= 4 * gate * s_i + ulp(want_i) for EVERY element.  The row gate bounds the rms error per sample by
           gate * rms(row); one sample of that noise stays below four times it (tests/test_half_rows_gpu.py).  s_i is the local scale of the
           noise, from the oracle: rms(want row) for the ungated y, du and for dk; where a gate multiplies the convolution's row sample by
           sample the noise of that row times the gate -- y: rms(c) |postgate_i|, du: rms(dv) |pregate_i|, dpregate: rms(dv) |u_i|,
           dpostgate: rms(c) |dout_i| (c = conv(u * pregate, k), dv = the gradient of u * pregate).  ulp(want_i), one unit in the last place
           of the result's dtype, covers the final rounding.  The measured error of the kernels is <= 0.41 x the row gate
           (profiles/r04_parity_margins.txt), which puts the bound near 10 sigma.

No assertion has exceptions.  check() evaluates all three and returns a Report with what it measured and what failed; Report.assert_ok()
raises.  Nothing here needs a GPU: tests/test_rowcheck.py runs the checker on the oracle itself and on corruptions of it."""
import numpy as np
import torch

from oracle import ref_fft_conv as O
from test_flashfftconv_gpu import REL, rel

P = 8       # representative heads
NAMES = ("y", "du", "dk", "dpregate", "dpostgate")
# mantissa bits, exponent of the smallest normal number
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}


def head_map(H, seed=0):
    """pi: head -> representative, the identity on the first min(H, P) heads and seeded pseudo-random beyond (not h % P: a systematic
    mix-up h <-> h + 1, h ^ 1, h + 8 or between chunk neighbours then lands on other data in seven cases of eight)"""
    n = min(H, P)
    pi = np.empty(H, np.int64)
    pi[:n] = np.arange(n)
    pi[n:] = np.random.RandomState(seed).randint(0, n, H - n)
    return pi


def tile(rep, pi, dim):
    """the tensor over all heads whose head h (along `dim`) is representative pi[h] of `rep`"""
    return rep.index_select(dim, torch.as_tensor(pi, device=rep.device))


def gates(dtype, gated):
    f = 1.5 if gated else 1.0
    return {nm: f * (max(REL[dtype], 1e-2) if nm == "dk" else REL[dtype]) for nm in NAMES}


def ulp(x, dtype):
    """one unit in the last place of `dtype` at the float64 values x (the subnormal step below the smallest normal number)"""
    mant, emin = _FMT[dtype]
    ax = np.abs(np.asarray(x, np.float64))
    e = np.where(ax > 0, np.frexp(ax)[1] - 1, emin)
    return np.ldexp(1.0, np.maximum(e, emin) - mant)


def rms(a):
    return np.sqrt(np.mean(a * a, axis=-1, keepdims=True))


class Want:
    """the oracle's results on the representative heads and the noise scale s_i of each (broadcasts against its result)"""

    def __init__(self, want, scale):
        self.want, self.scale = want, scale

    def nbytes(self):
        return sum(a.nbytes for a in self.want.values()) + sum(a.nbytes for a in self.scale.values())


def oracle(u, k, dout, N, pregate=None, postgate=None, residual=None):
    """float64 oracle on the given heads: u, dout, gates, residual (B, P, L), k (P, Lk) as numpy float64 arrays holding the inputs as rounded
    to the module dtype.  y = postgate * conv(u * pregate, k) + residual; the residual changes no gradient and no noise scale."""
    if pregate is None:
        y = O.ref_fft_conv(u, k, N)
        du, dk = O.ref_grads(u, k, dout, N)
        want = {"y": y, "du": du, "dk": dk}
        scale = {nm: rms(w) for nm, w in want.items()}
    else:
        y = O.ref_fft_conv_gated(u, k, pregate, postgate, N)
        du, dk, dpre, dpost, dv, c = O.ref_grads(u, k, dout, N, pregate, postgate, parts=True)
        want = {"y": y, "du": du, "dk": dk, "dpregate": dpre, "dpostgate": dpost}
        rc, rdv = rms(c), rms(dv)
        scale = {"y": rc * np.abs(postgate), "du": rdv * np.abs(pregate), "dk": rms(dk), "dpregate": rdv * np.abs(u), "dpostgate": rc * np.abs(dout)}
    if residual is not None:
        want["y"] = want["y"] + residual
    return Want(want, scale)


class Report:
    def __init__(self):
        self.row, self.elem, self.failures = {}, {}, []      # worst row error, worst |err_i| / bound_i per tensor; (kind, tensor, message)

    def kinds(self, name=None):
        return {k for k, nm, _ in self.failures if name in (None, nm)}

    def line(self):
        return "  ".join(f"{nm} {self.row[nm]:.2e}/{self.elem[nm]:.2f}" for nm in NAMES if nm in self.row)

    def assert_ok(self, what=""):
        assert not self.failures, f"{what}: " + "\n".join(f"[{k}] {nm}: {m}" for k, nm, m in self.failures)


def _where(idx, shape):
    pos = np.unravel_index(int(idx), shape)
    return "(h, t) = " + str(tuple(int(v) for v in pos)) if len(shape) == 2 else "(b, h, t) = " + str(tuple(int(v) for v in pos))


def check(got, want, pi, dtype, gated):
    """got: {name: tensor over all H heads} (any device); want: Want on the representative heads; pi: head_map.  Returns a Report."""
    rep = Report()
    tol = gates(dtype, gated)
    nrep = min(len(pi), P)
    assert list(pi[:nrep]) == list(range(nrep))
    for nm in NAMES:
        if nm not in got:
            continue
        t = got[nm].detach()
        hdim = 0 if nm == "dk" else 1
        w = want.want[nm]
        assert t.shape[hdim] == len(pi) and tuple(t.shape[:hdim]) + (nrep,) + tuple(t.shape[hdim + 1:]) == w.shape, (nm, tuple(t.shape), w.shape)
        # tied heads: bit for bit, compared where the tensor lives
        if len(pi) > nrep:
            twin = tile(t.narrow(hdim, 0, nrep), pi, hdim)
            if not torch.equal(t, twin):
                ne = (t != twin) | (t != t)
                heads = ne.transpose(0, hdim).reshape(len(pi), -1).any(dim=1)
                first = int(ne.reshape(-1).to(torch.uint8).argmax())
                rep.failures.append(("tied", nm, f"{int(heads.sum())} of {len(pi)} heads differ from their representative's in {int(ne.sum())} elements; "
                                                 f"first at {_where(first, tuple(t.shape))}, head {int(heads.to(torch.uint8).argmax())} "
                                                 f"carries representative {int(pi[int(heads.to(torch.uint8).argmax())])}"))
        g = t.narrow(hdim, 0, nrep).cpu()
        # rows of the representative heads
        g2, w2 = g.reshape(-1, g.shape[-1]), torch.from_numpy(np.ascontiguousarray(w)).reshape(-1, w.shape[-1])
        errs = np.array([rel(g2[i], w2[i]) for i in range(g2.shape[0])])
        bad = ~(errs < tol[nm])
        rep.row[nm] = float(np.nanmax(errs)) if not np.isnan(errs).all() else float("nan")
        if bad.any():
            i = int(np.argmax(np.where(np.isnan(errs), np.inf, errs)))
            rep.failures.append(("row", nm, f"rel-L2 of {int(bad.sum())} of {len(errs)} rows >= {tol[nm]:.1e}; worst {errs[i]:.3e} at row "
                                            + (f"h = {i}" if nm == "dk" else f"(b, h) = ({i // nrep}, {i % nrep})")))
        # every element of those rows
        err = np.abs(g.double().numpy() - w)
        bound = 4.0 * tol[nm] * want.scale[nm] + ulp(w, t.dtype)
        ratio = err / bound
        bad = ~(err <= bound)
        rep.elem[nm] = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float("nan")
        if bad.any():
            i = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
            rep.failures.append(("element", nm, f"{int(bad.sum())} of {err.size} elements beyond 4 x {tol[nm]:.1e} x s_i + ulp; first at "
                                                f"{_where(int(np.argmax(bad.reshape(-1))), err.shape)}, worst |err| / bound = {ratio.reshape(-1)[i]:.2f} at "
                                                f"{_where(i, err.shape)} (got {g.reshape(-1)[i].item():.6g}, want {w.reshape(-1)[i]:.6g})"))
    return rep
