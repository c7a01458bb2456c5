"""Frequency-sparse fused backward (Modes::bwd_sp) and the live-row dk inverse (Modes::dkifft_sp) on the CPU wave simulator, against the float64
definition with the masked k_f.  Bounds: those of the sparse forward and of the dk path in tests/test_sim_kernels.py (1.5 TOL[dt]; dk 1.5 TOL[bf16],
its inverse always runs in bf16 arithmetic).  ws starts as NaN: dk must come out finite and the dead spectrum rows must still be NaN."""
import numpy as np
import pytest

import simlib as S
from test_sim_kernels import TOL, q, rel

N, L, B, H = 16384, 8192, 3, 2      # two units per workgroup, the second with a half-empty pair; L <= N / 2


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,keep", [(1, N // 32), (4, 3 * N // 32 + 5)], ids=["rows1", "rows4"])
def test_sparse_backward_on_the_simulator(rows, keep, dt, gated):
    rng = np.random.default_rng(rows + 10 * dt + 100 * gated)
    u, d, g1, g2 = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(4))
    k = (rng.standard_normal((H, L)) * 0.1).astype(np.float32)
    f = np.arange(N)
    live = (f < keep) | (f > N - keep)
    kfn = np.fft.fft(k.astype(np.float64), n=N) * live
    kf = S.make_kf_from_spectrum(kfn, N, dt)
    nt, _, _, freq = S.plan_info(N, dt)
    mask = live[freq].astype(np.float32)
    pre, post = (S.to_bits(g1, dt), S.to_bits(g2, dt)) if gated else (None, None)
    ub, db = S.to_bits(u, dt), S.to_bits(d, dt)
    ws = np.full(H * nt * 2048, np.nan, np.float32)
    du, dpre, dpost = (np.zeros_like(ub) if (gated or i == 0) else None for i in range(3))
    nslab = S.lib().ffcsim_conv_bwd_sparse(N, dt, S.p(db), S.p(ub), S.p(kf), S.p(pre), S.p(post), S.p(du), S.p(dpre), S.p(dpost), S.p(ws),
                                           B, H, L, 1, rows)
    assert nslab == 1, nslab
    slab = ws.reshape(H, nt, 8, 32 * 4 * 2)      # [head][tile][spectrum row rho][...]
    assert np.isfinite(slab[:, :, [0, 7]]).all() and np.isnan(slab[:, :, 1:7]).all(), "live rows written, dead rows untouched"
    dk = np.full((H, L), np.nan, np.float32)
    assert S.lib().ffcsim_kernel_ifft_grad_sp(N, dt, S.p(ws), S.p(mask), rows, nslab, H, L, S.p(dk)) == 0
    assert np.isnan(slab[:, :, 1:7]).all() and np.isfinite(dk).all()

    v = q(q(u, dt) * q(g1, dt), dt) if gated else q(u, dt)
    dc = q(q(d, dt) * q(g2, dt), dt) if gated else q(d, dt)
    vf, df = np.fft.fft(v, n=N), np.fft.fft(dc, n=N)
    dv = np.fft.ifft(df * np.conj(kfn)[None], n=N).real[..., :L]
    want = {"du": dv * q(g1, dt) if gated else dv, "dk": np.fft.ifft((df * np.conj(vf)).sum(0) * live).real[:, :L]}
    got = {"du": S.from_bits(du, dt), "dk": dk}
    if gated:
        want["dpre"] = dv * q(u, dt)
        want["dpost"] = np.fft.ifft(vf * kfn[None], n=N).real[..., :L] * q(d, dt)
        got["dpre"], got["dpost"] = S.from_bits(dpre, dt), S.from_bits(dpost, dt)
    errs = {nm: rel(got[nm], want[nm]) for nm in want}
    print("sparse_bwd_sim", rows, keep, dt, gated, {nm: f"{e:.2e}" for nm, e in errs.items()})
    for nm, e in errs.items():
        assert e < 1.5 * (TOL[0] if nm == "dk" else TOL[dt]), (nm, e)
