"""The forward's output epilogue with an addend (ConvArgs::addend, ffcsim_conv_fwd_res = the body of ffc_conv_fwd_res) on the CPU
wave simulator: y = postgate * conv(u * pregate, k) + addend, fp32 product and sum, ONE rounding to the plan dtype.

Every store site of the forward is reached (Body::rows_out on both branches, rows_out_g, rows_out_rp_t, the merged fft-2048 store), gated
and ungated, and checked for BIT equality against the output before gate and addend that the same launch stores (y_raw):
    y == round_dtype(f32(y_raw) * f32(gate) + f32(addend)),   gate = 1 when absent,
and y_raw itself must be the bits of the same call without an addend (the addend never leaks into what the backward reads)."""
import ctypes

import numpy as np
import pytest

import simlib as S

i64 = ctypes.c_int64


def _fwd_res(N, dt, u, kf, pre, post, add, want_raw=True, sb_add=0, sb_y=0, y=None):
    """-> (rc, y, z, y_raw); y_raw needs the spectrum buffer at the sizes with an outer digit (fft >= 4096)"""
    B, H, L = u.shape
    z = np.zeros(((B + 1) // 2) * H * max(N, 1024) * 2, np.uint16) if want_raw else None
    yraw = np.zeros((B, H, L), np.uint16) if want_raw else None
    if y is None:
        y = np.zeros((B, H, L), np.uint16)
    rc = S.lib().ffcsim_conv_fwd_res(N, dt, S.p(u), S.p(kf), S.p(pre), S.p(post), S.p(add), S.p(y), S.p(z), S.p(yraw), B, H, L, 0,
                                     i64(0), i64(0), i64(0), i64(sb_add), i64(sb_y))
    return rc, y, z, yraw


def _expect(dt, yraw, gate, add):
    v = S.from_bits(yraw, dt)
    if gate is not None:
        v = v * S.from_bits(gate, dt)          # exact in fp32: two 16-bit significands
    return S.to_bits(v + S.from_bits(add, dt), dt)


def _inputs(N, L, B, H, dt, seed):
    rng = np.random.default_rng(seed)
    u, g1, g2, r = (S.to_bits(rng.standard_normal((B, H, L)).astype(np.float32), dt) for _ in range(4))
    k = (rng.standard_normal((H, min(L, N))) * 0.1).astype(np.float32)
    return u, g1, g2, r, S.make_kf_internal(k, N, dt)


# (fft size, L, H): B = 3 everywhere -- the last pair is half empty
ROUTES = [
    (256, 256, 2), (1024, 1024, 2), (1024, 999, 2),      # single tile: rows_out_g, and rows_out's element-wise arm
    (2048, 1024, 2),                                       # merged store (rows fit one block, kept in registers over both passes)
    (2048, 2048, 2),                                       # per-pass store: rows_out_rp_t, addend on the last pass
    (2048, 1001, 2),                                       # ... its element-wise arm
    (4096, 4096, 2),                                       # one wave per unit
    (16384, 8192, 2), (16384, 16384, 2),                   # HALF / full rows: rows_out_g
    (16384, 8189, 2),                                      # not 16-byte: rows_out instead of rows_out_g
    (32768, 16384, 1),                                     # HALF on the 32-point outer digit
    (65536, 32768, 1), (65536, 65536, 1), (65536, 65533, 1),      # 2 passes: one row block, two row blocks, element-wise
    (131072, 131072, 1),                                   # 4 passes
]


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("dt", [S.DT_BF16, S.DT_F16])
@pytest.mark.parametrize("N,L,H", ROUTES)
def test_addend_is_one_rounding_after_the_gate(N, L, H, dt, gated):
    B = 3
    u, g1, g2, r, kf = _inputs(N, L, B, H, dt, N + L + dt)
    pre, post = (g1, g2) if gated else (None, None)
    rc, y, z, yraw = _fwd_res(N, dt, u, kf, pre, post, r)
    assert rc == 0, rc
    assert np.any(yraw), "y_raw was not written"
    assert np.array_equal(y, _expect(dt, yraw, post, r))
    rc, y0, z0, yraw0 = _fwd_res(N, dt, u, kf, pre, post, None)
    assert rc == 0, rc
    assert np.array_equal(yraw, yraw0), "y_raw must not see the addend"
    assert np.array_equal(z, z0)
    # the same call without an addend: y = gate * y_raw (the product alone: -0 stays -0)
    assert np.array_equal(y0, yraw0 if post is None else S.to_bits(S.from_bits(yraw0, dt) * S.from_bits(post, dt), dt))


@pytest.mark.parametrize("dt", [S.DT_BF16, S.DT_F16])
@pytest.mark.parametrize("N,L", [(1024, 1024), (16384, 8192), (65536, 32768)])
def test_addend_and_y_with_batch_strides(N, L, dt):
    """addend and y as channel slices of wider (B, C, L) tensors: batch strides larger than H * L, nothing written outside the slice"""
    B, H = 3, 1
    u, g1, g2, r, kf = _inputs(N, L, B, H, dt, 7 * N + dt)
    wide_r = np.full((B, H + 2, L), 0x7fc0 if dt == S.DT_BF16 else 0x7e00, np.uint16)      # NaN around the slice
    wide_r[:, 1:1 + H] = r
    wide_y = np.full((B, H + 1, L), 0xabcd, np.uint16)
    add_view = wide_r.reshape(-1)[L:]            # slice [:, 1:1+H]: starts L elements in, batch stride (H + 2) * L
    y_view = wide_y.reshape(-1)
    rc, _, _, yraw = _fwd_res(N, dt, u, kf, g1, g2, add_view, sb_add=(H + 2) * L, sb_y=(H + 1) * L, y=y_view)
    assert rc == 0, rc
    assert np.array_equal(wide_y[:, :H], _expect(dt, yraw, g2, r))
    assert np.all(wide_y[:, H:] == 0xabcd)


def test_addend_overlapping_y_is_refused():
    N, L, B, H, dt = 1024, 1024, 3, 2, S.DT_BF16
    u, g1, g2, r, kf = _inputs(N, L, B, H, dt, 1)
    y = r.copy()
    before = y.copy()
    rc, _, _, _ = _fwd_res(N, dt, u, kf, None, None, y, want_raw=False, y=y)
    assert rc == -4
    rc, _, _, _ = _fwd_res(N, dt, u, kf, None, None, y.reshape(-1)[L:], want_raw=False, sb_add=H * L, y=y)      # partial overlap
    assert rc == -4
    assert np.array_equal(y, before), "a refused call must not run"
