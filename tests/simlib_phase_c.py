"""Simulator hooks for the half-height phase C of fft 32768 (csrc/ffc_body.h Body::outer_inv_half): the 16x16x32 MFMA of the backend, the
stage alone, the tuning flags of the next calls, the count of direct-store kernel runs and the launch rule that picks the sink."""
import contextlib
import ctypes
import numpy as np

import simlib as S


def mfma16(dt, A, Bm, C):
    """D = A (16 x 32) B (32 x 16) + C through SimB::mfma16, operands packed by the ISA's lane layout: lane l holds A[l % 16][8 (l / 16) + e],
    B[8 (l / 16) + e][l % 16] in element e of its 4 operand dwords and D[4 (l / 16) + r][l % 16] in accumulator register r"""
    ab, bb = S.to_bits(A, dt), S.to_bits(Bm, dt)
    a, b, d = np.zeros((64, 4), np.uint32), np.zeros((64, 4), np.uint32), np.zeros((64, 4), np.float32)
    for l in range(64):
        for e in range(8):
            a[l, e // 2] |= np.uint32(int(ab[l % 16, 8 * (l // 16) + e]) << (16 * (e % 2)))
            b[l, e // 2] |= np.uint32(int(bb[8 * (l // 16) + e, l % 16]) << (16 * (e % 2)))
        for r in range(4):
            d[l, r] = C[4 * (l // 16) + r, l % 16]
    assert S.lib().ffcsim_mfma16(dt, S.p(a), S.p(b), S.p(d)) == 0
    D = np.zeros((16, 16), np.float32)
    for l in range(64):
        for r in range(4):
            D[4 * (l // 16) + r, l % 16] = d[l, r]
    return D


def stage(dt, e):
    """e (2 planes, 32 rows k1, 1024 columns) float -> rows n1 < 16 of the stage's output (2, 16, 1024) float"""
    eb = np.ascontiguousarray(S.to_bits(e, dt))
    out = np.zeros((2, 16, 1024), np.uint16)
    assert S.lib().ffcsim_outer_inv_half(dt, S.p(eb), S.p(out)) == 0
    return S.from_bits(out, dt)


@contextlib.contextmanager
def flags(f):
    """ConvArgs::flags (the library's FFC_FLAGS) of the simulator's forward / backward calls inside the block"""
    S.lib().ffcsim_set_flags(f)
    try:
        yield
    finally:
        S.lib().ffcsim_set_flags(0)


_gs_total = 0


def gs_count():
    """runs of a direct-store kernel variant so far (monotonic)"""
    global _gs_total
    S.lib().ffcsim_gs_count.restype = ctypes.c_long
    _gs_total += S.lib().ffcsim_gs_count()
    return _gs_total


def launch_sink(N, L, fl, B=4, H=2, dt=0):
    out = np.zeros(3, np.int32)
    assert S.lib().ffcsim_launch_sink(N, dt, B, H, L, fl, S.p(out)) == 0
    return tuple(int(v) for v in out)
