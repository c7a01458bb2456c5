"""The simulator backend of flashfftconv.bigfft on BATCH-STRIDED long-side tensors: numpy views whose rows are dense and whose batch stride is free
(a channel slice of a wider array), through the ffcsim_big_outer*_strided entry points -- the same kernel body as the library's
ffc_outer_pass*_strided (csrc/ffc_big.h BigArgs::pin / pout / pgate)."""
import ctypes
import numpy as np

import simlib as S

SENTINEL = 0x7fc1      # a NaN in bf16 and in fp16: a level that reads a neighbouring slice poisons its result, one that writes there is seen


def aligned_full(shape, fill, dtype=np.uint16, align=16):
    """np.full whose first element sits on an `align`-byte boundary (the 16-byte accesses of a level need aligned base pointers)"""
    n = int(np.prod(shape))
    item = np.dtype(dtype).itemsize
    raw = np.full(n + align // item, fill, dtype)
    off = (-raw.ctypes.data % align) // item
    a = raw[off:off + n].reshape(shape)
    assert a.ctypes.data % align == 0
    return a


def pitch(a, Hin, Llong):
    """batch pitch in elements of a long-side view (B, Hin, Llong) with dense rows; 0 for none"""
    if a is None:
        return 0
    es = a.itemsize
    assert a.shape[1:] == (Hin, Llong) and a.strides[2] == es and a.strides[1] == Llong * es and a.strides[0] % es == 0, (a.shape, a.strides)
    return a.strides[0] // es


class StridedSimOps(S.SimOps):
    """SimOps whose `outer` takes numpy VIEWS on the long side and always calls the *_strided entry points (16-bit long side; the fp32 filter /
    dk rows and the wide form stay contiguous and go through SimOps.outer)"""

    def outer(self, dt, n0, fwd, inp, out, gate, bv, npair, Hin, mi, Llong, scale, lf32=None):
        if lf32 is not None or (n0 in (64, 128) and Llong > 32 * mi):
            return super().outer(dt, n0, fwd, inp, out, gate, bv, npair, Hin, mi, Llong, scale, lf32)
        if self.half:
            assert bv == 1 and npair == 1
            dt = dt | 32
        pl, pg = pitch(inp if fwd else out, Hin, Llong), pitch(gate, Hin, Llong)
        pitches = [ctypes.c_int64(v) for v in ((pl, 0, pg) if fwd else (0, pl, pg))]
        short = out if fwd else inp
        assert short.flags["C_CONTIGUOUS"]
        L_, f = S.lib(), ctypes.c_float(scale)
        if n0 in (64, 128) and self.one_launch:
            rc = L_.ffcsim_big_outer_all_strided(n0 // 32, dt, int(fwd), S.p(inp), S.p(out), S.p(gate), bv, npair, Hin, mi, Llong, f, *pitches)
            assert rc == 0, rc
        elif n0 in (64, 128):
            for c in range(n0 // 32):
                rc = L_.ffcsim_big_outer_r_strided(32, n0 // 32, c, dt, int(fwd), S.p(inp), S.p(out), S.p(gate), bv, npair, Hin, mi, Llong, f, *pitches)
                assert rc == 0, rc
        else:
            rc = L_.ffcsim_big_outer_strided(n0, dt, int(fwd), S.p(inp), S.p(out), S.p(gate), bv, npair, Hin, mi, Llong, f, *pitches)
            assert rc == 0, rc
