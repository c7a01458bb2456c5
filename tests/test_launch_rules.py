"""The host launch rules (csrc/ffc_route.h), which the HIP launchers and the CPU simulator share: which kernel variant a call runs, with
which grid and how much LDS.  Every expected value below was written by hand from the launcher text of the commit BEFORE the rules moved
into ffc_route.h (6970bff); the comment next to it names the line it was read from.  Nothing here is produced by running the code under test.
Pure host arithmetic through one simulator export, ffcsim_launch_route."""
import ctypes
import numpy as np
import pytest
import simlib as S

BF, F16 = 0, 1
ZSAVE, YRAW, SPARSE, FAST = 1 << 16, 1 << 17, 1 << 18, 1 << 19      # the export's own flag bits, next to the tuning flags 32 / 64 / 128
PERSIST = 256                  # ffc_persist(): CU count rounded down to 8 (ffc_dev.h:311)
UNCAPPED = 1 << 30             # ffc_persist() under FFC_PERSIST=0 (ffc_dev.h:312)
IPASS = 2 * 6144 + 2 * 8192    # Body::IPASS_BYTES (ffc_body.h:1476)
# Geo<..>::LDS_BYTES by hand from ffc_layout.h:50-61, for N3 == N2.  Single tile: 8 exchange buffers of 4096 bytes, one operand table
# (6144), forward and inverse inner twiddle tables (8192 each).  Outer digit: 131072 of exchange buffers, two operand tables, one twiddle
# table; + 3072 for the frequency-sparse table of the 32 x 32 inner digits
LDS_1024 = 8 * 4096 + 6144 + 8192 + 8192          # Geo<1,32,32> and Geo<1,16,16>
LDS_4096 = 131072 + 6144 + 6144 + 8192            # Geo<16,16,16>, Geo<32,16,16>
LDS_32768 = LDS_4096 + 3072                       # Geo<16,32,32>, Geo<32,32,32>


def route(N, L, dt=BF, B=16, H=768, nchunk=1, persist=PERSIST, flags=0):
    out = np.full(27, -99, np.int32)
    assert S.lib().ffcsim_launch_route(N, dt, B, H, L, nchunk, persist, flags, out.ctypes.data_as(ctypes.c_void_p)) == 0
    keys_f = ("multi_pass", "half", "sz", "sp", "grid", "lds_max", "lds", "err")
    keys_b = ("multi_pass", "half", "fastk", "small", "grid", "lds_max", "lds", "err")
    return {"fwd": dict(zip(keys_f, out[0:8].tolist())), "bwd": dict(zip(keys_b, out[8:16].tolist())), "dkf": dict(zip(keys_b, out[16:24].tolist())),
            "kfft": int(out[24]), "dk": int(out[25]), "dk_rows": int(out[26])}


# HALF iff L <= bound.  Single pass: (GEO::N1 / 2) * GEO::Mi >= L (ffc_k_conv.hip:158, ffc_bwd_launch.h:103, ffc_k_dkf.hip:75);
# multi-pass sizes, passes of the 32768 kernel: 16 * GEO::Mi >= L with Mi = 1024 (ffc_k_conv.hip:88, ffc_bwd_launch.h:77, ffc_k_dkf.hip:50)
HALF_BOUND = {4096: 2048,      # Geo<16,16,16>: 8 * 256
              8192: 4096,      # Geo<32,16,16>: 16 * 256
              16384: 8192,     # Geo<16,32,32>: 8 * 1024
              32768: 16384,    # Geo<32,32,32>: 16 * 1024
              65536: 16384, 131072: 16384}


@pytest.mark.parametrize("N", sorted(HALF_BOUND))
def test_half_boundary(N):
    for L, half in ((HALF_BOUND[N], 1), (HALF_BOUND[N] + 1, 0)):
        r = route(N, L)
        multi = int(N > 32768)             # `if (a.R > 1)` + `GEO::N == 32768`: ffc_k_conv.hip:73-74, ffc_bwd_launch.h:74-75, ffc_k_dkf.hip:47-48
        for k in ("fwd", "bwd", "dkf"):
            assert (r[k]["half"], r[k]["multi_pass"], r[k]["err"]) == (half, multi, 0), (N, L, k, r[k])
        assert r["bwd"]["small"] == 0 and r["fwd"]["grid"] == (PERSIST if N == 4096 else 768)      # ffc_k_conv.hip:117 (NW == 1 only at fft 4096)


@pytest.mark.parametrize("N,L", [(256, 128), (512, 200), (1024, 512), (2048, 1024), (2048, 8)])
def test_no_half_at_the_single_tile_sizes(N, L):
    r = route(N, L)            # `GEO::OUTER && ...` ffc_k_conv.hip:158; the single-tile branches name no HALF: ffc_bwd_launch.h:94-101, ffc_k_dkf.hip:67-73
    assert r["fwd"]["half"] == r["bwd"]["half"] == r["dkf"]["half"] == 0
    assert r["bwd"]["small"] == r["dkf"]["small"] == 1
    assert r["fwd"]["multi_pass"] == int(N == 2048)      # ffc_k_conv.hip:99: conv_rp_kernel of Geo<1,32,32>
    assert r["bwd"]["multi_pass"] == r["dkf"]["multi_pass"] == 0      # ffc_bwd_launch.h:86 `else if constexpr (GEO::OUTER)`: fft 2048 falls through to bwd_kernel_small


def test_fft2048_lds_pair_and_cap():
    # (fft 2048 always has R = 2, so lds_max and lds of the forward have the same value here and a swap of the two would pass; the fft 1024
    # backward line below, lds_max > lds, is the one that tells them apart)
    r = route(2048, 1024)
    f = r["fwd"]
    assert f["lds_max"] == LDS_1024 + 2 * IPASS          # ffc_k_conv.hip:100 `GEO::LDS_BYTES + 2 * BD::IPASS_BYTES`
    assert f["lds"] == LDS_1024 + 2 * IPASS              # ffc_k_conv.hip:105 `GEO::LDS_BYTES + a.R * BD::IPASS_BYTES`, R = 2
    assert f["grid"] == 2 * PERSIST                      # ffc_k_conv.hip:101, :105 `grid > cap ? cap : grid`, cap = 2 * persist < 768
    assert route(2048, 1024, H=40)["fwd"]["grid"] == 40
    assert route(2048, 1024, persist=UNCAPPED)["fwd"]["grid"] == 768      # ffc_k_conv.hip:101 `a.persist < (1 << 29)`
    b, d = r["bwd"], r["dkf"]
    assert (b["lds_max"], b["lds"]) == (LDS_1024 + 2 * IPASS, LDS_1024 + 2 * IPASS)      # ffc_bwd_launch.h:96-97
    assert (d["lds_max"], d["lds"]) == (LDS_1024 + 2 * IPASS, LDS_1024 + 2 * IPASS)      # ffc_k_dkf.hip:69-70
    r1 = route(1024, 1024)
    assert (r1["bwd"]["lds_max"], r1["bwd"]["lds"]) == (LDS_1024 + 2 * IPASS, LDS_1024)  # ffc_bwd_launch.h:96 `d.c.R > 1 ? ... : 0`
    assert (r1["fwd"]["lds_max"], r1["fwd"]["lds"]) == (LDS_1024, LDS_1024)               # ffc_k_conv.hip:163-165
    assert route(256, 256)["fwd"]["lds"] == LDS_1024
    for N in (4096, 8192):
        assert route(N, N)["fwd"]["lds"] == route(N, N)["bwd"]["lds"] == LDS_4096
    for N in (16384, 32768, 65536):
        assert route(N, N)["fwd"]["lds"] == route(N, N)["dkf"]["lds_max"] == LDS_32768


def test_grid_caps():
    assert route(4096, 4096)["fwd"]["grid"] == PERSIST                 # ffc_k_conv.hip:117 `grid > a.persist`
    assert route(4096, 4096)["bwd"]["grid"] == PERSIST                 # ffc_bwd_launch.h:90
    assert route(4096, 4096)["dkf"]["grid"] == PERSIST                 # ffc_k_dkf.hip:65
    assert route(4096, 4096, H=100)["fwd"]["grid"] == 104              # (H + 7) & ~7, ffc_k_conv.hip:71-72
    assert route(4096, 4096, persist=UNCAPPED)["fwd"]["grid"] == 768
    for N in (256, 512, 1024):
        r = route(N, N)
        assert r["fwd"]["grid"] == 2 * PERSIST                         # ffc_k_conv.hip:118 `grid > 2 * a.persist`
        assert r["bwd"]["grid"] == 2 * PERSIST                         # ffc_bwd_launch.h:100-101
        assert r["dkf"]["grid"] == 768                                 # ffc_k_dkf.hip:66, :73: dkf_kernel_small takes the whole grid
        assert route(N, N, persist=UNCAPPED)["fwd"]["grid"] == route(N, N, persist=UNCAPPED)["bwd"]["grid"] == 768
    for N in (8192, 16384, 32768, 65536, 131072):                      # one workgroup per (head, chunk): no cap applies
        r = route(N, N, H=770, nchunk=2)
        assert r["fwd"]["grid"] == r["bwd"]["grid"] == r["dkf"]["grid"] == 776 * 2


def test_spectrum_saving_variant():
    for N in (256, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072):
        single_tile = N <= 2048
        assert route(N, 100, flags=ZSAVE)["fwd"]["sz"] == 1            # ffc_k_conv.hip:75, :102, :136
        assert route(N, 100, flags=ZSAVE | YRAW)["fwd"]["sz"] == 1
        # y_raw alone: `a.zsave || (!GEO::OUTER && a.yraw)` ffc_k_conv.hip:136, `a.zsave || a.yraw` of Geo<1,32,32> :102, `a.zsave` of the 32768 passes :75
        assert route(N, 100, flags=YRAW)["fwd"]["sz"] == int(single_tile), N
        assert route(N, 100)["fwd"]["sz"] == 0
    assert route(4096, 2048, flags=ZSAVE)["fwd"]["half"] == 1          # ffc_k_conv.hip:138
    assert route(1024, 512, flags=ZSAVE)["fwd"]["half"] == 0           # ffc_k_conv.hip:150 `conv_kernel<GEO, DT, false, true>`


def test_sparse_route():
    for N in (16384, 32768):                                           # `if constexpr (GEO::HAS_SP)` ffc_k_conv.hip:120, HAS_SP = OUTER && N2 == 32 && N3 == 32
        for L, half in ((HALF_BOUND[N], 1), (HALF_BOUND[N] + 1, 0)):   # ffc_k_conv.hip:121
            f = route(N, L, flags=SPARSE)["fwd"]
            assert (f["sp"], f["half"], f["sz"], f["err"], f["grid"]) == (1, half, 0, 0, 768)
    for N in (256, 1024, 4096, 8192):
        assert route(N, N, flags=SPARSE)["fwd"]["err"] == 1            # ffc_k_conv.hip:133 "frequency-sparse kernel: fft 16384 / 32768 only"
    assert route(32768, 100)["fwd"]["sp"] == 0


def test_kfft_inside_the_forward_launch():
    # ffc_k_conv.hip:222-223 / :343: nchunk == 1 && 8192 <= N <= 32768 && R == 1 && !sparse && !(flags & 64)
    assert route(4096, 4096)["kfft"] == 0
    for N in (8192, 16384, 32768):
        assert route(N, N)["kfft"] == 1
        assert route(N, N, dt=F16)["kfft"] == 1
        assert route(N, N, nchunk=2)["kfft"] == 0
        assert route(N, N, flags=64)["kfft"] == 0
    assert route(32768, 100, flags=SPARSE)["kfft"] == 0
    assert route(65536, 65536)["kfft"] == 0
    assert route(2048, 2048)["kfft"] == 0


def test_dk_inside_the_backward_launch():
    # the tail, ffc_k_bwd.hip:88-89: nchunk == 1 && N >= (flags & 128 ? 8192 : 16384) && N <= 32768 && R == 1 && !(flags & 32)
    for N in (16384, 32768):
        assert (route(N, N)["dk"], route(N, N)["dk_rows"]) == (1, 1)   # complex rows: the same rule, ffc_k_bwd.hip:104-105
        assert route(N, N, dt=F16)["dk"] == 1
        assert (route(N, N, nchunk=2)["dk"], route(N, N, nchunk=2)["dk_rows"]) == (0, 0)
        assert (route(N, N, flags=32)["dk"], route(N, N, flags=32)["dk_rows"]) == (0, 0)
    assert (route(8192, 8192)["dk"], route(8192, 8192)["dk_rows"]) == (0, 0)
    assert (route(8192, 8192, flags=128)["dk"], route(8192, 8192, flags=128)["dk_rows"]) == (1, 1)
    assert route(8192, 8192, flags=128 | 32)["dk"] == 0
    assert route(4096, 4096, flags=128)["dk"] == 0
    assert route(1024, 1024, flags=128)["dk"] == 0
    # the multi-pass tail, ffc_k_bwd.hip:96-97: nchunk == 1 && R > 1 && N1 > 1 && dtype == bf16 && !(flags & 32); real dk only (:104 asks R == 1)
    for N in (65536, 131072):
        assert (route(N, N)["dk"], route(N, N)["dk_rows"]) == (2, 0)
        assert route(N, N, dt=F16)["dk"] == 0
        assert route(N, N, nchunk=2)["dk"] == 0
        assert route(N, N, flags=32)["dk"] == 0
    assert route(2048, 2048)["dk"] == 0                                # R > 1 but no outer digit (N1 == 1)


def test_fast_only_backward_of_the_multi_pass_sizes():
    # ffc_bwd_launch.h:79 `d.c.fast && (FFC_RP_FASTK != 0)` inside the `GEO::N == 32768` branch of `d.c.R > 1`; the dk_f kernel has no such form
    for N in (65536, 131072):
        assert route(N, N, flags=FAST)["bwd"]["fastk"] == 1
        assert route(N, N)["bwd"]["fastk"] == 0
        assert route(N, N, flags=FAST)["dkf"]["fastk"] == 0
    assert route(32768, 32768, flags=FAST)["bwd"]["fastk"] == 0
    assert route(2048, 2048, flags=FAST)["bwd"]["fastk"] == 0
