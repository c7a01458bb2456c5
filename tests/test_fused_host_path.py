"""flashfftconv/fused.py without a GPU: the library is a recorder, the operands are CPU tensors (their data_ptr() is enough).  Which
C-ABI entry point a forward / backward takes and with which arguments, pointer values included, against the table written out below;
the optional-tensor packing, the k_f step per cache slot, the keep step and its out-of-memory fallback, the slab view and the dk step."""
import ctypes
import itertools
import types
import pytest
import torch

from flashfftconv import _lib, conv as C, fused as F

B, H, L, D, HFULL, G0 = 3, 2, 16, 2, 5, 3      # rows per call (B, H, L); slices of a (B, 3D, L) tensor with D = H; heads [3, 5) of HFULL
STREAM, PLAN = 77, 0x1000
ES = 2                                          # bytes per bf16 element


class _Recorder:
    """stands in for the loaded library: every entry point records (name, plain argument values) and succeeds"""

    def __init__(self, answers=None):
        self.calls, self.answers = [], answers or {}

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, tuple(x.value if isinstance(x, ctypes.c_void_p) else x for x in a)))
            return self.answers.get(name, 0)
        return call


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: STREAM)
    return rec


def _plan(seqlen=4096, kf_elems=8):
    return types.SimpleNamespace(handle=ctypes.c_void_p(PLAN), seqlen=seqlen, kf_elems=kf_elems, dtype=torch.bfloat16)


def _operands(layout, names, absent=()):
    """-> {name: (rows_of operand, expected pointer, expected stride)} for the three ways the callers address their rows; the names in
    `absent` have no tensor"""
    out = {}
    if layout == "slices":
        wide = {}
    for i, nm in enumerate(names):
        if layout == "contiguous":                   # FlashFFTConv: rows_of(t)
            t = torch.zeros(B, H, L, dtype=torch.bfloat16)
            out[nm] = (F.NULL, None, 0) if nm in absent else (F.rows_of(t), t.data_ptr(), 0)
        elif layout == "slices":                     # the Hyena op: slice j of a (B, 3D, L) tensor (one per role: inputs, gradients), others whole
            j = {"pre": 0, "post": 1, "u": 2, "dpre": 0, "dpost": 1, "du": 2}.get(nm)
            if nm in absent:
                out[nm] = (F.NULL, None, 0)
            elif j is None:
                t = torch.zeros(B, D, L, dtype=torch.bfloat16)
                out[nm] = (F.rows_of(t), t.data_ptr(), 0)
            else:
                t = wide.setdefault(nm[0] == "d", torch.zeros(B, 3 * D, L, dtype=torch.bfloat16))
                out[nm] = (F.rows_of(t, j * D * L, 3 * D * L), t.data_ptr() + j * D * L * ES, 3 * D * L)
        else:                                        # the B-shard: heads [G0, G0 + H) of (B, HFULL, L) tensors; a null operand keeps the stride
            t = torch.zeros(B, HFULL, L, dtype=torch.bfloat16)
            out[nm] = ((F.rows_of(None, G0 * L, HFULL * L), None, HFULL * L) if nm in absent
                       else (F.rows_of(t, G0 * L, HFULL * L), t.data_ptr() + G0 * L * ES, HFULL * L))
        out[nm] = out[nm] + (t if nm not in absent else None,)      # (keeps the tensor alive)
    return out


LAYOUTS = ("contiguous", "slices", "head range")
KEPT = ("nothing", "z", "z+yraw", "yraw")


def _kept(which):
    z = torch.zeros(64, dtype=torch.uint8) if which in ("z", "z+yraw") else None
    yraw = torch.zeros(B, H, L, dtype=torch.bfloat16) if which in ("z+yraw", "yraw") else None
    return z, yraw


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("layout,gated,kept,addend,rows", list(itertools.product(LAYOUTS, (False, True), KEPT, (False, True), (0, 2))))
def test_forward_entry_point_and_arguments(lib, layout, gated, kept, addend, rows):
    absent = (() if gated else ("pre", "post")) + (() if addend else ("add",))
    o = _operands(layout, ("u", "pre", "post", "y", "add"), absent)
    kf, (z, yraw) = torch.zeros(H, 8, 2, dtype=torch.bfloat16), _kept(kept)
    F.forward(_plan(), B, H, L, o["u"][0], kf, o["pre"][0], o["post"][0], o["y"][0], o["add"][0], z, yraw, rows)
    p, s = {n: v[1] for n, v in o.items()}, {n: v[2] for n, v in o.items()}
    head = (PLAN, p["u"], _p(kf), p["pre"], p["post"])
    strided = any(s[n] for n in ("u", "pre", "post", "y"))
    # the table: first row whose condition holds
    table = [
        (addend, "ffc_conv_fwd_res", head + (p["add"], p["y"], _p(z), _p(yraw), B, H, L, 0, s["u"], s["pre"], s["post"], s["add"], s["y"], STREAM)),
        (z is not None or yraw is not None, "ffc_conv_fwd_z", head + (p["y"], _p(z), _p(yraw), B, H, L, s["u"], s["pre"], s["post"], s["y"], STREAM)),
        (strided, "ffc_conv_fwd_strided", head + (p["y"], B, H, L, 0, s["u"], s["pre"], s["post"], s["y"], STREAM)),
        (rows > 0, "ffc_conv_fwd_sparse", head + (p["y"], B, H, L, 0, rows, STREAM)),
        (True, "ffc_conv_fwd", head + (p["y"], B, H, L, 0, STREAM)),
    ]
    want = next((name, a) for cond, name, a in table if cond)
    assert lib.calls == [want]
    assert strided == (layout != "contiguous")


@pytest.mark.parametrize("layout,gated,kept,rows", list(itertools.product(LAYOUTS, (False, True), KEPT, (0, 2))))
def test_backward_entry_point_and_arguments(lib, layout, gated, kept, rows):
    names = ("dout", "u", "pre", "post", "du", "dpre", "dpost")
    o = _operands(layout, names, () if gated else ("pre", "post", "dpre", "dpost"))
    kf, ws, (z, yraw) = torch.zeros(H, 8, 2, dtype=torch.bfloat16), torch.zeros(256, dtype=torch.uint8), _kept(kept)
    F.backward(_plan(), B, H, L, *(o[n][0] for n in ("dout", "u")), kf, *(o[n][0] for n in names[2:]), ws, z, yraw, rows)
    p, s = {n: v[1] for n, v in o.items()}, tuple(o[n][2] for n in names)
    head = (PLAN, p["dout"], p["u"], _p(kf), p["pre"], p["post"], p["du"], p["dpre"])
    table = [
        (rows > 0, "ffc_conv_bwd_sparse", head + (p["dpost"], _p(ws), None, B, H, L, rows, STREAM)),
        (gated and (z is not None or yraw is not None), "ffc_conv_bwd_zy", head + (p["dpost"], _p(ws), _p(z), _p(yraw), B, H, L) + s + (STREAM,)),
        (z is not None, "ffc_conv_bwd_z", head + (None, _p(ws), _p(z), B, H, L) + s + (STREAM,)),
        (any(s), "ffc_conv_bwd_gated_strided", head + (p["dpost"], _p(ws), B, H, L) + s + (STREAM,)),
        (True, "ffc_conv_bwd_gated", head + (p["dpost"], _p(ws), B, H, L, STREAM)),
    ]
    want = next((name, a) for cond, name, a in table if cond)
    assert lib.calls == [want]


def test_one_call_entries(lib):
    plan, mod = _plan(), types.SimpleNamespace(cache_kf=True, _kf_cache=None)
    u, k = torch.zeros(B, H, L, dtype=torch.bfloat16), torch.zeros(H, 7)
    y, kf = F.forward_k(mod, plan, k, u, None, None, None, None)
    assert lib.calls == [("ffc_conv_fwd_k", (PLAN, k.data_ptr(), 7, kf.data_ptr(), u.data_ptr(), None, None, y.data_ptr(), None, None, B, H, L, STREAM))]
    assert kf.shape == (H, plan.kf_elems, 2) and kf.dtype == plan.dtype and y.shape == u.shape
    assert mod._kf_cache[0] == C._kf_key(k) and mod._kf_cache[1] is kf
    del lib.calls[:]
    ws, z = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    dk = F.backward_k(plan, u, u, kf, None, None, y, None, None, ws, z, None, 7)
    assert lib.calls == [("ffc_conv_bwd_k", (PLAN, u.data_ptr(), u.data_ptr(), kf.data_ptr(), None, None, y.data_ptr(), None, None, ws.data_ptr(),
                                             z.data_ptr(), None, dk.data_ptr(), 7, B, H, L, STREAM))]
    assert dk.shape == (H, 7) and dk.dtype == torch.float32


@pytest.mark.parametrize("n", range(4))
def test_pack_kept_round_trips_every_pattern_of_holes(n):
    assert F.pack_kept(None) == (None, ()) and F.unpack_kept(None, ()) is None
    for holes in itertools.product((False, True), repeat=n):
        tensors = tuple(None if h else torch.zeros(1) for h in holes)
        layout, there = F.pack_kept(tensors)
        assert len(there) == holes.count(False) and all(t is not None for t in there)
        back = F.unpack_kept(layout, there + (torch.ones(1),))      # (a sequence that goes on behind them)
        assert len(back) == n and all(a is b for a, b in zip(back, tensors))
    # several groups behind one another share an iterator
    groups = [(torch.zeros(1), None), None, (None, torch.zeros(1), torch.zeros(1))]
    packs = [F.pack_kept(g) for g in groups]
    it = iter([t for _, there in packs for t in there])
    back = [F.unpack_kept(layout, it) for layout, _ in packs]
    assert back[1] is None and all(a is b for g, r in ((groups[0], back[0]), (groups[2], back[2])) for a, b in zip(g, r))


def _kf_module(**kw):
    d = dict(cache_kf=True, seqlen=4096, _folded=False, _kf_keep=None, _kf_cache=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.fixture
def transforms(monkeypatch):
    """stub k -> k_f launches: count them, return a fresh tensor that names its inputs"""
    made = []

    def plain(plan, k):
        made.append(("plain", k))
        return torch.ones(k.shape[0], plan.kf_elems, 2)

    def bi(plan, k, k_rev):
        made.append(("bi", k, k_rev))
        return torch.ones(k.shape[0], plan.kf_elems, 2)
    monkeypatch.setattr(C, "_kernel_fft", plain)
    monkeypatch.setattr(C, "_kernel_fft_bi", bi)
    return made


def test_kf_step_hits_misses_and_stores_per_slot(transforms):
    plan, mod = _plan(), _kf_module()
    k, k2, kr = torch.zeros(H, 5), torch.zeros(H, 5), torch.zeros(H, 3)
    a = F.kf_for(mod, plan, k)
    assert len(transforms) == 1 and mod._kf_cache == (C._kf_key2(k, None), a)                 # miss, stored
    assert F.kf_for(mod, plan, k) is a and F.cached_kf(mod, k) is a and len(transforms) == 1  # hit
    r = F.kf_for(mod, plan, k2, None, "_kf_cache_res")                                        # a second slot does not evict the first
    assert len(transforms) == 2 and mod._kf_cache_res[1] is r and F.kf_for(mod, plan, k) is a and len(transforms) == 2
    assert F.kf_for(mod, plan, k2, None, "_kf_cache_res") is r and len(transforms) == 2
    assert F.cached_kf(mod, k2) is None                                                       # another filter: a miss in the first slot
    k.add_(1)                                                                                 # same storage, next version: a miss
    b = F.kf_for(mod, plan, k)
    assert b is not a and len(transforms) == 3 and mod._kf_cache[1] is b
    p = F.kf_for(mod, plan, k, kr)                                                            # the pair (k, k_rev): its own key, the two-tensor launch
    assert transforms[-1][0] == "bi" and transforms[-1][2] is kr and mod._kf_cache == (C._kf_key2(k, kr), p)
    assert F.kf_for(mod, plan, k, kr) is p and len(transforms) == 4
    for kk, rr in ((k.clone().requires_grad_(), None), (k, kr.clone().requires_grad_())):     # a filter that requires grad: never cached
        before = mod._kf_cache
        F.kf_for(mod, plan, kk, rr); F.kf_for(mod, plan, kk, rr)
        assert mod._kf_cache is before and F.cached_kf(mod, kk, rr) is None
    assert len(transforms) == 8
    off = _kf_module(cache_kf=False)
    F.kf_for(off, plan, k2); F.kf_for(off, plan, k2)
    assert len(transforms) == 10 and off._kf_cache is None


def test_kf_step_folded_row_and_sparse_mask(transforms):
    plan = _plan()
    k = torch.arange(6.).view(2, 3)
    F.kf_for(_kf_module(cache_kf=False, seqlen=2048, _folded=True), plan, k)
    row = transforms[-1][1]
    assert row.shape == (2, 4096) and torch.equal(row[:, :3], k) and torch.equal(row[:, 2048:2051], k) and row[:, 3:2048].abs().sum() == 0
    mask = torch.tensor([1., 0.] * (plan.kf_elems // 2))
    mod = _kf_module(_kf_keep=5, _kf_mask=lambda plan, dtype: mask)
    kf = F.kf_for(mod, plan, k)
    assert torch.equal(kf, mask[None, :, None].expand(2, -1, 2)) and mod._kf_cache[1] is kf      # (the masked k_f is what the slot holds)


def test_keep_step_and_its_out_of_memory_fallback(monkeypatch):
    answers = {"ffc_spectrum_bytes": 4096}
    monkeypatch.setattr(_lib, "lib", lambda: _Recorder(answers))
    plan, like = _plan(), torch.zeros(B, H, L, dtype=torch.bfloat16)
    mod = types.SimpleNamespace(save_spectrum=True)
    asked = []
    real = C._spectrum_buffer
    monkeypatch.setattr(C, "_spectrum_buffer", lambda *a: (asked.append(a), real(*a))[1])
    assert F.keep(mod, plan, B, H, like, True, False) == (None, None) and not asked               # nobody wants gradients
    assert F.keep(types.SimpleNamespace(save_spectrum=False), plan, B, H, like, True, True) == (None, None) and not asked
    z, yraw = F.keep(mod, plan, B, H, like, True, True)
    assert asked == [(plan, B, H, like.device, True, True)]
    assert z.numel() == 4096 and z.dtype == torch.uint8 and yraw.shape == (B, H, L) and yraw.dtype == like.dtype
    z, yraw = F.keep(mod, plan, B, H, like, False, True)                                           # ungated: spectra alone
    assert z is not None and yraw is None
    del asked[:]
    z, yraw = F.keep(mod, plan, B, H, like, True, True, y_only=True)                               # the module's y-only choice
    assert z is None and yraw.shape == (B, H, L) and not asked
    assert F.keep(mod, _plan(1024), B, H, like, False, True) == (None, None)                       # single-tile sizes without gates keep nothing
    # out of memory: the spectrum allocation (counted inside conv._spectrum_buffer, as at every site before), and the y_raw allocation
    # behind it (the spectra are dropped too; no site has ever counted that one)
    empty, fail_at, n = torch.empty, [], [0]

    def failing(*a, **kw):
        n[0] += 1
        if n[0] in fail_at:
            raise torch.cuda.OutOfMemoryError("out of memory")
        return empty(*a, **kw)
    monkeypatch.setattr(torch, "empty", failing)
    before = dict(C.SPECTRUM_FALLBACKS)
    n[0], fail_at[:] = 0, [1]
    assert F.keep(mod, plan, B, H, like, True, True) == (None, None)
    assert C.SPECTRUM_FALLBACKS == {"budget": before["budget"], "oom": before["oom"] + 1} and n[0] == 1
    n[0], fail_at[:] = 0, [2]
    assert F.keep(mod, plan, B, H, like, True, True) == (None, None)
    assert C.SPECTRUM_FALLBACKS == {"budget": before["budget"], "oom": before["oom"] + 1} and n[0] == 2
    monkeypatch.setitem(C.SPECTRUM_FALLBACKS, "oom", before["oom"])


def test_slab_view_and_dk_step(monkeypatch):
    rec = _Recorder({"ffc_dkf_slab_count": 2})
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: STREAM)
    plan = _plan(kf_elems=4)
    ws = torch.zeros(2 * H * 4 * 8 + 40, dtype=torch.uint8)
    slabs = F.dkf_slabs(plan, ws, B, H)
    assert rec.calls == [("ffc_dkf_slab_count", (PLAN, B, H))]
    assert slabs.shape == (2, H, 4, 2) and slabs.dtype == torch.float32 and slabs.data_ptr() == ws.data_ptr()
    slabs[0].fill_(1.0); slabs[1].fill_(2.0)
    assert torch.equal(F.dkf_sum(plan, ws, B, H), torch.full((H, 4, 2), 3.0))
    rec.answers["ffc_dkf_slab_count"] = 1
    assert F.dkf_sum(plan, ws, B, H).data_ptr() == ws.data_ptr()            # one slab: a view, no sum kernel
    # dk step: plain, folded (the plan's length in, the fold-back out), and the pair of a bidirectional filter
    del rec.calls[:]
    mod = types.SimpleNamespace(_folded=False, seqlen=4096)
    dk, dk_rev = F.dk_from(mod, plan, ws, B, H, 7, torch.float64)
    assert rec.calls == [("ffc_kernel_ifft_grad", (PLAN, ws.data_ptr(), B, H, 7, rec.calls[0][1][5], STREAM))]
    assert dk.shape == (H, 7) and dk.dtype == torch.float64 and dk_rev is None
    del rec.calls[:]
    dk, _ = F.dk_from(types.SimpleNamespace(_folded=True, seqlen=2048), plan, ws, B, H, 7, torch.float32)
    assert rec.calls[0][0] == "ffc_kernel_ifft_grad" and rec.calls[0][1][4] == plan.seqlen and dk.shape == (H, 7)
    del rec.calls[:]
    dk, dk_rev = F.dk_from(mod, plan, ws, B, H, 7, torch.float32, (5, torch.float64))
    assert [c[0] for c in rec.calls] == ["ffc_kernel_ifft_grad_bi"] and rec.calls[0][1][2:5] == (B, H, 7) and rec.calls[0][1][6] == 5
    assert dk.shape == (H, 7) and dk_rev.shape == (H, 5) and dk_rev.dtype == torch.float64
