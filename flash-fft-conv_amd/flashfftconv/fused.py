"""The fused host path: what a convolution on a fused plan (fft 256 ... 131072) does on the host, in one place -- one forward, one
backward, one k_f step, one keep step, one dk step.  Three callers, which differ only in how they address their rows:

    FlashFFTConv (conv.py)                 contiguous (B, H, L) tensors                          rows_of(t)
    gated_conv_from_slices (hyena.py)      channel slices of one (B, 3D, L) tensor, in place     rows_of(uc, j * D * L, 3 * D * L)
    BatchShardedFFTConv (sharding.py)      head ranges [g0, g1) of (B, H, L) tensors, in place   rows_of(t, g0 * L, H * L)

Route selection (who runs on a fused plan at all) stays with the callers; the budget of the kept spectra, the k -> k_f launches and the
plans stay in conv.py, which this module reads at call time (conv.py imports this module too: neither uses the other while importing)."""
import ctypes
import torch

from . import _lib
from . import conv as _C

NULL = (None, 0)


def rows_of(t, offset=0, stride=0):
    """Row operand of forward / backward: (pointer to row (0, 0), batch stride in elements, 0 = contiguous) of a tensor whose rows
    (b, h) start at offset + b * stride + h * L elements.  No tensor: a null pointer with the same stride."""
    return (None if t is None else ctypes.c_void_p(t.data_ptr() + offset * t.element_size()), stride)


def forward(plan, B, H, L, u, kf, pre, post, y, addend=NULL, z=None, yraw=None, rows=0, conj=False):
    """y = post * conv(u * pre, k) [+ addend] of B x H rows of L samples; u, pre, post, y, addend: rows_of operands (pre / post / addend
    NULL when absent), kf the filter's k_f.  z / yraw: buffers for the spectra FFT(u * pre) and for the output before `post` and
    `addend`, kept for the backward.  rows > 0: the kernel that skips the dead spectrum rows of a low-pass k_f (conv._sparse_rows)."""
    lib, kf, s = _lib.lib(), _lib.ptr(kf), _lib.stream_ptr()
    if addend[0] is not None:
        _lib.check(lib.ffc_conv_fwd_res(plan.handle, u[0], kf, pre[0], post[0], addend[0], y[0], _lib.ptr(z), _lib.ptr(yraw), B, H, L,
                                        int(conj), u[1], pre[1], post[1], addend[1], y[1], s), "ffc_conv_fwd_res")
    elif z is not None or yraw is not None:
        _lib.check(lib.ffc_conv_fwd_z(plan.handle, u[0], kf, pre[0], post[0], y[0], _lib.ptr(z), _lib.ptr(yraw), B, H, L,
                                      u[1], pre[1], post[1], y[1], s), "ffc_conv_fwd_z")
    elif u[1] or pre[1] or post[1] or y[1]:
        _lib.check(lib.ffc_conv_fwd_strided(plan.handle, u[0], kf, pre[0], post[0], y[0], B, H, L, int(conj),
                                            u[1], pre[1], post[1], y[1], s), "ffc_conv_fwd_strided")
    elif rows:
        _lib.check(lib.ffc_conv_fwd_sparse(plan.handle, u[0], kf, pre[0], post[0], y[0], B, H, L, int(conj), rows, s), "ffc_conv_fwd_sparse")
    else:
        _lib.check(lib.ffc_conv_fwd(plan.handle, u[0], kf, pre[0], post[0], y[0], B, H, L, int(conj), s), "ffc_conv_fwd")


def backward(plan, B, H, L, dout, u, kf, pre, post, du, dpre, dpost, ws, z=None, yraw=None, rows=0):
    """One fused launch: du (+ dpre, dpost when gated) into their rows_of operands and the fp32 dk_f partial sums into ws
    (conv._ws_bytes; dk_from finishes them).  z / yraw: what forward kept.  rows > 0: the recomputing kernel on the live spectrum
    rows, which writes only those rows of the slabs (conv._ifft_grad_sparse finishes them)."""
    lib, kf, s = _lib.lib(), _lib.ptr(kf), _lib.stream_ptr()
    if rows:
        _lib.check(lib.ffc_conv_bwd_sparse(plan.handle, dout[0], u[0], kf, pre[0], post[0], du[0], dpre[0], dpost[0], _lib.ptr(ws), None,
                                           B, H, L, rows, s), "ffc_conv_bwd_sparse")
    elif pre[0] is not None and (z is not None or yraw is not None):
        # dpostgate = dout * y_raw out of the kernel's dout row load (round 3: a torch elementwise kernel, 3 x |u| bytes more)
        _lib.check(lib.ffc_conv_bwd_zy(plan.handle, dout[0], u[0], kf, pre[0], post[0], du[0], dpre[0], dpost[0], _lib.ptr(ws), _lib.ptr(z),
                                       _lib.ptr(yraw), B, H, L, dout[1], u[1], pre[1], post[1], du[1], dpre[1], dpost[1], s), "ffc_conv_bwd_zy")
    elif z is not None:
        _lib.check(lib.ffc_conv_bwd_z(plan.handle, dout[0], u[0], kf, pre[0], post[0], du[0], dpre[0], None, _lib.ptr(ws), _lib.ptr(z),
                                      B, H, L, dout[1], u[1], pre[1], post[1], du[1], dpre[1], dpost[1], s), "ffc_conv_bwd_z")
    elif dout[1] or u[1] or pre[1] or post[1] or du[1] or dpre[1] or dpost[1]:
        _lib.check(lib.ffc_conv_bwd_gated_strided(plan.handle, dout[0], u[0], kf, pre[0], post[0], du[0], dpre[0], dpost[0], _lib.ptr(ws),
                                                  B, H, L, dout[1], u[1], pre[1], post[1], du[1], dpre[1], dpost[1], s),
                   "ffc_conv_bwd_gated_strided")
    else:
        _lib.check(lib.ffc_conv_bwd_gated(plan.handle, dout[0], u[0], kf, pre[0], post[0], du[0], dpre[0], dpost[0], _lib.ptr(ws),
                                          B, H, L, s), "ffc_conv_bwd_gated")


def forward_k(mod, plan, k, u, pregate, postgate, z, yraw):
    """the module's forward in one C-ABI call, k -> k_f + the convolution (ffc_conv_fwd_k), on contiguous tensors -> (y, k_f)"""
    B, H, L = u.shape
    k32 = k if (k.dtype == torch.float32 and k.is_contiguous()) else k.detach().to(torch.float32).contiguous()
    kf = torch.empty(H, plan.kf_elems, 2, dtype=plan.dtype, device=u.device)
    y = torch.empty_like(u)
    _lib.check(_lib.lib().ffc_conv_fwd_k(plan.handle, _lib.ptr(k32), k32.shape[-1], _lib.ptr(kf), _lib.ptr(u), _lib.ptr(pregate),
                                         _lib.ptr(postgate), _lib.ptr(y), _lib.ptr(z), _lib.ptr(yraw), B, H, L,
                                         _lib.stream_ptr()), "ffc_conv_fwd_k")
    if mod.cache_kf and not k.requires_grad:
        mod._kf_cache = (_C._kf_key(k), kf)
    return y, kf


def backward_k(plan, dout, u, kf, pregate, postgate, du, dpre, dpost, ws, z, yraw, k_len):
    """the module's backward in one C-ABI call: the fused backward (on the kept spectra when there are any) + dk_f -> dk
    (ffc_conv_bwd_k), on contiguous tensors -> dk (H, k_len) fp32"""
    B, H, L = u.shape
    dk = torch.empty(H, k_len, dtype=torch.float32, device=u.device)
    _lib.check(_lib.lib().ffc_conv_bwd_k(plan.handle, _lib.ptr(dout), _lib.ptr(u), _lib.ptr(kf), _lib.ptr(pregate), _lib.ptr(postgate),
                                         _lib.ptr(du), _lib.ptr(dpre), _lib.ptr(dpost), _lib.ptr(ws), _lib.ptr(z), _lib.ptr(yraw), _lib.ptr(dk),
                                         k_len, B, H, L, _lib.stream_ptr()), "ffc_conv_bwd_k")
    return dk


def cached_kf(mod, k, k_rev=None, slot="_kf_cache"):
    """the inference cache's k_f of this filter (mod.cache_kf, a filter that does not require grad, the same storage at the same
    version), or None"""
    if not mod.cache_kf or k.requires_grad or (k_rev is not None and k_rev.requires_grad):
        return None
    c = getattr(mod, slot, None)
    return c[1] if c is not None and c[0] == _C._kf_key2(k, k_rev) else None


def kf_for(mod, plan, k, k_rev=None, slot="_kf_cache"):
    """k_f of a filter as a launch of its own: from the cache slot, or k -> k_f of the plain row, of the bidirectional pair (k, k_rev),
    or of the periodised row of the folded fft-2048 plan; a frequency-sparse module's mask applied; stored in the slot"""
    kf = cached_kf(mod, k, k_rev, slot)
    if kf is not None:
        return kf
    if k_rev is not None:
        kf = _C._kernel_fft_bi(plan, k, k_rev)
    else:
        kf = _C._kernel_fft(plan, _C._periodise_k(k, mod.seqlen) if mod._folded else k)
    if mod._kf_keep is not None:       # frequency-sparse k_f (flashfftconv/sparse_conv.py)
        kf.mul_(mod._kf_mask(plan, kf.dtype)[None, :, None])
    if mod.cache_kf and not k.requires_grad and not (k_rev is not None and k_rev.requires_grad):
        setattr(mod, slot, (_C._kf_key2(k, k_rev), kf))
    return kf


def keep(mod, plan, B, H, like, gated, wants_grad, y_only=False):
    """What a training forward keeps for the backward -> (z, yraw), either may be None.
    MI355X design (memory laid out for 288 GB of HBM): a training forward keeps every pair's spectrum FFT(u * pregate) (2x the
    bytes of u at L = N/2) so that the backward pass does not transform u a second time: its kernel runs two transforms per pair
    instead of three (fused backward -30 % at B16 H768 fft 32768, profiles/r03_spectrum.txt).  The gated form also keeps the output
    before the postgate multiply (1x the bytes of u): dpostgate = dout * that, instead of one more inverse transform of the
    spectrum.  module.save_spectrum = False (or FFC_SAVE_SPECTRUM=0) keeps the reference's recomputing backward.
    like: a tensor with the rows' dtype, device and length.  wants_grad: the caller's own conditions (training, a graph being
    recorded, an input that requires grad).  y_only: yraw WITHOUT the spectra (the module's choice, conv._Y_ONLY_MAX)."""
    if not (wants_grad and mod.save_spectrum):
        return None, None
    z = None if y_only else _C._spectrum_buffer(plan, B, H, like.device, gated, mod.save_spectrum)
    yraw = None
    if gated and (z is not None or y_only):
        try:
            yraw = torch.empty(B, H, like.shape[-1], dtype=like.dtype, device=like.device)
        except torch.cuda.OutOfMemoryError:      # no spectra without their y_raw: the recomputing backward
            z = None
    return z, yraw


def dkf_slabs(plan, ws, B, H):
    """the fp32 dk_f partial sums at the head of a backward workspace: (nslab, H, kf_elems, 2), k_f's internal order"""
    nslab = _lib.lib().ffc_dkf_slab_count(plan.handle, B, H)
    return ws[: nslab * H * plan.kf_elems * 8].view(torch.float32).view(nslab, H, plan.kf_elems, 2)


def dkf_sum(plan, ws, B, H):
    """those slabs summed over the batch chunks: dk_f (H, kf_elems, 2) fp32"""
    slabs = dkf_slabs(plan, ws, B, H)
    return slabs[0] if slabs.shape[0] == 1 else slabs.sum(0)


def dk_from(mod, plan, ws, B, H, k_len, k_dtype, rev=None):
    """dk_f partial sums -> (dk (H, k_len) in k_dtype, dk_rev or None).  rev = (Lr, dtype) of a bidirectional filter's k_rev: both
    halves of its gradient from one inverse."""
    n = plan.seqlen if mod._folded else k_len
    dk_rev = None
    if rev is not None:
        dk, dk_rev = _C._ifft_grad_bi(plan, ws, B, H, n, rev[0], ws.device)
        dk_rev = dk_rev.to(rev[1])
    else:
        dk = torch.empty(H, n, dtype=torch.float32, device=ws.device)
        _lib.check(_lib.lib().ffc_kernel_ifft_grad(plan.handle, _lib.ptr(ws), B, H, n, _lib.ptr(dk), _lib.stream_ptr()), "ffc_kernel_ifft_grad")
    if mod._folded:      # chain rule of conv._periodise_k
        dk = (dk[:, :mod.seqlen] + dk[:, mod.seqlen:])[:, :k_len]
    return dk.to(k_dtype), dk_rev


def pack_kept(tensors):
    """optional tensors for save_for_backward: a tuple with None holes (or None altogether) -> (layout, the tensors that are there)"""
    if tensors is None:
        return None, ()
    return tuple([t is not None for t in tensors]), tuple([t for t in tensors if t is not None])


def unpack_kept(layout, saved):
    """the tuple pack_kept was given, rebuilt from its layout and the saved tensors (a sequence that starts with them, or an iterator
    that several calls share)"""
    if layout is None:
        return None
    it = iter(saved)
    return tuple([next(it) if present else None for present in layout])
