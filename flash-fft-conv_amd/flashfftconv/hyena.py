"""Fused Hyena / Monarch-Mixer sequence operator on the MI355X kernels.

The reference's callers build the gated long convolution out of separate kernels around FlashFFTConv
(examples/hyena-dna/hyenadna_flashfftconv.py:269-289, examples/bert/monarch_mixer_sequence_mixer_flashfftconv.py:118-175):

    uc = flash_short_filter(u)[..., :l]            # depthwise k=3 conv over the 3*D projected channels
    x1, x2, v = uc.split(d_model, dim=1)           # three (B, D, L) channel slices (non-contiguous)
    x1v = (x1 * v).contiguous()                    # elementwise kernel + copy
    y = flashfftconv(x1v, k)                       # FFT convolution
    y = y * x2                                     # elementwise kernel
    y = y + flashfftconv(v.contiguous(), k2)       # M2-BERT with residual_long_conv=True: copy, second convolution, add kernel

Here the three slices are handed to the gated FFT-conv kernel IN PLACE (batch-strided rows, ffc_conv_fwd_strided): v is the
input, x1 the pregate, x2 the postgate, so the multiply kernels, the copy and their HBM round trips disappear, in the forward
and in the backward (du / dpregate / dpostgate are written straight into the slices of d(uc), one launch; then the short
convolution's own backward).  y = x2 * conv(x1 * v, k): the same function as the reference composition.

The HBM-level routes (fft >= 262144, and fft 131072 with rows longer than half of it: flashfftconv/bigfft.py) do the same through the
batch pitches of their level kernels (ffc_outer_pass*_strided): the first forward level of every transform reads v, x1, x2 (and, in the
backward, writes du, dpregate, dpostgate through the last inverse level) as slices of uc / d(uc) -- _GatedSlicesBigFn.

With k_res (the M2 residual long convolution, monarch_mixer_sequence_mixer_flashfftconv.py:151-175) y = x2 * conv(x1 * v, k) +
conv(v, k_res) in two launches: conv(v, k_res) reading the v slice in place, then the gated kernel with that result as the addend of its
output epilogue (ffc_conv_fwd_res) -- no copy of v and no add kernel."""
import torch

from . import _lib
from .conv import (FlashFFTConv, _check_inputs, _kernel_fft, _periodise_k, _spectrum_buffer, _kf_key, _apply_noting_grad_mode, _recording,
                   _big_forward_routed, _big_backward, _dev_ctx, _TorchOps, _kernel_fft_bi, _ifft_grad_bi, _compose_k_full, _kf_key2,
                   _check_k_rev)
from . import bigfft as _bigfft
from .depthwise_1d import FlashDepthWiseConv1d


def _slice_ptr(t, j, D, L):
    return _lib.ctypes.c_void_p(t.data_ptr() + j * D * L * t.element_size())


class _GatedSlicesFn(torch.autograd.Function):
    """y = uc[:, 1] * conv(uc[:, 0] * uc[:, 2], k) [+ conv(uc[:, 2], k_res)] for uc viewed as (B, 3, D, L): x1 = slice 0, x2 = slice 1,
    v = slice 2.  k_rev / k_res_rev: the reversed halves of bidirectional filters (FlashFFTConv.forward), read by the k -> k_f kernel and
    their gradients written by the dk_f -> dk kernel (unfolded modules only: gated_conv_from_slices composes the others)."""

    @staticmethod
    def forward(ctx, uc, k, mod, k_res=None, k_rev=None, k_res_rev=None):
        B, D3, L = uc.shape
        D = D3 // 3
        plan = mod._get_plan(uc.device, mod._plan_seqlen)
        if (k_rev is not None or k_res_rev is not None) and mod._folded:
            raise RuntimeError("FlashHyenaOp: internal: a reversed filter on a folded plan")
        with torch.cuda.device(uc.device):
            cache = mod.cache_kf and not k.requires_grad and not (k_rev is not None and k_rev.requires_grad)
            kf = mod._cached_kf(k, k_rev) if cache else None      # inference cache, as FlashFFTConv
            if kf is None:
                if k_rev is not None:
                    kf = _kernel_fft_bi(plan, k, k_rev)
                else:
                    kf = _kernel_fft(plan, _periodise_k(k, mod.seqlen) if mod._folded else k)
                if cache:
                    mod._kf_cache = (_kf_key2(k, k_rev), kf)
            y = torch.empty(B, D, L, dtype=uc.dtype, device=uc.device)
            sb = D3 * L
            kf_res = yu = None
            if k_res is not None:
                # launch 1: yu = conv(v, k_res), v read in place; its k_f has a cache slot of its own (k and k_res would evict each other)
                cache_res = mod.cache_kf and not k_res.requires_grad and not (k_res_rev is not None and k_res_rev.requires_grad)
                c = getattr(mod, "_kf_cache_res", None) if cache_res else None
                kf_res = c[1] if c is not None and c[0] == _kf_key2(k_res, k_res_rev) else None
                if kf_res is None:
                    if k_res_rev is not None:
                        kf_res = _kernel_fft_bi(plan, k_res, k_res_rev)
                    else:
                        kf_res = _kernel_fft(plan, _periodise_k(k_res, mod.seqlen) if mod._folded else k_res)
                    if cache_res:
                        mod._kf_cache_res = (_kf_key2(k_res, k_res_rev), kf_res)
                yu = torch.empty_like(y)
                _lib.check(_lib.lib().ffc_conv_fwd_strided(plan.handle, _slice_ptr(uc, 2, D, L), _lib.ptr(kf_res), None, None, _lib.ptr(yu),
                                                           B, D, L, 0, sb, 0, 0, 0, _lib.stream_ptr()), "ffc_conv_fwd_strided")
            # training: keep the spectra FFT(x1 * v) and the output before the x2 multiply (FlashFFTConv.save_spectrum)
            z = yraw = None
            if mod.training and mod.save_spectrum and _recording() and any(ctx.needs_input_grad[:2]):
                z = _spectrum_buffer(plan, B, D, uc.device, True, mod.save_spectrum)
                if z is not None:
                    try:
                        yraw = torch.empty_like(y)
                    except torch.cuda.OutOfMemoryError:
                        z = None
            if yu is not None:
                # launch 2: the gated kernel with yu as the addend of its output epilogue (z / yraw nullable: the output before x2 and yu)
                _lib.check(_lib.lib().ffc_conv_fwd_res(plan.handle, _slice_ptr(uc, 2, D, L), _lib.ptr(kf), _slice_ptr(uc, 0, D, L),
                                                       _slice_ptr(uc, 1, D, L), _lib.ptr(yu), _lib.ptr(y), _lib.ptr(z), _lib.ptr(yraw), B, D, L,
                                                       0, sb, sb, sb, 0, 0, _lib.stream_ptr()), "ffc_conv_fwd_res")
            elif z is None:
                _lib.check(_lib.lib().ffc_conv_fwd_strided(plan.handle, _slice_ptr(uc, 2, D, L), _lib.ptr(kf), _slice_ptr(uc, 0, D, L),
                                                           _slice_ptr(uc, 1, D, L), _lib.ptr(y), B, D, L, 0, sb, sb, sb, 0,
                                                           _lib.stream_ptr()), "ffc_conv_fwd_strided")
            else:
                _lib.check(_lib.lib().ffc_conv_fwd_z(plan.handle, _slice_ptr(uc, 2, D, L), _lib.ptr(kf), _slice_ptr(uc, 0, D, L),
                                                     _slice_ptr(uc, 1, D, L), _lib.ptr(y), _lib.ptr(z), _lib.ptr(yraw), B, D, L,
                                                     sb, sb, sb, 0, _lib.stream_ptr()), "ffc_conv_fwd_z")
        ctx.mod, ctx.k_len, ctx.k_dtype = mod, k.shape[-1], k.dtype
        ctx.res = None if k_res is None else (k_res.shape[-1], k_res.dtype)
        ctx.rev = None if k_rev is None else (k_rev.shape[-1], k_rev.dtype)
        ctx.res_rev = None if k_res_rev is None else (k_res_rev.shape[-1], k_res_rev.dtype)
        if mod.training:
            ctx.save_for_backward(*((uc, kf) + (() if z is None else (z, yraw)) + (() if kf_res is None else (kf_res,))))
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.saved_tensors:
            raise RuntimeError("FlashHyenaOp: backward needs module.training=True at forward time")
        uc, kf = ctx.saved_tensors[:2]
        rest = ctx.saved_tensors[2:]
        kf_res = None
        if ctx.res is not None:
            rest, kf_res = rest[:-1], rest[-1]
        z, yraw = rest[:2] if len(rest) >= 2 else (None, None)
        mod = ctx.mod
        B, D3, L = uc.shape
        D = D3 // 3
        plan = mod._get_plan(uc.device, mod._plan_seqlen)
        lib = _lib.lib()
        with torch.cuda.device(uc.device):
            dy = dy.contiguous()
            duc = torch.empty_like(uc)
            ws = torch.empty(lib.ffc_dkf_workspace_bytes(plan.handle, B, D), dtype=torch.uint8, device=uc.device)
            sb = D3 * L
            # u = v (slice 2), pregate = x1 (slice 0), postgate = x2 (slice 1); gradients land in the same slices of duc
            if z is not None:
                # d x2 = dy * (output before the x2 multiply): written into its slice of duc by the kernel's dy row load
                _lib.check(lib.ffc_conv_bwd_zy(plan.handle, _lib.ptr(dy), _slice_ptr(uc, 2, D, L), _lib.ptr(kf),
                                               _slice_ptr(uc, 0, D, L), _slice_ptr(uc, 1, D, L), _slice_ptr(duc, 2, D, L),
                                               _slice_ptr(duc, 0, D, L), _slice_ptr(duc, 1, D, L), _lib.ptr(ws), _lib.ptr(z), _lib.ptr(yraw),
                                               B, D, L, 0, sb, sb, sb, sb, sb, sb, _lib.stream_ptr()), "ffc_conv_bwd_zy")
            else:
              _lib.check(lib.ffc_conv_bwd_gated_strided(plan.handle, _lib.ptr(dy), _slice_ptr(uc, 2, D, L), _lib.ptr(kf),
                                                      _slice_ptr(uc, 0, D, L), _slice_ptr(uc, 1, D, L), _slice_ptr(duc, 2, D, L),
                                                      _slice_ptr(duc, 0, D, L), _slice_ptr(duc, 1, D, L), _lib.ptr(ws), B, D, L,
                                                      0, sb, sb, sb, sb, sb, sb, _lib.stream_ptr()), "ffc_conv_bwd_gated_strided")
            k_len = plan.seqlen if mod._folded else ctx.k_len
            dk_rev = dk_res_rev = None
            if ctx.rev is not None:
                dk, dk_rev = _ifft_grad_bi(plan, ws, B, D, k_len, ctx.rev[0], uc.device)
                dk_rev = dk_rev.to(ctx.rev[1])
            else:
                dk = torch.empty(D, k_len, dtype=torch.float32, device=uc.device)
                _lib.check(lib.ffc_kernel_ifft_grad(plan.handle, _lib.ptr(ws), B, D, k_len, _lib.ptr(dk), _lib.stream_ptr()),
                           "ffc_kernel_ifft_grad")
            if mod._folded:
                n = mod.seqlen
                dk = (dk[:, :n] + dk[:, n:])[:, :ctx.k_len]
            dk_res = None
            if kf_res is not None:
                # the residual branch yu = conv(v, k_res): the ungated fused backward on (dy, v in place, kf_res) -> dk_res and a (B, D, L)
                # input gradient, added into v's slice of duc (the workspace is free again: stream order)
                dv = torch.empty_like(dy)
                _lib.check(lib.ffc_conv_bwd_gated_strided(plan.handle, _lib.ptr(dy), _slice_ptr(uc, 2, D, L), _lib.ptr(kf_res), None, None,
                                                          _lib.ptr(dv), None, None, _lib.ptr(ws), B, D, L, 0, sb, 0, 0, 0, 0, 0,
                                                          _lib.stream_ptr()), "ffc_conv_bwd_gated_strided")
                kr_len = plan.seqlen if mod._folded else ctx.res[0]
                if ctx.res_rev is not None:
                    dk_res, dk_res_rev = _ifft_grad_bi(plan, ws, B, D, kr_len, ctx.res_rev[0], uc.device)
                    dk_res_rev = dk_res_rev.to(ctx.res_rev[1])
                else:
                    dk_res = torch.empty(D, kr_len, dtype=torch.float32, device=uc.device)
                    _lib.check(lib.ffc_kernel_ifft_grad(plan.handle, _lib.ptr(ws), B, D, kr_len, _lib.ptr(dk_res), _lib.stream_ptr()),
                               "ffc_kernel_ifft_grad")
                if mod._folded:
                    n = mod.seqlen
                    dk_res = (dk_res[:, :n] + dk_res[:, n:])[:, :ctx.res[0]]
                dk_res = dk_res.to(ctx.res[1])
                duc[:, 2 * D:].add_(dv)
        return duc, dk.to(ctx.k_dtype), None, dk_res, dk_rev, dk_res_rev      # (the caller passes every filter slot, None included)


class _GatedSlicesBigFn(torch.autograd.Function):
    """_GatedSlicesFn on the HBM-level routes: the module's own forward / backward of these sizes (conv._big_forward / _big_backward: levels,
    inner kernel, what is kept for the backward) with v, x1, x2 passed as VIEWS of uc and du, dpregate, dpostgate as views of one
    duc = empty_like(uc) -- the levels address them through their batch pitch.  Same kernels and arithmetic as the module called on
    contiguous copies, so the same bits.  With k_res, conv(v, k_res) is a second (ungated) call on the v view whose result is added by
    composition, as the module does at these sizes (no fused epilogue in the last inverse level); its input gradient is added into v's
    slice of duc."""

    @staticmethod
    def forward(ctx, uc, k, mod, k_res=None):
        B, D3, L = uc.shape
        D = D3 // 3
        x1, x2, v = uc[:, :D], uc[:, D:2 * D], uc[:, 2 * D:]
        with _dev_ctx(uc.device):
            y = torch.empty(B, D, L, dtype=uc.dtype, device=uc.device)
            _, kf, kept, fac, half = _big_forward_routed(mod, v, k, x1, x2, any(ctx.needs_input_grad[:2]), y)
            res = None
            if k_res is not None:
                yr, kf_r, kept_r, fac_r, half_r = _big_forward_routed(mod, v, k_res, None, None, ctx.needs_input_grad[0] or ctx.needs_input_grad[3])
                y = y + yr
                res = (kf_r, kept_r, fac_r, half_r, k_res.shape[-1], k_res.dtype)
        ctx.mod, ctx.k_len, ctx.k_dtype, ctx.fac, ctx.half = mod, k.shape[-1], k.dtype, fac, half
        ctx.layouts = ctx.res = None
        if mod.training:
            saved, layouts = [uc], []
            for kf_, kept_ in ((kf, kept),) + (() if res is None else (res[:2],)):
                layouts.append(None if kept_ is None else tuple(t is not None for t in kept_))
                saved += [kf_] + ([] if kept_ is None else [t for t in kept_ if t is not None])
            ctx.layouts = layouts
            ctx.res = None if res is None else res[2:]
            ctx.save_for_backward(*saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.saved_tensors:
            raise RuntimeError("FlashHyenaOp: backward needs module.training=True at forward time")
        it = iter(ctx.saved_tensors)
        uc = next(it)
        calls = []
        for layout in ctx.layouts:
            kf = next(it)
            calls.append((kf, None if layout is None else tuple(next(it) if present else None for present in layout)))
        mod = ctx.mod
        B, D3, L = uc.shape
        D = D3 // 3
        x1, x2, v = uc[:, :D], uc[:, D:2 * D], uc[:, 2 * D:]
        with _dev_ctx(uc.device):
            dy = dy.contiguous()
            duc = torch.empty_like(uc)
            # u = v (slice 2), pregate = x1 (slice 0), postgate = x2 (slice 1); gradients land in the same slices of duc
            outs = (duc[:, 2 * D:], duc[:, :D], duc[:, D:2 * D])
            _, dk, _, _ = _big_backward(mod, dy, v, calls[0][0], x1, x2, ctx.k_len, calls[0][1], False, ctx.fac, ctx.half, outs)
            dk_res = None
            if ctx.res is not None:
                fac_r, half_r, kr_len, kr_dtype = ctx.res
                dv, dk_res, _, _ = _big_backward(mod, dy, v, calls[1][0], None, None, kr_len, calls[1][1], False, fac_r, half_r)
                dk_res = dk_res.to(kr_dtype)
                duc[:, 2 * D:].add_(dv)
        return duc, dk.to(ctx.k_dtype), None, dk_res


def gated_conv_from_slices(conv, uc, k, k_res=None, k_rev=None, k_res_rev=None):
    """y = x2 * conv(x1 * v, k) [+ conv(v, k_res)] with (x1, x2, v) = uc.split(D, dim=1), uc (B, 3D, L) contiguous, through `conv`
    (a FlashFFTConv).  Every route reads the slices in place and writes the gradients into the slices of one d(uc): the fused kernels
    (fft <= 131072) through their strided launchers, the HBM-level routes (fft >= 262144, fft 131072 with rows longer than half of it)
    through the batch pitches of their level kernels, at any L (odd L: element-wise accesses).  Contiguous copies of the slices and the
    module's gated call (same result) remain for the frequency-sparse modules, the wide form of a level (FFC_BIG_WIDE=1), a
    non-contiguous uc and uc.numel() >= 2^31.  k_res (D, Lk2) fp32: the M2 residual long convolution, added in the gated kernel's
    output epilogue on the fused routes and by composition (a second convolution reading v in place, one add) on the HBM-level ones.
    Both convolutions run on ONE module, fitted to the longer of the two filters (_fit_seqlen); the composition conv(v, k, x1, x2,
    residual=conv(v, k_res)) fits each call to its own filter.  Nothing wraps at either size, so the results agree to rounding; they are the
    same bits when both filters select the same fft size.
    k_rev / k_res_rev (D, Lr) fp32: the reversed halves of bidirectional filters, FlashFFTConv.forward's k_rev for k and for k_res (M2-BERT
    builds both filters that way).  On the fused routes the k -> k_f kernel reads the two tensors of a filter and the dk_f -> dk kernel writes
    both gradients, each filter with its own cache slot; the fft size is conv.seqlen (a bidirectional filter fills it: no fitting).  The
    HBM-level routes (which include fft 131072 here), folded and frequency-sparse modules and every case that falls back to contiguous
    copies build the full rows with torch ops (conv._compose_k_full) and run as without the reversed tensors."""
    if uc.dim() != 3 or uc.shape[1] % 3:
        raise RuntimeError("gated_conv_from_slices: uc must be (B, 3*D, L)")
    D, L = uc.shape[1] // 3, uc.shape[2]
    if k_res is not None and (not torch.is_tensor(k_res) or k_res.dim() != 2 or k_res.shape[0] != D):
        raise RuntimeError(f"gated_conv_from_slices: k_res must be (D = {D}, Lk)")
    if k_rev is not None or k_res_rev is not None:
        if k_res_rev is not None and k_res is None:
            raise RuntimeError("gated_conv_from_slices: k_res_rev needs k_res")
        for what, t in (("k_rev", k_rev), ("k_res_rev", k_res_rev)):
            if t is not None:
                _check_k_rev(what, t, D, conv.seqlen, uc.device)
        N = conv.seqlen
        wide = (uc.shape[0] - 1) * 3 * D * L + D * L >= 2 ** 31
        fused = (torch.is_tensor(k) and k.dim() == 2 and not conv._k_rev_composes() and (D * L) % 8 == 0 and uc.is_contiguous() and not wide)
        if not fused:
            _check_inputs(conv, uc[:, :D], k, ())
            if k_res is not None:
                _check_inputs(conv, uc[:, :D], k_res, ())
            kk = k if k_rev is None else _compose_k_full(k, k_rev, N)
            kk_res = k_res if k_res_rev is None else _compose_k_full(k_res, k_res_rev, N)
            return gated_conv_from_slices(conv, uc, kk, kk_res)
        _check_inputs(conv, uc[:, :D], k, ())
        if k_res is not None:
            _check_inputs(conv, uc[:, :D], k_res, ())
        return _apply_noting_grad_mode(_GatedSlicesFn, uc, k, conv, k_res, k_rev, k_res_rev)
    # a model built for its longest sequence and run on a shorter one: the smallest fft size that holds the rows (FlashFFTConv._fit_seqlen)
    lk = k.shape[-1] if k_res is None or k.dim() != 2 else max(k.shape[-1], k_res.shape[-1])
    n = conv._fit_seqlen(L, lk) if k.dim() == 2 else conv.seqlen
    if n != conv.seqlen:
        conv = conv._fitted_module(n)
    # (the strided launchers address one tensor with 31-bit element offsets: (B-1) * 3*D*L + D*L has to stay below 2^31,
    # where the composition on contiguous copies only needs B*D*L < 2^31)
    too_wide = (uc.shape[0] - 1) * 3 * D * L + D * L >= 2 ** 31
    # HBM-level route or fused route: decided per filter by its own length, as the module does for conv(v, k) and conv(v, k_res)
    lks = (k.shape[-1],) + (() if k_res is None else (k_res.shape[-1],))
    bigs = [k.dim() == 2 and bool(conv._big or conv._route_big(max(L, lkx))) for lkx in lks]
    big = all(bigs)
    if big:
        # the level routes: no (D * L) % 8 condition (unaligned slices take the element-wise path); not the wide form of a level
        fit = conv._kf_keep is None and uc.is_contiguous() and uc.numel() < 2 ** 31
        for lkx in lks:
            factors, _ = _bigfft.choose(conv.seqlen, max(L, lkx), _TorchOps)
            fit = fit and not _bigfft.is_wide(factors[0], conv.seqlen // factors[0], max(L, lkx))
    elif any(bigs):
        fit = False      # (fft 131072 with one filter routed by length and one not: the composition on copies)
    else:
        fit = not conv._big and conv._kf_keep is None and (D * L) % 8 == 0 and uc.is_contiguous() and not too_wide
    if not fit:
        x1, x2, v = (t.contiguous() for t in uc.split(D, dim=1))
        return conv(v, k, x1, x2) if k_res is None else conv(v, k, x1, x2, residual=conv(v, k_res))
    _check_inputs(conv, uc[:, :D], k, ())
    if k_res is not None:
        _check_inputs(conv, uc[:, :D], k_res, ())
    if big:
        return _apply_noting_grad_mode(_GatedSlicesBigFn, uc, k, conv, k_res)
    return _apply_noting_grad_mode(_GatedSlicesFn, uc, k, conv, k_res, None, None)


class FlashHyenaOp(torch.nn.Module):
    """short depthwise conv (k = 3, "same" length) over the 3*D projected channels, then y = x2 * fftconv(x1 * v, k).

    forward(x1x2v, k, k_res=None, k_rev=None, k_res_rev=None): x1x2v (B, 3*D, L) bf16/fp16 (the in-projection's output, channels first), k (D, Lk) fp32 -> (B, D, L);
    with k_res (D, Lk2) fp32, y = x2 * fftconv(x1 * v, k) + fftconv(v, k_res) (M2-BERT's residual_long_conv).
    k_rev / k_res_rev (D, Lr) fp32: the reversed halves of bidirectional filters (FlashFFTConv.forward's k_rev, for k and for k_res).
    `short_filter_weight` (3D, 1, 3) or (3D, 3) and `short_filter_bias` (3D,) are the nn.Conv1d parameters the reference
    callers pass to FlashDepthWiseConv1d (hyenadna_flashfftconv.py:248-261: padding=1, i.e. the [..., :l] crop is a no-op)."""

    def __init__(self, d_model, fft_size, short_filter_weight, short_filter_bias, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.d_model = d_model
        self.short_filter = FlashDepthWiseConv1d(3 * d_model, 3, 1, short_filter_weight, short_filter_bias, is_bhl=True,
                                                 device=device, dtype=dtype)
        self.flashfftconv = FlashFFTConv(fft_size, dtype=dtype)

    def forward(self, x1x2v, k, k_res=None, k_rev=None, k_res_rev=None):
        uc = self.short_filter(x1x2v)
        return gated_conv_from_slices(self.flashfftconv, uc, k, k_res, k_rev, k_res_rev)


_LOOP_MAX_BATCH = 16


class _ProjectIn(torch.autograd.Function):
    """(C, D) x (B, L, D) -> (B, C, L): one 2-D GEMM per batch row on the transposed view, forward and backward"""

    @staticmethod
    def forward(ctx, weight, u):
        B, L, _ = u.shape
        w = weight if weight.dtype == u.dtype else weight.to(u.dtype)      # fp32 master weights under mixed precision
        out = torch.empty(B, w.shape[0], L, dtype=u.dtype, device=u.device)
        for b in range(B):
            torch.mm(w, u[b].t(), out=out[b])
        ctx.save_for_backward(w, u)
        ctx.w_dtype = weight.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        weight, u = ctx.saved_tensors
        B = u.shape[0]
        du = dw = None
        if ctx.needs_input_grad[1]:
            du = torch.empty_like(u)
            for b in range(B):
                torch.mm(g[b].t(), weight, out=du[b])              # (L, C) x (C, D), g[b].t() read as a transposed operand
        if ctx.needs_input_grad[0]:
            dw = torch.mm(g[0], u[0])                              # (C, L) x (L, D)
            for b in range(1, B):
                dw.addmm_(g[b], u[b])
            dw = dw.to(ctx.w_dtype)
        return dw, du


class _ProjectOut(torch.autograd.Function):
    """(B, D, L) -> (B, L, C) = y[b]^T W^T + bias: one 2-D GEMM per batch row reading y[b].t() as its transposed operand"""

    @staticmethod
    def forward(ctx, weight, bias, y):
        B, _, L = y.shape
        w = weight if weight.dtype == y.dtype else weight.to(y.dtype)      # fp32 master weights under mixed precision
        bb = bias if bias is None or bias.dtype == y.dtype else bias.to(y.dtype)
        out = torch.empty(B, L, w.shape[0], dtype=y.dtype, device=y.device)
        wt = w.t()
        for b in range(B):
            if bb is None:
                torch.mm(y[b].t(), wt, out=out[b])
            else:
                torch.addmm(bb, y[b].t(), wt, out=out[b])
        ctx.save_for_backward(w, y)
        ctx.has_bias = bias is not None
        ctx.w_dtype, ctx.b_dtype = weight.dtype, (None if bias is None else bias.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        weight, y = ctx.saved_tensors
        B = y.shape[0]
        dw = db = dy = None
        if ctx.needs_input_grad[2]:
            dy = torch.empty_like(y)
            wt = weight.t()
            for b in range(B):
                torch.mm(wt, g[b].t(), out=dy[b])                  # (D, C) x (C, L)
        if ctx.needs_input_grad[0]:
            dw = torch.mm(g[0].t(), y[0].t())                      # (C, L) x (L, D)
            for b in range(1, B):
                dw.addmm_(g[b].t(), y[b].t())
            dw = dw.to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = g.sum(dim=(0, 1)).to(ctx.b_dtype)
        return dw, db, dy


def project_in(weight, u, bias=None):
    """in-projection of a (B, L, D) activation straight into the channels-first layout the convolutions read:
    (C, D) x (B, L, D) -> (B, C, L), one plain 2-D GEMM per batch row on the transposed view u[b].t(), written into its slice of
    the output (forward and backward: _ProjectIn).  The reference callers write `self.in_proj.weight @ u.transpose(-1, -2)`
    (hyenadna_flashfftconv.py:269-270, monarch_mixer_sequence_mixer_flashfftconv.py:124-125, bias dropped there too):
    torch.matmul folds that into a (B*L, D) x (D, C) GEMM and then copies the result into (B, C, L) with a strided elementwise
    kernel -- 224 of its 267 us at B2 L32K D256 on MI355X, 15 % of a HyenaDNA layer (benchmarks/scratch/proj_probe.py).
    (Not torch.bmm on the broadcast weight: on this ROCm 7.0 / PyTorch 2.10 stack the BATCHED GEMM with a transposed-view
    operand writes out of bounds at D = 768, L >= 8192 -- hipBLASLt and rocBLAS alike, the reference's own matmul form included;
    benchmarks/scratch/bmm_fault2.py.  The 2-D GEMM is the path every nn.Linear takes.)"""
    if u.shape[0] > _LOOP_MAX_BATCH:      # many short sequences: one GEMM + the layout copy, which is small there
        # (fp32 master weights under mixed precision: cast like _ProjectIn does; autograd returns the gradient in the weight's dtype)
        out = torch.nn.functional.linear(u, weight if weight.dtype == u.dtype else weight.to(u.dtype)).transpose(-1, -2).contiguous()
    else:
        out = _ProjectIn.apply(weight, u)
    return out if bias is None else out + bias.to(out.dtype).view(1, -1, 1)


def project_out(weight, bias, y):
    """out-projection of a channels-first (B, D, L) result back to (B, L, C): nn.Linear on y.transpose(-1, -2) first copies
    the transposed view (55 of 88 us at the shape above); a 2-D GEMM per batch row reads y[b].t() as its transposed operand."""
    if y.shape[0] > _LOOP_MAX_BATCH:
        w = weight if weight.dtype == y.dtype else weight.to(y.dtype)
        bb = bias if bias is None or bias.dtype == y.dtype else bias.to(y.dtype)
        return torch.nn.functional.linear(y.transpose(-1, -2), w, bb)
    return _ProjectOut.apply(weight, bias, y)


class FlashHyenaMixer(torch.nn.Module):
    """The whole order-2 Hyena operator of the reference callers (hyenadna_flashfftconv.py:228-289 HyenaOperator.forward):
    in_proj -> short depthwise conv -> x2 * fftconv(x1 * v, k) -> out_proj, on (B, L, D) activations, with no layout copy:
    the two projections are GEMMs on transposed views (project_in / project_out), the gates are read in place
    (FlashHyenaOp).  `in_proj` (D -> 3D) and `out_proj` (D -> D) are the caller's nn.Linear modules (shared, not copied);
    the in-projection bias is not applied, as in the reference (`self.in_proj.weight @ u`)."""

    def __init__(self, d_model, fft_size, in_proj, out_proj, short_filter_weight, short_filter_bias, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.in_proj, self.out_proj = in_proj, out_proj
        self.op = FlashHyenaOp(d_model, fft_size, short_filter_weight, short_filter_bias, dtype=dtype, device=device)

    def forward(self, u, k, k_res=None, k_rev=None, k_res_rev=None):
        y = self.op(project_in(self.in_proj.weight, u), k, k_res, k_rev, k_res_rev)
        return project_out(self.out_proj.weight, self.out_proj.bias, y)
