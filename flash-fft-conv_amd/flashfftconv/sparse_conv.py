"""Partial and frequency-sparse convolutions on the MI355X FlashFFTConv kernels.

Same classes, constructor arguments and semantics as the reference's torch.fft demos
(/root/reference/flashfftconv/sparse_conv.py:8-38), but running through the fused HIP path:

  PartialFFTConv(N_partial)(x, k)          y = conv(x, k[..., :N_partial]),             fft size 2L
  PartialFFTConv(N_partial, overlap_save=True)   the same y block by block for N_partial <= 16384: any L, blocks of max(2048, nextpow2(taps))
  PartialFFTConv(..)(x, k, pregate, postgate, residual)   y = postgate * conv(x * pregate, k[..., :N_partial]) + residual, each optional
  PartialFFTConv(.., overlap_save=True)(x, k, .., state=s, return_state=True)   a row in pieces: (y, new state), the filter's history carried over
  PartialFFTConv(.., overlap_save="direct")   the same, pieces of 1 .. 64 samples on the direct step kernels (generation): no transform, one launch
  FrequencySparseFFTConv(N_partial)(x, k)  y = irfft(rfft(x) * rfft(k) * [f < N_partial // 2]), fft size 2L

x is (B, H, L) bf16/fp16 on the GPU, k is (H, Lk) fp32 (the reference demos up-cast x to fp32 and back;
here the module dtype is x's dtype).  Both are differentiable in x and k.  The frequency-sparse variant
zeroes k_f's bins in the library's internal order (mask built once from ffc_plan_kf_index) and masks the
fp32 dk_f partial sums the same way in the backward, at every fft size the module supports (sequence lengths up to 2097152: above
fft 131072 the mask goes onto the inner k_f / dk_f rows of the HBM-level form, flashfftconv/bigfft.py row_freq).
"""
import torch

from . import _lib
from . import conv as _C
from .conv import FlashFFTConv


class _ConvCache(torch.nn.Module):
    def __init__(self, N_partial):
        super().__init__()
        self.N_partial = N_partial
        self._convs = {}

    def _conv_for(self, x, keep=None):
        if not torch.is_tensor(x) or x.dtype not in (torch.bfloat16, torch.float16):
            raise RuntimeError(f"{type(self).__name__}: x must be a bf16 / fp16 tensor, got {getattr(x, 'dtype', type(x))}")
        key = (2 * x.shape[-1], x.dtype)
        conv = self._convs.get(key)
        if conv is None:
            conv = FlashFFTConv(key[0], dtype=x.dtype)
            if keep is not None:
                # (fft sizes with HBM levels, >= 262144: the mask is applied to the inner k_f / dk_f rows, conv._big_kf_mask)
                # folded size (2048 on the 4096 plan): natural bin f of the 2048-point spectrum is bin 2f of the plan
                conv._kf_keep = keep * (conv._plan_seqlen // conv.seqlen)
            self._convs[key] = conv
        conv.train(self.training)
        return conv


OS_MAX_TAPS = 16384      # overlap-save route: the block fft size 2 * nextpow2(taps) stays a single-pass size with an outer digit (<= 32768)


def os_fft_size(taps):
    """block fft size N' of the overlap-save route for a filter of `taps` taps: blocks of S = N' / 2 samples, S >= taps"""
    return max(4096, 2 * (1 << (taps - 1).bit_length()))


def _conv_os(plan, x, kf, conj, wrap):
    """ffc_conv_fwd_os on a contiguous (B, H, L) tensor: every row as ceil(L / S) blocks on the plan's fused kernel"""
    B, H, L = x.shape
    y = torch.empty_like(x)
    _lib.check(_lib.lib().ffc_conv_fwd_os(plan.handle, _lib.ptr(x), _lib.ptr(kf), _lib.ptr(y), B, H, L, int(conj), int(wrap), _lib.stream_ptr()),
               "ffc_conv_fwd_os")
    return y


def _dkf_os(plan, dy, x):
    """ffc_conv_bwd_dkf_os: the fp32 dk_f partial sums over all blocks -> (the kernels' batch B * nblk, the workspace that holds them)"""
    B, H, L = x.shape
    nb = B * (-(-L // (plan.seqlen // 2)))
    ws = torch.empty(_C._ws_bytes(plan, nb, H), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().ffc_conv_bwd_dkf_os(plan.handle, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(ws), B, H, L, _lib.stream_ptr()), "ffc_conv_bwd_dkf_os")
    return nb, ws


class _OverlapSaveFn(torch.autograd.Function):
    """y = conv(x, k) for k of at most S taps, block by block.  Keeps x and k_f only; the backward is the input-gradient launch (conj k_f on
    the natural-order windows of dy), the dk_f launch over all B * nblk blocks and the dk inverse."""

    @staticmethod
    def forward(ctx, x, k, plan):
        with torch.cuda.device(x.device):
            kf = _C._kernel_fft(plan, k)
            y = _conv_os(plan, x, kf, False, True)
        ctx.save_for_backward(x, kf)
        ctx.plan, ctx.k_shape, ctx.k_dtype = plan, tuple(k.shape), k.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, kf = ctx.saved_tensors
        plan, (H, Lk) = ctx.plan, ctx.k_shape
        B, _, L = x.shape
        dy = dy.contiguous()
        dx = dk = None
        with torch.cuda.device(x.device):
            if ctx.needs_input_grad[0]:
                dx = _conv_os(plan, dy, kf, True, False)
            if ctx.needs_input_grad[1]:
                nb, ws = _dkf_os(plan, dy, x)
                dk = torch.empty(H, Lk, dtype=torch.float32, device=x.device)
                _lib.check(_lib.lib().ffc_kernel_ifft_grad(plan.handle, _lib.ptr(ws), nb, H, Lk, _lib.ptr(dk), _lib.stream_ptr()),
                           "ffc_kernel_ifft_grad")
                dk = dk.to(ctx.k_dtype)
        return dx, dk, None


def _conv_os_gated(plan, x, kf, conj, wrap, pregate=None, postgate=None, addend=None, gate2=None):
    """ffc_conv_fwd_os_gated on contiguous (B, H, L) tensors: y = postgate * conv_os(x * pregate) + addend and, with gate2, the second
    output conv_os(x * pregate) * gate2 of the same launch -> (y, out2 or None)"""
    B, H, L = x.shape
    y = torch.empty_like(x)
    out2 = None if gate2 is None else torch.empty_like(x)
    _lib.check(_lib.lib().ffc_conv_fwd_os_gated(plan.handle, _lib.ptr(x), _lib.ptr(kf), _lib.ptr(pregate), _lib.ptr(postgate), _lib.ptr(addend),
                                                _lib.ptr(y), _lib.ptr(gate2), _lib.ptr(out2), B, H, L, int(conj), int(wrap), _lib.stream_ptr()),
               "ffc_conv_fwd_os_gated")
    return y, out2


def _dkf_os_gated(plan, dy, x, pregate, postgate):
    """ffc_conv_bwd_dkf_os_gated: the dk_f partial sums of the windows of x * pregate and dy * postgate -> (B * nblk, workspace)"""
    B, H, L = x.shape
    nb = B * (-(-L // (plan.seqlen // 2)))
    ws = torch.empty(_C._ws_bytes(plan, nb, H), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().ffc_conv_bwd_dkf_os_gated(plan.handle, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(pregate), _lib.ptr(postgate), _lib.ptr(ws),
                                                    B, H, L, _lib.stream_ptr()), "ffc_conv_bwd_dkf_os_gated")
    return nb, ws


class _OverlapSaveGatedFn(torch.autograd.Function):
    """y = postgate * conv(x * pregate, k) + residual block by block, every gate and the residual optional and inside the convolution
    launch.  Keeps x, the gates and k_f.  The backward runs, each only where its gradient is asked for: the input-gradient launch (window
    of dy * postgate, conj k_f; dx = g * pregate and dpregate = g * x from the same launch), the forward launch again with dy in the
    postgate slot (dpostgate), and the gated dk_f launch with the dk inverse.  residual receives dy."""

    @staticmethod
    def forward(ctx, x, k, pregate, postgate, residual, plan):
        with torch.cuda.device(x.device):
            kf = _C._kernel_fft(plan, k)
            y, _ = _conv_os_gated(plan, x, kf, False, True, pregate, postgate, residual)
        ctx.save_for_backward(x, kf, pregate, postgate)
        ctx.plan, ctx.k_shape, ctx.k_dtype = plan, tuple(k.shape), k.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, kf, pregate, postgate = ctx.saved_tensors
        plan, (H, Lk) = ctx.plan, ctx.k_shape
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        dx = dk = dpre = dpost = None
        with torch.cuda.device(x.device):
            want_dpre = need[2] and pregate is not None
            if need[0] or want_dpre:
                dx, dpre = _conv_os_gated(plan, dy, kf, True, False, postgate, pregate, None, x if want_dpre else None)
            if need[3] and postgate is not None:
                dpost, _ = _conv_os_gated(plan, x, kf, False, True, pregate, dy)
            if need[1]:
                nb, ws = _dkf_os_gated(plan, dy, x, pregate, postgate)
                dk = torch.empty(H, Lk, dtype=torch.float32, device=x.device)
                _lib.check(_lib.lib().ffc_kernel_ifft_grad(plan.handle, _lib.ptr(ws), nb, H, Lk, _lib.ptr(dk), _lib.stream_ptr()),
                           "ffc_kernel_ifft_grad")
                dk = dk.to(ctx.k_dtype)
        return dx if need[0] else None, dk, dpre, dpost, dy if need[4] else None, None


def _conv_os_hist(plan, x, kf, conj, wrap, pregate=None, postgate=None, addend=None, gate2=None, hist=None, want_dhist=False):
    """ffc_conv_fwd_os_hist: _conv_os_gated with the (B, H, S) history of block 0 (wrap) or, with want_dhist, a block -1 per row whose S
    outputs are the history's gradient -> (y, out2 or None, dhist or None)"""
    B, H, L = x.shape
    y = torch.empty_like(x)
    out2 = None if gate2 is None else torch.empty_like(x)
    dhist = torch.empty(B, H, plan.seqlen // 2, dtype=x.dtype, device=x.device) if want_dhist else None
    _lib.check(_lib.lib().ffc_conv_fwd_os_hist(plan.handle, _lib.ptr(x), _lib.ptr(kf), _lib.ptr(pregate), _lib.ptr(postgate), _lib.ptr(addend),
                                               _lib.ptr(y), _lib.ptr(gate2), _lib.ptr(out2), _lib.ptr(hist), _lib.ptr(dhist), B, H, L, int(conj),
                                               int(wrap), _lib.stream_ptr()), "ffc_conv_fwd_os_hist")
    return y, out2, dhist


def _dkf_os_hist(plan, dy, x, pregate, postgate, hist):
    """ffc_conv_bwd_dkf_os_hist: _dkf_os_gated with the history in block 0's window -> (B * nblk, workspace)"""
    B, H, L = x.shape
    nb = B * (-(-L // (plan.seqlen // 2)))
    ws = torch.empty(_C._ws_bytes(plan, nb, H), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().ffc_conv_bwd_dkf_os_hist(plan.handle, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(pregate), _lib.ptr(postgate), _lib.ptr(hist),
                                                   _lib.ptr(ws), B, H, L, _lib.stream_ptr()), "ffc_conv_bwd_dkf_os_hist")
    return nb, ws


class _OverlapSaveStateFn(torch.autograd.Function):
    """_OverlapSaveGatedFn for a call that starts in the middle of a signal: `state` (B, H, S) holds the S samples of x * pregate before
    the call's first one and is block 0's history in every launch that takes the wrapped window (forward, dpostgate, dk_f).  Its
    gradient is block -1 of the input-gradient launch, run only where it is asked for; that launch is skipped when neither x, pregate
    nor the state wants a gradient.  Where only the state wants one, the launch still computes and stores dx of the nblk blocks (the entry
    point has no form without y) and the result is dropped.  Gates stay optional: without any, the history kernels run with null gates."""

    @staticmethod
    def forward(ctx, x, k, pregate, postgate, residual, state, plan):
        with torch.cuda.device(x.device):
            kf = _C._kernel_fft(plan, k)
            y, _, _ = _conv_os_hist(plan, x, kf, False, True, pregate, postgate, residual, None, state)
        ctx.save_for_backward(x, kf, pregate, postgate, state)
        ctx.plan, ctx.k_shape, ctx.k_dtype = plan, tuple(k.shape), k.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, kf, pregate, postgate, state = ctx.saved_tensors
        plan, (H, Lk) = ctx.plan, ctx.k_shape
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        dx = dk = dpre = dpost = dstate = None
        with torch.cuda.device(x.device):
            want_dpre = need[2] and pregate is not None
            if need[0] or want_dpre or need[5]:
                dx, dpre, dstate = _conv_os_hist(plan, dy, kf, True, False, postgate, pregate, None, x if want_dpre else None, None, need[5])
            if need[3] and postgate is not None:
                dpost, _, _ = _conv_os_hist(plan, x, kf, False, True, pregate, dy, None, None, state)
            if need[1]:
                nb, ws = _dkf_os_hist(plan, dy, x, pregate, postgate, state)
                dk = torch.empty(H, Lk, dtype=torch.float32, device=x.device)
                _lib.check(_lib.lib().ffc_kernel_ifft_grad(plan.handle, _lib.ptr(ws), nb, H, Lk, _lib.ptr(dk), _lib.stream_ptr()),
                           "ffc_kernel_ifft_grad")
                dk = dk.to(ctx.k_dtype)
        return dx if need[0] else None, dk, dpre, dpost, dy if need[4] else None, dstate, None


STEP_MAX = 64      # overlap_save="direct": a stateful piece of up to this many samples runs the direct step kernels (ffc_partial_step_fwd)
_DT = {torch.bfloat16: 0, torch.float16: 1}


def _step_fwd(x, k, taps, S, pregate=None, postgate=None, residual=None, state=None, want_state=True, want_raw=False, new_state=None):
    """ffc_partial_step_fwd on a contiguous (B, H, L <= STEP_MAX) piece behind `state` (B, H, S; None: zeros), k (H, Lk) fp32: one launch
    -> (y, new_state or None, the fp32 sums before the postgate or None)"""
    B, H, L = x.shape
    y = torch.empty_like(x)
    if new_state is None and want_state:
        new_state = torch.empty(B, H, S, dtype=x.dtype, device=x.device)
    raw = torch.empty(B, H, L, dtype=torch.float32, device=x.device) if want_raw else None
    _lib.check(_lib.lib().ffc_partial_step_fwd(_DT[x.dtype], _lib.ptr(x), _lib.ptr(k), _lib.ptr(pregate), _lib.ptr(postgate), _lib.ptr(residual),
                                               _lib.ptr(state), _lib.ptr(y), _lib.ptr(new_state), _lib.ptr(raw), B, H, L, S, k.shape[-1], taps,
                                               _lib.stream_ptr()), "ffc_partial_step_fwd")
    return y, new_state, raw


def _step_bwd(dy, x, k, taps, S, pregate, postgate, state, raw, dnew, want_dx, want_dk, want_dpre, want_dpost, want_dstate):
    """ffc_partial_step_bwd: every gradient that is asked for from one launch -> (dx, dk partial sums (nsplit, H, taps) fp32, dpregate,
    dpostgate, dstate), None where not asked for"""
    B, H, L = x.shape
    dx = torch.empty_like(x) if want_dx else None
    dpre = torch.empty_like(x) if want_dpre else None
    dpost = torch.empty_like(x) if want_dpost else None
    dstate = torch.empty(B, H, S, dtype=x.dtype, device=x.device) if want_dstate else None
    nsplit = _lib.lib().ffc_partial_step_nsplit(B, H)
    dkp = torch.empty(nsplit, H, taps, dtype=torch.float32, device=x.device) if want_dk else None
    _lib.check(_lib.lib().ffc_partial_step_bwd(_DT[x.dtype], _lib.ptr(dy), _lib.ptr(x), _lib.ptr(k), _lib.ptr(pregate), _lib.ptr(postgate),
                                               _lib.ptr(state), _lib.ptr(raw), _lib.ptr(dnew), _lib.ptr(dx), _lib.ptr(dpre), _lib.ptr(dpost),
                                               _lib.ptr(dstate), _lib.ptr(dkp), nsplit, B, H, L, S, k.shape[-1], taps, _lib.stream_ptr()),
               "ffc_partial_step_bwd")
    return dx, dkp, dpre, dpost, dstate


class _DirectStepFn(torch.autograd.Function):
    """(y, new_state) of one direct step: a single launch each way.  Keeps x, k, the gates, the state and, where dpostgate will be asked
    for, the fp32 sums before the postgate (L values per row).  The backward takes the gradients of both outputs (the one that arrives
    on new_state is the shifted part of dstate and dx); the dk partial sums of a split batch are added in order by sum(0)."""

    @staticmethod
    def forward(ctx, x, k, pregate, postgate, residual, state, taps, S, want_state):
        kc = k if k.dtype == torch.float32 and k.is_contiguous() else k.float().contiguous()
        want_raw = postgate is not None and ctx.needs_input_grad[3]
        with torch.cuda.device(x.device):
            y, new_state, raw = _step_fwd(x, kc, taps, S, pregate, postgate, residual, state, want_state, want_raw)
        ctx.save_for_backward(x, kc, pregate, postgate, state, raw)
        ctx.taps, ctx.S, ctx.k_shape, ctx.k_dtype = taps, S, tuple(k.shape), k.dtype
        ctx.set_materialize_grads(False)
        return y, new_state

    @staticmethod
    def backward(ctx, dy, dnew):
        x, k, pregate, postgate, state, raw = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = torch.zeros_like(x) if dy is None else dy.contiguous()
        if dnew is not None:
            dnew = dnew.contiguous()
            if dnew.data_ptr() % 16:
                dnew = dnew.clone()
        want_dpre, want_dpost = need[2] and pregate is not None, need[3] and postgate is not None
        with torch.cuda.device(x.device):
            dx, dkp, dpre, dpost, dstate = _step_bwd(dy, x, k, ctx.taps, ctx.S, pregate, postgate, state, raw, dnew, need[0], need[1],
                                                     want_dpre, want_dpost, need[5] and state is not None)
        dk = None
        if need[1]:
            dk = dkp[0] if dkp.shape[0] == 1 else dkp.sum(0)
            if ctx.k_shape[1] > ctx.taps:
                dk = torch.nn.functional.pad(dk, (0, ctx.k_shape[1] - ctx.taps))
            dk = dk.to(ctx.k_dtype)
        return dx, dk, dpre, dpost, dy if need[4] else None, dstate, None, None, None


def _check_gate(x, name, g):
    if not torch.is_tensor(g):
        raise RuntimeError(f"PartialFFTConv: {name} must be a tensor")
    if g.device != x.device:
        raise RuntimeError(f"PartialFFTConv: {name} is on {g.device}, x on {x.device}")
    if g.shape != x.shape or g.dtype != x.dtype:
        raise RuntimeError(f"PartialFFTConv: {name} must match x in shape and dtype")


class PartialFFTConv(_ConvCache):
    """reference flashfftconv/sparse_conv.py:8-22

    overlap_save=True: a filter of P = min(N_partial, Lk) <= 16384 taps needs P - 1 samples of history, so every row is cut into blocks of
    S = os_fft_size(P) / 2 samples and each block runs on the one-launch fused kernel of fft size 2 S with the previous block as its
    history (ffc_conv_fwd_os): any sequence length, work per sample set by P and not by L, and nothing kept for the backward beyond x
    and k_f.  Rows that fit one block (L <= S) keep the 2 L route where 2 L is a supported fft size, as do filters of more than 16384
    taps.  Gates and `residual` are fused into the blocked launches as well (ffc_conv_fwd_os_gated, ffc_conv_bwd_dkf_os_gated): see forward.

    A row may be fed in pieces of any lengths: `state=` carries the last `state_len` = max(2048, nextpow2(N_partial)) samples of
    x * pregate from one call to the next (ffc_conv_fwd_os_hist, ffc_conv_bwd_dkf_os_hist), and the pieces give what one call on the whole
    row gives.  Such a call always takes the blocked route, whatever its length.

    overlap_save="direct": overlap_save=True in everything but one case.  A call with a state (state= or return_state=True) whose piece has
    at most STEP_MAX = 64 samples runs the direct step kernels instead (ffc_partial_step_fwd / _bwd: taps multiply-adds per sample on
    k in fp32, no transform of k, the new state written by the same launch).  The states of the two routes are the same tensors, so one
    module prefills a prompt on the blocked route and then generates sample by sample on the direct one.  The direct route refuses a
    state that is not 16-byte aligned where the blocked route copies it."""

    def __init__(self, N_partial, overlap_save=False):
        super().__init__(N_partial)
        self.overlap_save = overlap_save
        # S: length of the carried state, the block length of the route for filters of N_partial taps (None: no overlap-save route)
        self.state_len = os_fft_size(N_partial) // 2 if overlap_save and 1 <= N_partial <= OS_MAX_TAPS else None

    def _os_plan(self, x, k, stateful=False, want_plan=True):
        """the block plan of the overlap-save route for this call, or None: today's 2 L route.  stateful: a call that takes or returns a
        state runs blocks of state_len samples whatever L and k's length are, or raises.  want_plan=False: the checks alone (a direct
        step needs no plan) -> True"""
        if stateful:
            if self.state_len is None:
                raise RuntimeError("PartialFFTConv: state= / return_state= need overlap_save=True and N_partial <= 16384")
            if not torch.is_tensor(x) or not torch.is_tensor(k) or x.dim() != 3 or k.dim() != 2 or x.shape[-1] < 1 or k.shape[-1] < 1:
                raise RuntimeError("PartialFFTConv: state= / return_state= need x of shape (B, H, L >= 1) and k of shape (H, Lk >= 1)")
            if x.dtype not in (torch.bfloat16, torch.float16):
                raise RuntimeError(f"PartialFFTConv: x must be a bf16 / fp16 tensor, got {x.dtype}")
        if not self.overlap_save or not torch.is_tensor(x) or not torch.is_tensor(k) or x.dim() != 3 or k.dim() != 2:
            return None
        L, taps = x.shape[-1], min(self.N_partial, k.shape[-1])
        if x.dtype not in (torch.bfloat16, torch.float16) or L < 1 or not 1 <= taps <= OS_MAX_TAPS:
            return None
        n = 2 * self.state_len if stateful else os_fft_size(taps)
        if not stateful and L <= n // 2 and 2 * L in _C.SUPPORTED_SEQLENS:
            return None
        if x.numel() >= 2 ** 31 or L + n >= 2 ** 31:      # (the kernels index a row in 32 bits up to one window past its end)
            raise RuntimeError("PartialFFTConv: B * H * L and L + the block fft size must be below 2^31")
        if not x.is_cuda:
            raise RuntimeError("PartialFFTConv: x must be a CUDA/HIP tensor (no CPU fallback in the product path)")
        if k.device != x.device:
            raise RuntimeError(f"PartialFFTConv: k is on {k.device}, x on {x.device}")
        if k.shape[0] != x.shape[1]:
            raise RuntimeError(f"PartialFFTConv: k has {k.shape[0]} rows, x {x.shape[1]} heads")
        return _C.get_plan(n, x.dtype, x.device) if want_plan else True

    def _check_state(self, x, state):
        if not torch.is_tensor(state):
            raise RuntimeError("PartialFFTConv: state must be a tensor")
        if state.device != x.device:
            raise RuntimeError(f"PartialFFTConv: state is on {state.device}, x on {x.device}")
        if tuple(state.shape) != (x.shape[0], x.shape[1], self.state_len) or state.dtype != x.dtype:
            raise RuntimeError(f"PartialFFTConv: state must be {(x.shape[0], x.shape[1], self.state_len)} {x.dtype}, got {tuple(state.shape)} {state.dtype}")
        if not state.is_contiguous():
            raise RuntimeError("PartialFFTConv: state must be contiguous")

    def forward(self, x, k, pregate=None, postgate=None, residual=None, state=None, return_state=False):
        """y = postgate * conv(x * pregate, k[..., :N_partial]) + residual; each of pregate, postgate, residual (x's shape, dtype and device)
        is optional on its own.  Differentiable in x, k and the gates; residual receives the incoming gradient.  On the blocked route a
        call with a gate or a residual keeps x, the gates and k_f for the backward (no spectra, no output before the gate) and recomputes
        the forward once where dpostgate is asked for; a call with neither keeps x and k_f.

        state (B, H, state_len), x's dtype and device, contiguous; None: zeros): the samples of x * pregate that precede this call's,
        oldest first, already gated.  return_state=True returns (y, new_state) with new_state = cat(state, x * pregate)[..., -state_len:],
        the product rounded once to the module dtype as the kernel rounds it.  Differentiable in the state as well."""
        if state is not None or return_state:
            return self._forward_state(x, k, pregate, postgate, residual, state, return_state)
        plan = self._os_plan(x, k)
        if plan is None:
            if (pregate is None) != (postgate is None):      # FlashFFTConv takes both gates or none: the missing one is all ones
                ones = torch.ones_like(pregate if postgate is None else postgate)
                pregate, postgate = (ones if pregate is None else pregate), (ones if postgate is None else postgate)
            return self._conv_for(x)(x, k[..., : self.N_partial], pregate, postgate, residual=residual)
        if pregate is None and postgate is None and residual is None:
            return _OverlapSaveFn.apply(x.contiguous(), k[..., : self.N_partial], plan)
        for name, g in (("pregate", pregate), ("postgate", postgate)):
            if g is not None:
                _check_gate(x, name, g)
        if residual is not None:
            _C._check_residual(x, residual)
        pregate, postgate, residual = (None if t is None else t.contiguous() for t in (pregate, postgate, residual))
        return _OverlapSaveGatedFn.apply(x.contiguous(), k[..., : self.N_partial], pregate, postgate, residual, plan)

    def _forward_state(self, x, k, pregate, postgate, residual, state, return_state):
        direct = self.overlap_save == "direct" and torch.is_tensor(x) and x.dim() == 3 and x.shape[-1] <= STEP_MAX
        plan = self._os_plan(x, k, stateful=True, want_plan=not direct)
        for name, g in (("pregate", pregate), ("postgate", postgate)):
            if g is not None:
                _check_gate(x, name, g)
        if residual is not None:
            _C._check_residual(x, residual)
        if state is not None:
            self._check_state(x, state)
            if state.data_ptr() % 16 and not direct:      # (the kernels read the history 16 bytes at a time; the step entry point refuses)
                state = state.clone()
        x = x.contiguous()
        pregate, postgate, residual = (None if t is None else t.contiguous() for t in (pregate, postgate, residual))
        if direct:
            # one launch: y, the new state and (for dpostgate) the sums before the gate; states are those of the blocked route
            y, new_state = _DirectStepFn.apply(x, k, pregate, postgate, residual, state, min(self.N_partial, k.shape[-1]), self.state_len,
                                               return_state)
            return (y, new_state) if return_state else y
        if state is None and pregate is None and postgate is None and residual is None:
            y = _OverlapSaveFn.apply(x, k[..., : self.N_partial], plan)
        elif state is None:
            y = _OverlapSaveGatedFn.apply(x, k[..., : self.N_partial], pregate, postgate, residual, plan)
        else:
            y = _OverlapSaveStateFn.apply(x, k[..., : self.N_partial], pregate, postgate, residual, state, plan)
        if not return_state:
            return y
        # The new state is composed in torch from the tails: at most S samples per row are touched, against the L the kernels move, and
        # as plain torch ops their gradients reach x, pregate and the old state through autograd with no code of ours.
        S, L = self.state_len, x.shape[-1]
        tail = x[..., -S:] if pregate is None else x[..., -S:] * pregate[..., -S:]
        if L < S:
            old = state[..., L:] if state is not None else x.new_zeros(x.shape[0], x.shape[1], S - L)
            tail = torch.cat((old, tail), dim=-1)
        return y, tail.contiguous()


class FrequencySparseFFTConv(_ConvCache):
    """reference flashfftconv/sparse_conv.py:24-38: rfft bins >= N_partial // 2 of k are zeroed."""

    def forward(self, x, k, residual=None):
        # (residual: FlashFFTConv.forward; on the compute-skipping kernel, fft 16384 / 32768 with N_partial <= fft / 4, it is added by composition)
        return self._conv_for(x, keep=self.N_partial // 2)(x, k, residual=residual)
