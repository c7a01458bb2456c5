"""Which C-ABI calls the host path makes, and what they compute: a fixed, seeded matrix of small forward + backward calls through every
branch of the fused host path (flashfftconv/fused.py and its three callers).  Per case: the sequence of library calls -- entry name,
integer and float arguments verbatim, every pointer as null / ptr -- and the sha256 of every output and gradient.  Two versions of the
Python package on ONE built library must print the same text:

    FFC_LIB=.../libflashfftconv_hip.so python benchmarks/call_trace.py --pkg DIR_A > a.txt
    FFC_LIB=.../libflashfftconv_hip.so python benchmarks/call_trace.py --pkg DIR_B > b.txt ; diff a.txt b.txt

--pkg: the directory that holds the `flashfftconv` package to import (default: this tree's).  ffc_dkf_workspace_bytes is not listed: it is a
size query that launches nothing, and how often it is repeated (conv._ws_bytes remembers the answer) is not behaviour.
The shapes are the smallest at which each kernel family and each branch is reached: B = 3 (an odd last pair), H = 2 (D = 8 for the
operator), L = N / 2 unless stated; every spectrum request is below conv._SPEC_SMALL, so the memory budget cannot make two runs differ."""
import argparse, ctypes, hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "flash-fft-conv_amd"))
ap.add_argument("--folded-child", action="store_true", help="(internal) the fft-2048 cases on the folded plan, FFC_MULTIPASS without 2048")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
import torch
import flashfftconv
from flashfftconv import FlashFFTConv, FrequencySparseFFTConv, gated_conv_from_slices, _lib, conv as C, sharding

assert os.path.dirname(os.path.dirname(os.path.abspath(flashfftconv.__file__))) == os.path.abspath(args.pkg), flashfftconv.__file__
BF, HF = torch.bfloat16, torch.float16
B, H, D = 3, 2, 8
CALLS = []


def _show(a):
    if a is None:
        return "null"
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, ctypes.c_float):
        return repr(a.value)
    if isinstance(a, (bool, int, float)):
        return repr(a)
    return type(a).__name__      # (byref of a plan handle)


class _Recorder:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in ("ffc_dkf_workspace_bytes", "ffc_last_error"):
            return fn

        def call(*a):
            CALLS.append(f"  {name}({', '.join(_show(x) for x in a)})")
            return fn(*a)
        return call


_proxy = _Recorder(_lib.lib())
_lib.lib = lambda: _proxy


def sha(t):
    return "none" if t is None else hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def case(name, fn):
    """fn() -> dict of named result tensors; inputs are drawn from a generator seeded by the case's name"""
    torch.manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    del CALLS[:]
    out = fn()
    torch.cuda.synchronize()
    print(f"case {name}")
    print("\n".join(CALLS))
    for k, v in out.items():
        print(f"  = {k} {sha(v)}")
    sys.stdout.flush()


def rnd(*shape, dt=torch.float32, grad=True, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(dt).requires_grad_(grad)


def run_module(mod, L, Lk, dt, gated, mode="train", residual=False, k_rev=False, twice=False):
    def fn():
        u, k = rnd(B, H, L, dt=dt), rnd(H, Lk, scale=0.1)
        gates = [rnd(B, H, L, dt=dt) for _ in range(2)] if gated else []
        res = rnd(B, H, L, dt=dt) if residual else None
        kr = rnd(H, 5, scale=0.1) if k_rev else None
        dout = rnd(B, H, L, dt=dt, grad=False)
        mod.train(mode != "eval")
        kw = {k_: v for k_, v in (("residual", res), ("k_rev", kr)) if v is not None}
        if mode in ("eval", "no_grad"):
            with torch.no_grad():
                outs = {"y": mod(u, k, *gates, **kw)}
                if twice:
                    outs["y2"] = mod(u, k, *gates, **kw)
            return outs
        y = mod(u, k, *gates, **kw)
        y.backward(dout)
        outs = {"y": y, "du": u.grad, "dk": k.grad}
        for nm, t in zip(("dpre", "dpost"), gates):
            outs[nm] = t.grad
        if res is not None:
            outs["dres"] = res.grad
        if kr is not None:
            outs["dk_rev"] = kr.grad
        return outs
    return fn


def module_cases(sizes):
    for N in sizes:
        for gated in (False, True):
            g = "gated" if gated else "plain"
            for mode, save in (("train", True), ("train", False), ("eval", True), ("no_grad", True)):
                mod = FlashFFTConv(N, dtype=BF).cuda()
                mod.save_spectrum = save
                case(f"module fft{N} {g} {mode} save_spectrum={save}", run_module(mod, N // 2, N // 2, BF, gated, mode))


def hyena_cases():
    for N in (1024, 4096):
        for save in (True, False):
            for filt in ("k", "k+k_res", "k+k_res+rev"):
                def fn(N=N, save=save, filt=filt, Dd=D, L=N // 2):
                    mod = FlashFFTConv(N, dtype=BF).cuda()
                    mod.save_spectrum = save
                    uc = rnd(B, 3 * Dd, L, dt=BF)
                    ks = {"k": rnd(Dd, L, scale=0.1)}
                    if filt != "k":
                        ks["k_res"] = rnd(Dd, L, scale=0.1)
                    if filt == "k+k_res+rev":
                        ks["k_rev"], ks["k_res_rev"] = rnd(Dd, 5, scale=0.1), rnd(Dd, 5, scale=0.1)
                    y = gated_conv_from_slices(mod, uc, ks["k"], ks.get("k_res"), ks.get("k_rev"), ks.get("k_res_rev"))
                    y.backward(rnd(B, Dd, L, dt=BF, grad=False))
                    return {"y": y, "duc": uc.grad, **{"d" + nm: t.grad for nm, t in ks.items()}}
                case(f"slices fft{N} save_spectrum={save} {filt}", fn)

    def copies():      # (D * L) % 8 != 0: the composition on contiguous copies
        mod = FlashFFTConv(1024, dtype=BF).cuda()
        uc, k = rnd(B, 9, 511, dt=BF), rnd(3, 511, scale=0.1)
        y = gated_conv_from_slices(mod, uc, k)
        y.backward(rnd(B, 3, 511, dt=BF, grad=False))
        return {"y": y, "duc": uc.grad, "dk": k.grad}
    case("slices fft1024 D*L % 8 != 0", copies)


def shard_cases():
    N, L = 4096, 2048
    for gated in (False, True):
        for keep in (True, False):
            def fn(gated=gated, keep=keep):
                mod = FlashFFTConv(N, dtype=BF).cuda()
                ops = sharding._HipOps(mod, torch.device("cuda", 0))
                u, k, dout = rnd(B, H, L, dt=BF, grad=False), rnd(H, L, scale=0.1, grad=False), rnd(B, H, L, dt=BF, grad=False)
                pre, post = (rnd(B, H, L, dt=BF, grad=False), rnd(B, H, L, dt=BF, grad=False)) if gated else (None, None)
                kf = ops.kernel_fft(k)
                out, du = torch.zeros_like(u), torch.zeros_like(u)
                dpre, dpost = (torch.zeros_like(u), torch.zeros_like(u)) if gated else (None, None)
                outs = {}
                for g0, g1 in ((0, 1), (1, 2)):
                    kept = ops.conv_slice(u, kf[g0:g1], pre, post, out, g0, g1, keep)
                    dkf = ops.backward_slice(dout, u, kf[g0:g1], pre, post, du, dpre, dpost, g0, g1, kept)
                    outs[f"dkf{g0}"], outs[f"dk{g0}"] = dkf, ops.dk_from_dkf(dkf, L)
                outs.update(y=out, du=du, dpre=dpre, dpost=dpost)
                return outs
            case(f"bshard ops fft{N} {'gated' if gated else 'plain'} keep={keep}", fn)


if args.folded_child:
    assert 2048 not in C.MULTIPASS_SEQLENS and FlashFFTConv(2048)._folded
    for gated in (False, True):
        mod = FlashFFTConv(2048, dtype=BF).cuda()
        case(f"module fft2048 folded {'gated' if gated else 'plain'} train", run_module(mod, 1024, 1024, BF, gated))
    sys.exit(0)

with torch.cuda.device(0):
    module_cases((256, 1024, 2048, 4096, 32768, 65536))
    for N in (1024, 4096):
        for gated in (False, True):
            g = "gated" if gated else "plain"
            case(f"module fft{N} {g} fp16", run_module(FlashFFTConv(N, dtype=HF).cuda(), N // 2, N // 2, HF, gated))
            case(f"module fft{N} {g} residual", run_module(FlashFFTConv(N, dtype=BF).cuda(), N // 2, N // 2, BF, gated, residual=True))
    for N in (1024, 4096, 65536):
        for gated in (False, True):
            case(f"module fft{N} {'gated' if gated else 'plain'} k_rev", run_module(FlashFFTConv(N, dtype=BF).cuda(), N // 2, N // 2, BF, gated, k_rev=True))
    cached = FlashFFTConv(4096, dtype=BF).cuda()
    cached.cache_kf = True

    def cached_twice():
        u, k = rnd(B, H, 2048, dt=BF, grad=False), rnd(H, 2048, scale=0.1, grad=False)
        cached.eval()
        with torch.no_grad():
            return {"y": cached(u, k), "y2": cached(u, k)}
    case("module fft4096 cache_kf twice eval", cached_twice)
    for gated in (False, True):
        case(f"module fft4096 {'gated' if gated else 'plain'} L=N-3", run_module(FlashFFTConv(4096, dtype=BF).cuda(), 4093, 4093, BF, gated))
    # frequency-sparse at fft 16384: keep = N_partial // 2 bins, ceil(keep / 512) rows per side; 1024 -> rows 2, 4096 -> too wide for the row kernel
    for n_partial in (2048, 8192):
        for gated in (False, True):
            def fn(n_partial=n_partial, gated=gated):
                fs = FrequencySparseFFTConv(n_partial).cuda()
                x = rnd(B, H, 8192, dt=BF)
                return run_module(fs._conv_for(x, keep=n_partial // 2), 8192, 8192, BF, gated)()
            case(f"sparse fft16384 N_partial={n_partial} {'gated' if gated else 'plain'}", fn)
    hyena_cases()
    shard_cases()
    # fft 2048 on the folded plan: FFC_MULTIPASS is read at import, so a fresh child process
    sys.stdout.flush()
    env = dict(os.environ, FFC_MULTIPASS="65536,131072")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", args.pkg, "--folded-child"], env=env, check=True, timeout=300)
