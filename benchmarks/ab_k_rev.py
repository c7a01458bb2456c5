"""A/B of the bidirectional-filter arguments on a training step of the M2 sequence mixer (FlashHyenaMixer with k_res, both filters bidirectional).

    (a) composed   the filters built in torch every step, as the reference mixer does
                   (examples/bert/monarch_mixer_sequence_mixer_flashfftconv.py:141-170): k = pad(k_fwd, (0, L)) + pad(flip(k_rev), (L, 0)),
                   handed to the operator as one 2L-tap row each; autograd runs the mirror image in the backward.  This is the code path of
                   the package without k_rev: the baseline.
    (b) k_rev      k_rev / k_res_rev passed through: the k -> k_f kernel reads both tensors, the dk_f -> dk kernel writes both gradients.

Shapes of benchmarks/m2_bert_fwd.py: d_model 768, L = 128, 512, 2048, 8192, fft = 2 L.  One process; the two sides alternate window by window in
the same loop (a, b, a, b, ...), each window at least 0.5 s of steps between two device events after a warm-up; every window's ms per step is
printed, so the spread of each side is on the page.  Kernel launches per step are counted with torch.profiler.  The time is reported, not gated.
usage: python benchmarks/ab_k_rev.py [L ...]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "flash-fft-conv_amd"), ROOT]
import torch
import torch.nn as nn
import torch.nn.functional as F
from flashfftconv import FlashHyenaMixer

D = 768
BATCH = {128: 32, 512: 16, 2048: 8, 8192: 4}      # m2_bert_fwd.py's batches (512: between its neighbours)
WINDOWS, WINDOW_S = 5, 0.5


def build(L, dtype):
    torch.manual_seed(0)
    inp, outp = nn.Linear(D, 3 * D).cuda().to(dtype), nn.Linear(D, D).cuda().to(dtype)
    w, b = torch.randn(3 * D, 1, 3, device="cuda") * 0.5, torch.randn(3 * D, device="cuda") * 0.1
    mixer = FlashHyenaMixer(D, 2 * L, inp, outp, w, b, dtype=dtype, device="cuda").cuda()
    t = torch.linspace(0, 1, L, device="cuda")[None]
    decay = torch.exp(-t * torch.linspace(2.0, 12.0, D, device="cuda")[:, None])
    filt = [nn.Parameter(torch.randn(D, L, device="cuda") * 0.02 * decay) for _ in range(4)]      # k, k_rev, k_res, k_res_rev
    return mixer, filt


def steps(mixer, filt, u, dout, L):
    k, kr, k2, k2r = filt
    params = list(mixer.parameters()) + filt

    def zero():
        for p in params:
            p.grad = None

    def composed():
        zero()
        kf = F.pad(k, (0, L)) + F.pad(kr.flip(-1), (L, 0))
        kf2 = F.pad(k2, (0, L)) + F.pad(k2r.flip(-1), (L, 0))
        mixer(u, kf, kf2).backward(dout)

    def fused():
        zero()
        mixer(u, k, k2, k_rev=kr, k_res_rev=k2r).backward(dout)

    return composed, fused


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn(); torch.cuda.synchronize()
    return sum(1 for e in p.events() if not e.name.startswith(("Memcpy", "Memset", "hip", "cuda")))


def run(L, dtype=torch.bfloat16):
    B = BATCH.get(L, 4)
    mixer, filt = build(L, dtype)
    g = torch.Generator(device="cuda").manual_seed(L)
    u = torch.randn(B, L, D, device="cuda", generator=g).to(dtype)
    dout = torch.randn(B, L, D, device="cuda", generator=g).to(dtype)
    sides = dict(zip(("composed", "k_rev"), steps(mixer, filt, u, dout, L)))
    for fn in sides.values():          # warm-up: plans, allocator, clocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    iters = {nm: max(10, int(WINDOW_S * 1e3 / window(fn, 20)) + 1) for nm, fn in sides.items()}
    ms = {nm: [] for nm in sides}
    for _ in range(WINDOWS):
        for nm, fn in sides.items():
            ms[nm].append(window(fn, iters[nm]))
    n = {nm: launches(fn) for nm, fn in sides.items()}
    print(f"L={L} fft={2 * L} B={B} D={D} bf16, fwd+bwd step, {WINDOWS} alternating windows of >= {WINDOW_S} s")
    for nm in sides:
        v = sorted(ms[nm])
        print(f"  {nm:9s} ms/step median {v[len(v) // 2]:.4f}  min {v[0]:.4f}  max {v[-1]:.4f}  windows {' '.join(f'{x:.4f}' for x in ms[nm])}"
              f"  ({iters[nm]} steps each)  kernels/step {n[nm]}")
    a, b = sorted(ms["composed"]), sorted(ms["k_rev"])
    verdict = "k_rev faster outside the spread" if b[-1] < a[0] else ("k_rev slower outside the spread" if b[0] > a[-1] else "inside the spread")
    print(f"  median ratio k_rev / composed {b[len(b) // 2] / a[len(a) // 2]:.3f}: {verdict}", flush=True)


if __name__ == "__main__":
    for L in ([int(x) for x in sys.argv[1:]] or [128, 512, 2048, 8192]):
        run(L)
