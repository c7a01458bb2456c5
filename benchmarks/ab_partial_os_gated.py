"""PartialFFTConv(P, overlap_save=True) with gates and a residual: the fused call against the composition in torch, one process, alternating
windows: forward, forward + backward and peak memory.

    python benchmarks/ab_partial_os_gated.py [OUT.txt] [--quick]      the table of profiles/partial_os_gated_ab.txt

y = postgate * conv(x * pregate, k[:, :P]) + residual, bf16, B = 2, H = 768, L in 16384, 65536, 262144, P in 2048, 8192.
  fused      mod(x, k, pregate, postgate, residual): gates and residual inside the blocked launches
  composed   mod(x * pregate, k) * postgate + residual: the ungated blocked launches with torch's elementwise kernels and autograd around
             them (what the module could do before it took gates)
Gradients of x, k and both gates in either form.  Each window is sized to about a quarter of a second of device time; --quick: two
lengths, three windows."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-fft-conv_amd"))
import torch
from flashfftconv import PartialFFTConv

B, H = 2, 768
FORMS = {"fused": lambda mod, x, k, pre, post, res: mod(x, k, pre, post, res),
         "composed": lambda mod, x, k, pre, post, res: mod(x * pre, k) * post + res}


def window(form, mod, t, dout, steps, bwd):
    """ms per step, device events around `steps` steps"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        if bwd:
            for v in t:
                v.grad = None
            form(mod, *t).backward(dout)
        else:
            with torch.no_grad():
                form(mod, *t)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def peak_mb(form, mod, t, dout):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for v in t:
        v.grad = None
    form(mod, *t).backward(dout)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def table(path, quick):
    out = open(path, "w") if path else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    win = 3 if quick else 7
    say(f"PartialFFTConv(P, overlap_save=True), gates + residual: composed in torch / fused, B={B} H={H} bf16, {win} alternating windows; "
        "ms per call: median [min .. max]")
    for L in ((16384, 262144) if quick else (16384, 65536, 262144)):
        x, pre, post = (torch.randn(B, H, L, device="cuda").to(torch.bfloat16).requires_grad_(True) for _ in range(3))
        res, dout = (torch.randn(B, H, L, device="cuda").to(torch.bfloat16) for _ in range(2))
        for P in (2048, 8192):
            k = (torch.randn(H, P, device="cuda") * 0.1).requires_grad_(True)
            t = (x, k, pre, post, res)
            mod = PartialFFTConv(P, overlap_save=True).to("cuda")
            for bwd in (False, True):
                ms, steps = {nm: [] for nm in FORMS}, {}
                for nm, f in FORMS.items():      # warm-up, and the window length from a first timing
                    window(f, mod, t, dout, 2, bwd)
                    steps[nm] = max(3, min(200, int(250.0 / window(f, mod, t, dout, 3, bwd))))
                for _ in range(win):
                    for nm, f in FORMS.items():
                        ms[nm].append(window(f, mod, t, dout, steps[nm], bwd))
                m0, m1 = statistics.median(ms["composed"]), statistics.median(ms["fused"])
                say(f"L {L:8d} P {P:5d} {'fwd+bwd' if bwd else 'fwd    '}: composed {m0:9.4f} [{min(ms['composed']):.4f} .. {max(ms['composed']):.4f}]   "
                    f"fused {m1:9.4f} [{min(ms['fused']):.4f} .. {max(ms['fused']):.4f}]   fused / composed {m1 / m0:.3f}")
            say(f"L {L:8d} P {P:5d} peak MB of fwd+bwd above the inputs: composed {peak_mb(FORMS['composed'], mod, t, dout):.0f}   "
                f"fused {peak_mb(FORMS['fused'], mod, t, dout):.0f}")
            del mod
            torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--quick"]
    table(args[0] if args else None, "--quick" in sys.argv)
