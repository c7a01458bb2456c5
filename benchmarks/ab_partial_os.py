"""PartialFFTConv(P) with and without overlap_save, one process, alternating windows: forward, forward + backward and peak memory.

    python benchmarks/ab_partial_os.py [OUT.txt] [--quick]      the table of profiles/partial_os_ab.txt

bf16, B = 2, H = 768, L in 16384 .. 1048576, P in 2048, 8192.  Baseline: the same module without the flag (fft size 2 L) in the same run.
Each window is sized to about a quarter of a second of device time; --quick: two lengths, three windows."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-fft-conv_amd"))
import torch
from flashfftconv import PartialFFTConv

B, H = 2, 768


def window(mod, x, k, dout, steps, bwd):
    """ms per step, device events around `steps` steps"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        if bwd:
            x.grad = k.grad = None
            mod(x, k).backward(dout)
        else:
            with torch.no_grad():
                mod(x, k)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def peak_mb(mod, x, k, dout):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    x.grad = k.grad = None
    mod(x, k).backward(dout)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def table(path, quick):
    out = open(path, "w") if path else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    win = 3 if quick else 7
    say(f"PartialFFTConv(P): fft 2L route / overlap_save route, B={B} H={H} bf16, {win} alternating windows; ms per call: median [min .. max]")
    for L in ((16384, 262144) if quick else (16384, 65536, 262144, 1048576)):
        x = torch.randn(B, H, L, device="cuda").to(torch.bfloat16).requires_grad_(True)
        dout = torch.randn(B, H, L, device="cuda").to(torch.bfloat16)
        for P in (2048, 8192):
            k = (torch.randn(H, P, device="cuda") * 0.1).requires_grad_(True)
            mods = {"2L": PartialFFTConv(P).to("cuda"), "os": PartialFFTConv(P, overlap_save=True).to("cuda")}
            try:
                window(mods["2L"], x, k, dout, 1, False)
            except (RuntimeError, NotImplementedError) as e:      # a shape the 2 L route does not serve: the blocked route alone
                say(f"L {L:8d} P {P:5d} 2L route fails: {str(e)[:110]}")
                m = mods["os"]
                for bwd in (False, True):
                    window(m, x, k, dout, 2, bwd)
                    t = [window(m, x, k, dout, max(3, int(250.0 / window(m, x, k, dout, 3, bwd))), bwd) for _ in range(win)]
                    say(f"L {L:8d} P {P:5d} {'fwd+bwd' if bwd else 'fwd    '}: os {statistics.median(t):9.4f} [{min(t):.4f} .. {max(t):.4f}]")
                say(f"L {L:8d} P {P:5d} peak MB of fwd+bwd above the inputs: os {peak_mb(m, x, k, dout):.0f}")
                continue
            for bwd in (False, True):
                t, steps = {"2L": [], "os": []}, {}
                for nm, m in mods.items():      # warm-up, and the window length from a first timing
                    window(m, x, k, dout, 2, bwd)
                    steps[nm] = max(3, min(200, int(250.0 / window(m, x, k, dout, 3, bwd))))
                for _ in range(win):
                    for nm, m in mods.items():
                        t[nm].append(window(m, x, k, dout, steps[nm], bwd))
                m0, m1 = statistics.median(t["2L"]), statistics.median(t["os"])
                say(f"L {L:8d} P {P:5d} {'fwd+bwd' if bwd else 'fwd    '}: 2L {m0:9.4f} [{min(t['2L']):.4f} .. {max(t['2L']):.4f}]   "
                    f"os {m1:9.4f} [{min(t['os']):.4f} .. {max(t['os']):.4f}]   os / 2L {m1 / m0:.3f}")
            say(f"L {L:8d} P {P:5d} peak MB of fwd+bwd above the inputs: 2L {peak_mb(mods['2L'], x, k, dout):.0f}   os {peak_mb(mods['os'], x, k, dout):.0f}")
            del mods
            torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--quick"]
    table(args[0] if args else None, "--quick" in sys.argv)
