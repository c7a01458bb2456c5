"""Frequency-sparse backward on the live rows against the dense backward of the same module (FFC_SPARSE_BWD=1 / =0), one process, alternating windows.

    python benchmarks/ab_sparse_bwd.py [OUT.txt]          the table of profiles/sparse_bwd_ab.txt (fwd + bwd and the backward's device interval)
    python benchmarks/ab_sparse_bwd.py --trace FLAG L     10 fwd + bwd steps at sequence length L with FFC_SPARSE_BWD=FLAG, keep = N / 8, and nothing
                                                          else: the program to put behind `rocprofv3 --kernel-trace --stats ... --`
B = 16, H = 768, bf16; L = 16384 (fft 32768) and 8192 (fft 16384); keep = N / 32 and N / 8."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-fft-conv_amd"))
import torch
from flashfftconv import FrequencySparseFFTConv, FlashFFTConv, conv as C

B, H, WIN, IT = 16, 768, 7, 20


def inputs(L):
    x = torch.randn(B, H, L, device="cuda").to(torch.bfloat16).requires_grad_(True)
    k = (torch.randn(H, L, device="cuda") * 0.1).requires_grad_(True)
    return x, k, torch.randn(B, H, L, device="cuda").to(torch.bfloat16)


def window(mod, x, k, dout, only_bwd=False, steps=IT):
    """ms per step over `steps` steps: device events around the window, or around each y.backward and summed"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tot = 0.0
    if not only_bwd:
        e0.record()
    for _ in range(steps):
        x.grad = k.grad = None
        y = mod(x, k)
        if only_bwd:
            e0.record()
        y.backward(dout)
        if only_bwd:
            e1.record(); torch.cuda.synchronize(); tot += e0.elapsed_time(e1)
    if not only_bwd:
        e1.record(); torch.cuda.synchronize(); tot = e0.elapsed_time(e1)
    return tot / steps


def setflag(v):
    os.environ["FFC_SPARSE_BWD"] = v
    C.reload_env()


def table(path):
    out = open(path, "w") if path else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    say(f"B={B} H={H} bf16, {WIN} alternating windows of {IT} steps each; ms per step: median [min .. max]")
    for L in (16384, 8192):
        N = 2 * L
        x, k, dout = inputs(L)
        dense = FlashFFTConv(N, dtype=torch.bfloat16).to("cuda")
        for _ in range(3):
            window(dense, x, k, dout)
        d = [window(dense, x, k, dout) for _ in range(WIN)]
        say(f"fft {N} dense module (FlashFFTConv, its own default path) fwd+bwd: {statistics.median(d):.4f} [{min(d):.4f} .. {max(d):.4f}]")
        for keep in (N // 32, N // 8):
            mod = FrequencySparseFFTConv(2 * keep).to("cuda")
            for only_bwd in (False, True):
                t = {"0": [], "1": []}
                for f in ("0", "1"):
                    setflag(f); window(mod, x, k, dout, only_bwd)
                for _ in range(WIN):
                    for f in ("0", "1"):
                        setflag(f); t[f].append(window(mod, x, k, dout, only_bwd))
                m0, m1 = statistics.median(t["0"]), statistics.median(t["1"])
                say(f"fft {N} keep {keep} (rows {-(-keep // (N // 32))}) {'bwd only' if only_bwd else 'fwd+bwd '}: dense bwd {m0:.4f} [{min(t['0']):.4f} .. {max(t['0']):.4f}]"
                    f"   sparse bwd {m1:.4f} [{min(t['1']):.4f} .. {max(t['1']):.4f}]   ratio {m1 / m0:.3f}")
    setflag("1")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        L = int(sys.argv[3])
        setflag(sys.argv[2])
        window(FrequencySparseFFTConv(L // 2).to("cuda"), *inputs(L), steps=10)      # N_partial = N / 4: keep = N / 8
    else:
        table(sys.argv[1] if len(sys.argv) > 1 else None)
