"""PartialFFTConv(P, overlap_save="direct") against overlap_save=True on stateful pieces of L samples (generation), one process, alternating
windows: forward under no_grad and forward + backward, the same inputs and the same state for both.

    python benchmarks/ab_partial_os_step.py [OUT.txt] [--quick]      the table of profiles/partial_os_step_ab.txt

y_i, s = mod(x_i, k, state=s, return_state=True), bf16, B = 2, H = 768, L in 1, 16, 64, P in 2048, 8192 (S = P).  Forward + backward is
truncated at the piece: the state comes in detached and x, k want gradients.  Times are device events around a window of steps, so a
step includes its host time wherever the host is slower than the device (a step is launch-bound there: the line says how many
microseconds a step took; a launch with its allocations costs the host some tens of them).  The forward's bytes are what the step has to
move: state read and written, k once per head, x and y; they are set against the device's streaming-copy rate (ffc_debug_peaks).  The
L = 64 lines are the STEP_MAX crossover: the longest piece of the direct route against the blocked route on the same piece.  Outputs of
the two routes are compared once per case (largest difference over the largest |y|)."""
import ctypes, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-fft-conv_amd"))
import torch
from flashfftconv import PartialFFTConv, _lib

B, H = 2, 768


def step(mod, x, k, s, dout, bwd):
    y, ns = mod(x, k, state=s, return_state=True)
    if bwd:
        y.backward(dout)
    return y, ns


def window(mod, x, k, s, dout, steps, bwd):
    """microseconds per step, device events around `steps` steps"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        if bwd:
            x.grad = k.grad = None
            step(mod, x, k, s, dout, True)
        else:
            with torch.no_grad():
                step(mod, x, k, s, dout, False)
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / steps


def table(path, quick):
    out = open(path, "w") if path else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    win = 3 if quick else 7
    copy, mfma = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().ffc_debug_peaks(ctypes.byref(copy), ctypes.byref(mfma)), "ffc_debug_peaks")
    say(f"PartialFFTConv stateful pieces: overlap_save=\"direct\" (step kernels) / overlap_save=True (blocked), B={B} H={H} bf16, {win} alternating "
        f"windows; us per step: median [min .. max]; streaming copy of this device {copy.value:.0f} GB/s")
    for P in ((2048,) if quick else (2048, 8192)):
        k = (torch.randn(H, P, device="cuda") * 0.1).requires_grad_(True)
        mods = {"direct": PartialFFTConv(P, overlap_save="direct").to("cuda"), "blocked": PartialFFTConv(P, overlap_save=True).to("cuda")}
        S = mods["direct"].state_len
        s = torch.randn(B, H, S, device="cuda").to(torch.bfloat16)
        for L in (1, 16, 64):
            x, dout = (torch.randn(B, H, L, device="cuda").to(torch.bfloat16) for _ in range(2))
            x.requires_grad_(True)
            with torch.no_grad():
                ys = {nm: step(m, x, k, s, dout, False) for nm, m in mods.items()}
            diff = max(float((ys["direct"][i].float() - ys["blocked"][i].float()).abs().max()) for i in (0, 1)) / float(ys["blocked"][0].float().abs().max())
            for bwd in (False, True):
                us, steps = {nm: [] for nm in mods}, {}
                for nm, m in mods.items():      # warm-up, and the window length from a first timing: about a quarter of a second
                    window(m, x, k, s, dout, 3, bwd)
                    steps[nm] = max(10, min(20000, int(250e3 / window(m, x, k, s, dout, 10, bwd))))
                for _ in range(win):
                    for nm, m in mods.items():
                        us[nm].append(window(m, x, k, s, dout, steps[nm], bwd))
                md = {nm: statistics.median(v) for nm, v in us.items()}
                line = f"P {P:5d} L {L:2d} {'fwd+bwd' if bwd else 'fwd    '}: " + "   ".join(
                    f"{nm} {md[nm]:8.1f} [{min(v):.1f} .. {max(v):.1f}]" for nm, v in us.items()) + f"   direct / blocked x{md['direct'] / md['blocked']:.3f}"
                if not bwd:
                    nbytes = 2 * (2 * B * H * S + 2 * B * H * L) + 4 * H * P      # state in and out, x and y, k
                    line += f"   direct moves {nbytes / 2 ** 20:.1f} MB: {nbytes / md['direct'] / 1e3:.0f} GB/s   |y - y_blocked| / max|y| {diff:.1e}"
                say(line)
        del mods, k, s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--quick"]
    table(args[0] if args else None, "--quick" in sys.argv)
