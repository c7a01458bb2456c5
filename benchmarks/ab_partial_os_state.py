"""PartialFFTConv(P, overlap_save=True) on a row held in pieces: chunks that carry the state against one call on the whole row and against
the work-around in torch, one process, alternating windows: forward, forward + backward and peak memory.

    python benchmarks/ab_partial_os_state.py [OUT.txt] [--quick]      the table of profiles/partial_os_state_ab.txt

y = conv(x, k[:, :P]), bf16, B = 2, H = 768, L in 262144, 1048576, P in 2048, 8192; n = 4 and 16 chunks of L / n samples.
  whole      mod(x, k): one call on the whole row
  state n    y_i, s = mod(x_i, k, state=s, return_state=True) chunk by chunk
  cat n      the work-around without the keywords: y_i = mod(cat(tail, x_i), k)[..., S:], tail = the last S samples of what went in
Forward + backward is truncated back-propagation in both chunked forms, the use that caps memory: every chunk's backward runs before
the next chunk's forward and the carried state (or tail) is detached, so the state-gradient block of the input-gradient launch is not
part of these figures.  Peak memory is that of forward + backward above the inputs and their gradients.  Each window is sized to about a quarter of a second
of device time; --quick: one length, three windows."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-fft-conv_amd"))
import torch
from flashfftconv import PartialFFTConv

B, H = 2, 768


def whole(mod, xs, k, douts, bwd):
    y = mod(xs[0], k)
    if bwd:
        y.backward(douts[0])


def with_state(mod, xs, k, douts, bwd):
    s = None
    for x, d in zip(xs, douts):
        y, s = mod(x, k, state=s, return_state=True)
        if bwd:
            y.backward(d)
        s = s.detach()


def with_cat(mod, xs, k, douts, bwd):
    S = mod.state_len
    tail = torch.zeros(B, H, S, dtype=xs[0].dtype, device="cuda")
    for x, d in zip(xs, douts):
        xin = torch.cat((tail, x), -1)
        y = mod(xin, k)[..., S:]
        if bwd:
            y.backward(d)
        tail = xin[..., -S:].detach()


def window(form, mod, xs, k, douts, steps, bwd):
    """ms per row, device events around `steps` rows"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        if bwd:
            for v in xs + [k]:
                v.grad = None
            form(mod, xs, k, douts, True)
        else:
            with torch.no_grad():
                form(mod, xs, k, douts, False)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def peak_mb(form, mod, xs, k, douts):
    """(the gradients of the last step are part of the base, as in ab_partial_os_gated.py: the figure is what a step needs beyond inputs and gradients)"""
    form(mod, xs, k, douts, True)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for v in xs + [k]:
        v.grad = None
    form(mod, xs, k, douts, True)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def table(path, quick):
    out = open(path, "w") if path else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()
    win = 3 if quick else 5
    say(f"PartialFFTConv(P, overlap_save=True) on a row in pieces: whole row / chunks with state= / chunks with cat + crop, B={B} H={H} bf16, "
        f"{win} alternating windows; ms per row: median [min .. max]; fwd+bwd of the chunked forms is truncated at the chunk")
    for L in ((262144,) if quick else (262144, 1048576)):
        x, dout = (torch.randn(B, H, L, device="cuda").to(torch.bfloat16) for _ in range(2))
        data = {"whole": ([x.requires_grad_(True)], [dout])}
        for n in (4, 16):
            data[f"state {n}"] = data[f"cat {n}"] = ([c.contiguous().requires_grad_(True) for c in x.detach().chunk(n, -1)],
                                                     [c.contiguous() for c in dout.chunk(n, -1)])
        forms = {nm: whole if nm == "whole" else with_state if nm.startswith("state") else with_cat for nm in data}
        for P in (2048, 8192):
            k = (torch.randn(H, P, device="cuda") * 0.1).requires_grad_(True)
            mod = PartialFFTConv(P, overlap_save=True).to("cuda")
            for bwd in (False, True):
                ms, steps = {nm: [] for nm in forms}, {}
                for nm, f in forms.items():      # warm-up, and the window length from a first timing
                    window(f, mod, data[nm][0], k, data[nm][1], 1, bwd)
                    steps[nm] = max(2, min(100, int(250.0 / window(f, mod, data[nm][0], k, data[nm][1], 2, bwd))))
                for _ in range(win):
                    for nm, f in forms.items():
                        ms[nm].append(window(f, mod, data[nm][0], k, data[nm][1], steps[nm], bwd))
                m0 = statistics.median(ms["whole"])
                say(f"L {L:8d} P {P:5d} {'fwd+bwd' if bwd else 'fwd    '}: " + "   ".join(
                    f"{nm} {statistics.median(v):8.3f} [{min(v):.3f} .. {max(v):.3f}] x{statistics.median(v) / m0:.3f}" for nm, v in ms.items()))
            say(f"L {L:8d} P {P:5d} peak MB of fwd+bwd above the inputs and gradients: " + "   ".join(f"{nm} {peak_mb(f, mod, data[nm][0], k, data[nm][1]):.0f}" for nm, f in forms.items()))
            del mod
            torch.cuda.empty_cache()
        del x, dout, data
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--quick"]
    table(args[0] if args else None, "--quick" in sys.argv)
