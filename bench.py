"""Benchmark of the FlashFFTConv hot path on MI355X (driver contract: see task statement).

Step = one forward + backward of FlashFFTConv(32768) on BASELINE.json configs[1]
(B=16, H=768, L=16384, bf16 activations, fp32 k), synthetic randn inputs resident in HBM:
   k -> k_f (kfft kernel), conv forward, fused backward (du + fp32 dk_f partial sums), dk inverse.
Nothing is cached between steps (the reference recomputes k_f every forward, conv.py:572-575).  The module default is timed:
its training forward keeps FFT(u) for the backward pass of the same step (module.save_spectrum, 2x the bytes of u), so the
backward kernel runs two transforms per pair instead of three; the object `recompute` holds the same step with
save_spectrum = False (the reference's memory footprint: its backward kernels transform u again).

N > 1 GPUs: one process per GPU, heads sharded, no data-path collective.  BASELINE's metric is the FIXED problem (B=16 x
H=768 on 1/2/4/8 GPUs), so for N > 1 `value` is that problem with H/N heads per rank ("scaling": "strong", timed with the
contract's barrier + max over ranks); the object `weak` beside it holds the weak-scaled job of the same run (every rank runs
the full per-GPU shape on its own 768 heads).  At N = 1 the two coincide.

A plain run (`--gpus 1 --steps K --warmup W`) does only what the headline needs: set-up, preheat + W warm-up steps, K timed steps,
the outputs of the last timed step if `--dump-outputs DIR` is given, and the contract line (contract keys, `ms_per_step`, the two
TFLOP/s figures).

`--full` adds everything else, after the headline: the recompute-mode step, the torch.utils.benchmark timing, per-kernel times and
the roofline objects, the box's measured peaks, the CPU baseline, and (N = 1) the tables -- BASELINE sweep (B=16, H=768,
L = 1K .. 1M), gated sweep rows, configs[1..4], the reference's README table -- or (N > 1) the weak-scaled job and the strong-scaled
rows.  The tables are printed before the contract line, one JSON line per row; the line carries `roofline`, `roofline_fwd`,
`cpu_baseline`, kernel times and a [fwd, bwd] ms digest per table row; the complete object goes to bench_out/bench_full.json.

`--dump-outputs DIR`: what a caller of the timed step receives from its last step, as float32 .npy files -- y = the forward output,
du = u.grad, dk = k.grad -- each a fixed, seeded sample of DUMP_ROWS rows (full rows of L), about 50 MB in all.  The inputs are
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse, hashlib, json, os, sys, time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "flash-fft-conv_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

CFG = dict(N=32768, B=16, H=768, L=16384, dtype=torch.bfloat16)
# nominal peaks (MI355X_MICROARCH.md); the measured ones of the box are reported as `peak_measured`
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
MFMA_PEAK_TFLOPS = 2500.0   # dense bf16
MFMA_FLOP = 2 * 32 * 32 * 16  # one v_mfma_f32_32x32x16_bf16


# ---- the contract line ------------------------------------------------------------------------------------------------
# The driver parses the LAST stdout line as one JSON object.  Round 4 printed everything (sweep, README table, peak-memory
# objects) on that line: 24 KB, and the driver's parser gave up (BENCH_r04.json parsed: null).  Now: the tables go out as one
# small JSON line per row BEFORE the contract line, the complete object is written to a side file, and the contract line holds
# the contract keys plus a few numbers per table row -- asserted below LINE_LIMIT bytes.
LINE_LIMIT = 4096
ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "frac_traffic", "launch_ms", "alg_bytes", "frac_hbm", "frac_executed")
CPU_KEYS = ("value", "unit", "cores", "kind", "sample", "host_cpus")


def _r(x, nd=4):
    """round floats (recursively) so that the line stays short; ints / strings / None pass through"""
    if isinstance(x, float):
        return float(f"{x:.{nd}g}") if abs(x) < 1 else round(x, 3)
    if isinstance(x, dict):
        return {k: _r(v, nd) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, nd) for v in x]
    return x


def _peak3(pm):
    """peak-memory object of a row reduced to three integers (MB): fwd+bwd with saved spectra / recomputing / torch.fft form"""
    if not pm:
        return None
    mb = lambda k: None if pm.get(k) is None else int(round(pm[k] / 1e6))
    return [mb("fwd_bwd_save_spectrum"), mb("fwd_bwd_recompute"), mb("fwd_bwd_torch_fft")]


def _row_line(table, r):
    r = {k: v for k, v in r.items() if k not in ("timing",)}
    if "peak_mem_bytes" in r:
        r["peak_fwd_bwd_MB"] = _peak3(r.pop("peak_mem_bytes"))
    return {"table": table, **_r(r)}


def compact(out):
    """the contract line: contract keys + roofline / cpu_baseline objects + per-row digests of the tables"""
    c = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data", "config") if k in out}
    for k in ("roofline", "roofline_fwd"):
        if out.get(k):
            r = {kk: out[k][kk] for kk in ROOF_KEYS if kk in out[k]}
            r["kernel"] = r["kernel"].split(":")[0].split(" (")[0][:80]
            tp = out[k].get("traffic_profiled")
            if tp:      # `traffic` is read from a committed rocprofv3 --pmc summary, not measured in this run: say which one
                r["traffic_source"] = f"{tp['file']}#{tp['sha256_16']}"
            c[k] = r
    if out.get("cpu_baseline"):
        c["cpu_baseline"] = {k: out["cpu_baseline"][k] for k in CPU_KEYS if k in out["cpu_baseline"]}
    for k in ("kernel_ms", "peak_measured", "recompute", "strong", "weak"):
        if out.get(k):
            v = dict(out[k])
            for drop in ("how", "guide_figures", "what", "workload"):
                v.pop(drop, None)
            c[k] = v
    # BASELINE's metric is "TFLOP/s & seq/s": both TFLOP/s figures of the headline step ride on the line (VERDICT r05 missing #5)
    for k in ("tflops_fft_equiv", "tflops_dense_monarch"):
        if out.get(k) is not None:
            c[k] = out[k]
    if out.get("ms_per_step_torch_benchmark_timer") is not None:
        c["ms_per_step_timer"] = out["ms_per_step_torch_benchmark_timer"]
    if out.get("preheat_steps") is not None:
        c["preheat_steps"] = out["preheat_steps"]
    # tables: [fwd_ms, bwd_ms] per row, keyed by L (sweep) / config name; README table: speed-up over the published H100 time
    if out.get("sweep"):
        c["sweep_fwd_bwd_ms"] = {str(r["L"]): [r["fwd_ms"], r["bwd_ms"]] for r in out["sweep"]}
        gs = {str(r["L"]): r["graph_step_ms"] for r in out["sweep"] if r.get("graph_step_ms") is not None}
        if gs:      # short rows: fwd+bwd as one HIP graph (the eager backward is host-bound there)
            c["sweep_graph_step_ms"] = gs
    if out.get("sweep_gated"):
        c["sweep_gated_fwd_bwd_ms"] = {str(r["L"]): [r["fwd_ms"], r["bwd_ms"]] for r in out["sweep_gated"]}
    if out.get("configs"):
        c["configs_fwd_bwd_ms"] = {r["row"].split(" ")[0]: [r["fwd_ms"], r["bwd_ms"]] for r in out["configs"]}
        # rows whose module ran a smaller fft size than it was built for (FlashFFTConv._fit_seqlen: cfg4's rows fit 2097152 points)
        fr = {r["row"].split(" ")[0]: r["fft_run"] for r in out["configs"] if r.get("fft_run") not in (None, r.get("fft"))}
        if fr:
            c["configs_fft_run"] = fr
            # ... and the same module forced to its full size (fit_fft = False), for comparison
            c["configs_seqlen_points_fwd_bwd_ms"] = {r["row"].split(" ")[0]: [r.get("fwd_ms_seqlen_points"), r.get("bwd_ms_seqlen_points")]
                                                     for r in out["configs"] if r["row"].split(" ")[0] in fr}
    if out.get("readme_table"):
        c["readme_x_h100"] = {str(r["fft"]): r["speedup_vs_h100_published"] for r in out["readme_table"]}
        if all("speedup_vs_h100_timer" in r for r in out["readme_table"]):      # the same rows timed with the reference's tool (host clock)
            c["readme_x_h100_timer"] = {str(r["fft"]): r["speedup_vs_h100_timer"] for r in out["readme_table"]}
        if all("bwd_ms_scaled" in r for r in out["readme_table"]):
            c["readme_gated_fwd_bwd_ms"] = {str(r["fft"]): [r["fwd_ms_scaled_to_B64_H768"], r["bwd_ms_scaled"]] for r in out["readme_table"]}
    if out.get("strong_rows"):      # N > 1: the fixed-problem rows of the metric's grid, [fwd+bwd ms, heads per rank] (max over ranks)
        c["strong_rows_step_ms"] = {r["row"]: [r["step_ms"], r["heads_per_rank"]] for r in out["strong_rows"]}
    if out.get("scaling_note"):
        c["scaling_note"] = out["scaling_note"]
    if out.get("full"):
        c["full"] = out["full"]
    return _r(c)


def emit(out, full_path=None, stream=None):
    """table rows (one JSON line each), the full object to `full_path`, then the contract line -- LAST, < LINE_LIMIT bytes"""
    stream = stream or sys.stdout
    for table in ("configs", "sweep", "sweep_gated", "readme_table", "strong_rows"):
        for r in out.get(table) or ():
            print(json.dumps(_row_line(table, r)), file=stream, flush=True)
    if full_path:
        try:
            os.makedirs(os.path.dirname(full_path), exist_ok=True)
            with open(full_path, "w") as f:
                json.dump(out, f)
            out = dict(out, full=os.path.relpath(full_path, ROOT))
        except OSError:
            pass
    line = json.dumps(compact(out))
    assert len(line) < LINE_LIMIT, f"contract line is {len(line)} bytes (limit {LINE_LIMIT})"
    print(line, file=stream, flush=True)
    return line


def flops_dense_fwd_per_row(N):
    # reference factorisation 32x32x32, r2c first / c2r last stage
    n = [32, 32, 32]; p = 3
    return 2 * (sum(8 * N * ni for ni in n) - 4 * N * n[0]) + 6 * N * (2 * (p - 1) + 1)


def flops_fft_equiv(N):
    import math
    lg = math.log2(N)
    return 2 * 5 * N * lg + 6 * N, 3 * 5 * N * lg + 14 * N


def mfma_per_pair_32k_half():
    """MFMA instructions the kernels EXECUTE per packed pair (two batch rows as one complex sequence) at fft 32768,
    L <= N/2 (csrc/ffc_body.h): 8 waves x 4 tiles; phase A (half-empty outer digit) 4, phase B 16 forward + 16 inverse,
    phase C 8 per tile.  forward = A + B + C; fused backward = 2 forward halves + 1 inverse half."""
    tiles = 8 * 4
    fwd_half, inv_half = 4 + 16, 16 + 8
    return tiles * (fwd_half + inv_half), tiles * (2 * fwd_half + inv_half)


def time_kernel(fn, iters=20):
    """HIP-event timing on torch's current stream (the stream the library launches on)."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def cpu_baseline(seconds_per_point=3.0):
    """Reference CPU path (torch.fft oracle, oracle/torch_ref.py) fwd+bwd on an H-slice of the workload, at several thread
    counts (pocketfft over a batch oversubscribes quickly: round 1 timed 256 threads only and got 15x less than 8 threads
    gives); the best one is reported with its thread count."""
    from oracle.torch_ref import ref_fft_conv
    B, L, N, Hs = CFG["B"], CFG["L"], CFG["N"], 48
    g = torch.Generator().manual_seed(0)
    u = torch.randn(B, Hs, L, generator=g).to(CFG["dtype"]).requires_grad_(True)
    k = torch.randn(Hs, L, generator=g).requires_grad_(True)
    dout = torch.randn(B, Hs, L, generator=g).to(CFG["dtype"])

    def step():
        u.grad = None; k.grad = None
        ref_fft_conv(u, k, n=N).backward(dout)

    ncpu = os.cpu_count() or 1
    tried, best = {}, None
    for th in sorted({t for t in (8, 16, 32, 64, 128, 256) if t <= ncpu} | {min(ncpu, 8)}):
        torch.set_num_threads(th)
        step()
        t0 = time.perf_counter(); reps = 0
        while True:
            step(); reps += 1
            el = time.perf_counter() - t0
            if el > seconds_per_point or reps >= 50:
                break
        v = B * Hs * reps / el
        tried[str(th)] = round(v, 1)
        if best is None or v > best[0]:
            best = (v, th, reps, el)
    v, th, reps, el = best
    return {"value": v, "unit": "seq/s", "cores": th, "kind": "port", "host_cpus": ncpu, "by_threads": tried,
            "sample": f"fwd+bwd, B={B} H={Hs} (1/16 of H=768) L={L} fft={N}, {reps} reps in {el:.1f}s at the best of "
                      f"{len(tried)} thread counts, torch.fft oracle"}


PREHEAT_S = 0.5
DUMP_ROWS = 256


def dump_outputs(d, y, du, dk):
    """y, du: (B, H, L); dk: (H, L) -> d/{y,du,dk}.npy in float32, DUMP_ROWS rows of each picked by a fixed seed"""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0)
    for name, t in (("y", y), ("du", du), ("dk", dk)):
        t = t.detach().reshape(-1, t.shape[-1])
        rows = np.sort(rng.choice(t.shape[0], size=min(DUMP_ROWS, t.shape[0]), replace=False))
        a = t[torch.from_numpy(rows).to(t.device)].float().cpu().numpy()
        np.save(os.path.join(d, name + ".npy"), a)


def timed_steps(step, steps, warmup, dist, dev):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = t.item()
    return el


# N > 1: the rest of BASELINE's metric ("B=16 H=768 L in 1K .. 1M, 1/2/4/8 GPU" and configs[3] "1 vs 8 GPU H-sharded") as STRONG-scaled rows:
# the fixed problem, this rank's share of the heads, no data-path collective; fwd+bwd per step, barrier-bracketed, max over ranks
# (reference harness for the grid: benchmarks/benchmark_flashfftconv.py:94-212).  Heads above the single-GPU sweep's memory cap are
# rescaled linearly, as that sweep (and the reference's own benchmark) does; the row says so.
STRONG_ROWS = [("sweep L=1024", 2048, 16, 768, 1024), ("sweep L=16384", 32768, 16, 768, 16384), ("sweep L=131072", 262144, 16, 768, 131072),
               ("sweep L=1048576", 2097152, 16, 768, 1048576), ("cfg4 H-sharded", 4194304, 1, 16, 1048576)]


def strong_scaled_rows(world, rank, dist, dev, rows=None, steps=None):
    from flashfftconv import FlashFFTConv
    from flashfftconv.sharding import head_range
    out = []
    for (name, N, B, H, L) in (rows or STRONG_ROWS):
        s0, s1 = head_range(H, rank, world)
        hr = s1 - s0
        cap = H if N <= 131072 else max(1, (768 * 131072 // N) * 16 // B)      # heads one GPU holds at this size (benchmarks/sweep.py sweep_rows)
        hrun = max(1, min(hr, cap))
        u = torch.randn(B, hrun, L, device=dev).to(CFG["dtype"]).requires_grad_(True)
        k = torch.randn(hrun, L, device=dev).requires_grad_(True)
        dout = torch.randn(B, hrun, L, device=dev).to(CFG["dtype"])
        mod = FlashFFTConv(N, dtype=CFG["dtype"]).to(dev)

        def step():
            u.grad = None; k.grad = None
            mod(u, k).backward(dout)
        n = steps or (10 if N <= 262144 else 3)
        el = timed_steps(step, n, 2, dist, dev)
        ms = el / n * 1e3 * (hr / hrun)
        out.append({"row": name, "fft": N, "fft_run": mod._fit_seqlen(L, L), "B": B, "H": H, "L": L, "n_gpus": world, "heads_per_rank": hr, "H_run": hrun,
                    "rescaled": hrun != hr, "step_ms": ms, "seq_per_s": B * H / (ms * 1e-3), "scaling": "strong",
                    "timing": f"fwd+bwd, {n} steps between barriers, max over {world} ranks"})
        del u, k, dout, mod
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="everything beyond the headline step (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-sweep", action="store_true", help="--full without the tables")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if int(os.environ.get("FFC_BENCH_SAME_GPU", "0")):     # test hook: all ranks on cuda:0
            local = 0
        torch.cuda.set_device(local)
        # RCCL ("nccl" on ROCm) over xGMI; FFC_BENCH_BACKEND=gloo only exists to exercise this path on a 1-GPU box
        dist.init_process_group(os.environ.get("FFC_BENCH_BACKEND", "nccl"), rank=rank, world_size=world)
    dev = torch.device("cuda", local if world > 1 else 0)
    torch.cuda.set_device(dev)

    from flashfftconv import FlashFFTConv
    from flashfftconv import conv as C, _lib
    from flashfftconv.sharding import head_range

    N, B, H, L, dtype = CFG["N"], CFG["B"], CFG["H"], CFG["L"], CFG["dtype"]
    torch.manual_seed(rank)
    u = torch.randn(B, H, L, device=dev).to(dtype).requires_grad_(True)
    k = torch.randn(H, L, device=dev).requires_grad_(True)
    dout = torch.randn(B, H, L, device=dev).to(dtype)
    mod = FlashFFTConv(N, dtype=dtype).to(dev)
    # --dump-outputs: the forward output of the last step is kept (detached: no reference to the autograd graph)
    keep_y = args.dump_outputs is not None and rank == 0
    last = {}

    def step():
        u.grad = None; k.grad = None
        y = mod(u, k)
        y.backward(dout)
        if keep_y:
            last["y"] = y.detach()

    # Preheat (untimed, before the W warm-up steps): a fresh process starts with the GPU in a low power state and the first
    # ~100 steps run 3-6 % slower than steady state (measured: W=5 1.35 ms, W=50 1.29, W=300 1.27 per step at K=20), so the
    # job first runs the step for PREHEAT_S seconds.  Reported in the JSON line as "preheat_steps".
    preheat = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < PREHEAT_S:
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        preheat += 10

    # ---- the headline.  N = 1: the step above.  N > 1: strong scaling, the FIXED B=16 x H=768 problem, this rank's H/world heads
    # (no collective in the data path)
    strong = None
    if world == 1:
        el = timed_steps(step, args.steps, args.warmup, dist, dev)
        outs = (u.grad, k.grad)
    else:
        s0, s1 = head_range(H, rank, world)
        us = u.detach()[:, s0:s1].contiguous().requires_grad_(True)
        ks = k.detach()[s0:s1].contiguous().requires_grad_(True)
        ds = dout[:, s0:s1].contiguous()

        def step_s():
            us.grad = None; ks.grad = None
            y = mod(us, ks)
            y.backward(ds)
            if keep_y:
                last["y"] = y.detach()
        el_s = timed_steps(step_s, args.steps, args.warmup, dist, dev)
        outs = (us.grad, ks.grad)
        strong = {"value": B * H / (el_s / args.steps), "unit": "seq/s", "ms_per_step": el_s / args.steps * 1e3,
                  "scaling": "strong", "heads_per_rank": s1 - s0,
                  "workload": f"the fixed B={B} H={H} L={L} problem, {H}//{world} heads per rank"}
    if keep_y:
        dump_outputs(args.dump_outputs, last.pop("y"), *outs)
    del outs

    rows = B * H
    dense_fwd = flops_dense_fwd_per_row(N)
    fft_fwd, fft_bwd = flops_fft_equiv(N)
    head_value = strong["value"] if strong is not None else world * rows / (el / args.steps)
    head_ms = strong["ms_per_step"] if strong is not None else el / args.steps * 1e3
    out = {
        "metric": "FFT-conv fwd+bwd seq/s, B=16 H=768 L=16384 fft=32768 bf16",
        "value": head_value, "unit": "seq/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "preheat_steps": preheat,
        "ms_per_step": head_ms, "higher_is_better": True,
        "scaling": "weak" if world == 1 else "strong", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {"workload": "FlashFFTConv(32768) B=16 H=768 L=16384 bf16, fwd+bwd incl. k->k_f and dk (BASELINE configs[1])",
                   "rows_per_step": rows, "heads_per_rank": (strong or {}).get("heads_per_rank", H),
                   "parallelism": f"head-shard x{world} (no collective)"},
        # TFLOP/s of the SAME step as `value` (N > 1: the fixed problem's rows over the strong-scaled step)
        "tflops_dense_monarch": rows * dense_fwd * 2.5 / (head_ms * 1e-3) / 1e12,
        "tflops_fft_equiv": rows * (fft_fwd + fft_bwd) / (head_ms * 1e-3) / 1e12,
    }
    if strong is not None:
        out["strong"] = strong
    # one place that says it: no multi-GPU run has ever been measured by the builder (every box has ONE GPU; RCCL has only run world-size-1)
    out["scaling_note"] = "N>1 never measured by the builder: 1-GPU boxes only" if world == 1 else None
    if not args.full:
        if rank == 0:
            emit(out)
        if dist is not None:
            dist.destroy_process_group()
        return

    # ---- --full from here on
    if world > 1:       # the weak-scaled job of the same run: every rank runs the full per-GPU shape on its own 768 heads
        el = timed_steps(step, args.steps, args.warmup, dist, dev)
    # the same step with the reference's memory footprint (FFT(u) recomputed by the backward kernel)
    mod.save_spectrum = False
    el_rc = timed_steps(step, args.steps, args.warmup, dist, dev)
    mod.save_spectrum = True
    # the same step under torch.utils.benchmark.Timer, the reference's own timing tool (benchmarks/benchmark.py:16-21), for
    # comparability with its published tables; the contract figure above is the barrier-bracketed wall clock
    from torch.utils import benchmark as tbench
    timer_ms = tbench.Timer(stmt="step()", globals={"step": step}).timeit(args.steps).mean * 1e3

    strong_rows = None
    if world > 1 and not args.no_sweep:
        sel = os.environ.get("FFC_BENCH_STRONG_ROWS")      # test hook: a comma-separated subset of the row names
        strong_rows = strong_scaled_rows(world, rank, dist, dev, [r for r in STRONG_ROWS if not sel or r[0] in sel.split(",")])

    # ---- per-kernel timing (rank 0 reports): the launches of one step
    plan = mod._get_plan(dev)
    ud, kd = u.detach(), k.detach()
    kf = C._kernel_fft(plan, kd)
    lib = _lib.lib()
    P = _lib.ptr
    ws = torch.empty(lib.ffc_dkf_workspace_bytes(plan.handle, B, H), dtype=torch.uint8, device=dev)
    zb = torch.empty(lib.ffc_spectrum_bytes(plan.handle, B, H), dtype=torch.uint8, device=dev)
    dk = torch.empty(H, L, dtype=torch.float32, device=dev)
    dk_du = torch.empty_like(ud)
    y_buf = torch.empty_like(ud)
    sp = _lib.stream_ptr
    z2 = torch.empty(lib.ffc_spectrum_bytes(plan.handle, B, H), dtype=torch.uint8, device=dev)
    calls = {
        # the module's two calls (round 4): k -> k_f inside the forward launch, dk out of the backward launch (one chunk per head)
        "conv_fwd_k": lambda: _lib.check(lib.ffc_conv_fwd_k(plan.handle, P(kd), L, P(kf), P(ud), None, None, P(y_buf), P(z2), None, B, H, L, sp()), "fwd_k"),
        "conv_bwd_k": lambda: _lib.check(lib.ffc_conv_bwd_k(plan.handle, P(dout), P(ud), P(kf), None, None, P(dk_du), None, None, P(ws), P(z2), None, P(dk), L, B, H, L, sp()), "bwd_k"),
        "kfft": lambda: _lib.check(lib.ffc_kernel_fft(plan.handle, P(kd), H, L, P(kf), sp()), "kfft"),
        "conv_fwd_save": lambda: _lib.check(lib.ffc_conv_fwd_z(plan.handle, P(ud), P(kf), None, None, P(y_buf), P(zb), None, B, H, L, 0, 0, 0, 0, sp()), "fwd_z"),
        "bwd_fused_saved": lambda: _lib.check(lib.ffc_conv_bwd_z(plan.handle, P(dout), P(ud), P(kf), None, None, P(dk_du), None, None, P(ws), P(zb), B, H, L,
                                                             0, 0, 0, 0, 0, 0, 0, sp()), "bwd_z"),
        "dk_ifft": lambda: _lib.check(lib.ffc_kernel_ifft_grad(plan.handle, P(ws), B, H, L, P(dk), sp()), "dk"),
    }
    # (a) inside the step sequence: one event after every launch of K back-to-back steps (what the step really pays per kernel:
    #     a kernel that starts on the heels of another one runs slower than in a loop of its own)
    order = ["conv_fwd_k", "conv_bwd_k"]
    order_r03 = ["kfft", "conv_fwd_save", "bwd_fused_saved", "dk_ifft"]      # the four separate launches of round 3, timed the same way
    for _ in range(5):
        for n in order + order_r03: calls[n]()
    torch.cuda.synchronize()
    K = 20
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)] for _ in range(K)]
    for i in range(K):
        evs[i][0].record()
        for j, n in enumerate(order):
            calls[n](); evs[i][j + 1].record()
    torch.cuda.synchronize()
    kt_step = {n: sum(evs[i][j].elapsed_time(evs[i][j + 1]) for i in range(K)) / K * 1e-3 for j, n in enumerate(order)}
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(order_r03) + 1)] for _ in range(K)]
    for i in range(K):
        evs[i][0].record()
        for j, n in enumerate(order_r03):
            calls[n](); evs[i][j + 1].record()
    torch.cuda.synchronize()
    kt_step.update({n: sum(evs[i][j].elapsed_time(evs[i][j + 1]) for i in range(K)) / K * 1e-3 for j, n in enumerate(order_r03)})
    # (b) each kernel in a loop of its own, plus the recomputing pair and the two halves of the backward for reference
    kt = {n: time_kernel(calls[n]) for n in order + order_r03}
    kt.update({
        "conv_fwd": time_kernel(lambda: C._conv(plan, ud, kf, None, None, False)),
        "conv_dx": time_kernel(lambda: C._conv(plan, dout, kf, None, None, True)),
        "bwd_fused": time_kernel(lambda: _lib.check(lib.ffc_conv_bwd(plan.handle, P(dout), P(ud), P(kf), None, None, P(dk_du), None, P(ws), B, H, L, sp()), "bwd")),
        "dkf_only": time_kernel(lambda: _lib.check(lib.ffc_conv_bwd_dkf(plan.handle, P(dout), P(ud), None, None, P(ws), B, H, L, sp()), "dkf")),
    })
    peaks = None
    if rank == 0:
        import ctypes
        cg, mt = ctypes.c_double(), ctypes.c_double()
        del zb, z2
        if lib.ffc_debug_peaks(ctypes.byref(cg), ctypes.byref(mt)) == 0:
            peaks = {"stream_copy_GBs": round(cg.value), "mfma_bf16_dense_TFLOPs": round(mt.value),
                     "how": "streaming (non-temporal) 4 x 16 B per lane copy of 2 GiB to 2 GiB (read + write bytes), best over grids of 2..32 "
                            "workgroups per CU x 3 launches; register-resident v_mfma_f32_32x32x16_bf16 loop, best of 3",
                     "guide_figures": "MI355X_MICROARCH.md: 6.29 TB/s measured float4 copy (79 % of the 8 TB/s spec), 2.5 PFLOP/s dense bf16"}
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    npair = (B // 2) * H
    sec_per_step = el / args.steps
    seq_s = world * rows / sec_per_step
    # Roofline objects: `roofline` = the dominant kernel of the step (the fused backward, ~60 % of the step time),
    # `roofline_fwd` = the forward conv_kernel.  Three yardsticks, all per launch and all over the launch time measured
    # above with HIP events:
    #   hbm            algorithmic bytes                                       / 8 TB/s
    #   mfma_executed  MFMA flops the pair-packed kernel really issues (mfma_per_pair_32k_half) / 2.5 PFLOP/s
    #   mfma_reference SURVEY 8(d)'s dense-Monarch count of the REFERENCE's r2c/c2r factorisation (42.9 MFLOP/row forward,
    #                  63.4 backward) -- about twice what these kernels execute; kept for comparability with round 1 only
    # `bound` is whichever of hbm / mfma_executed gives the LONGER ideal time, `achieved`/`peak`/`frac` are on that basis.
    matmul_fwd = dense_fwd - 30 * N
    dense_bwd = 1.5 * matmul_fwd + 14 * N
    mf_fwd, mf_bwd = mfma_per_pair_32k_half()
    fwd_bytes = B * H * L * 2 * 2 + H * N * 4                      # read u, write y, read k_f once
    bwd_bytes = B * H * L * 2 * 3 + H * N * 4 + H * N * 8          # read u + dout, write du, read k_f, write fp32 dk_f

    def prof_traffic(fname, key):
        """HBM traffic per launch from a rocprofv3 --pmc profile committed under profiles/ (NOT measured in this run:
        PMC passes serialise the kernel and need rocprofv3 around the process).  Returned with the file's hash."""
        path = os.path.join(ROOT, "profiles", fname)
        if not os.path.exists(path):
            return None
        txt = open(path).read()
        import re
        m = re.search(key + r"\D+([0-9.]+)\s*MB", txt)
        return {"bytes": float(m.group(1)) * 1e6 if m else None, "file": "profiles/" + fname,
                "sha256_16": hashlib.sha256(txt.encode()).hexdigest()[:16]}

    def roof(name, mfma_pair, dense_row, alg_bytes, t, prof):
        ex_flops = mfma_pair * npair * MFMA_FLOP
        t_hbm, t_mfma = alg_bytes / (HBM_PEAK_GBS * 1e9), ex_flops / (MFMA_PEAK_TFLOPS * 1e12)
        hbm = {"achieved": alg_bytes / t / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg_bytes / t / 1e9 / HBM_PEAK_GBS}
        mf = {"achieved": ex_flops / t / 1e12, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ex_flops / t / 1e12 / MFMA_PEAK_TFLOPS}
        bound = "hbm" if t_hbm >= t_mfma else "mfma"
        r = {"kernel": name, "bound": bound, **(hbm if bound == "hbm" else mf),
             # HBM-side bytes per launch from the committed rocprofv3 --pmc pass of this kernel (PMC passes need rocprofv3 around
             # the process, so they cannot be taken inside this run; file + hash in traffic_profiled); null without the file
             "traffic": (prof or {}).get("bytes"),
             "traffic_profiled": prof, "launch_ms": t * 1e3, "alg_bytes": alg_bytes,
             "t_ideal_hbm_us": t_hbm * 1e6, "t_ideal_mfma_executed_us": t_mfma * 1e6,
             "frac_hbm": hbm["frac"], "frac_executed": mf["frac"], "executed_TFLOPs": mf["achieved"],
             "frac_reference_basis": dense_row * rows / t / 1e12 / MFMA_PEAK_TFLOPS,
             "basis": "achieved = algorithmic bytes (or executed MFMA flops) per launch / launch_ms; launch_ms = HIP events after every "
                      "launch of 20 back-to-back steps of this run (the conservative figure: each event costs the sequence ~14 us, so the "
                      "four in-step times add up to MORE than the measured step, see kernel_sum_check); launch_ms_isolated_loop = events "
                      "around a loop of launches of this kernel alone"}
        return r

    # the backward kernel on saved spectra executes one forward half + one inverse half per pair
    mf_bwd_saved = mf_bwd - 32 * (4 + 16)
    roof_bwd = roof("bwd_kernel<Geo<32,32,32>,bf16,HALF,ZM=1> on saved spectra: du + dk in one launch (dk_f stays in the accumulation registers and is inverted by the same workgroup; the recomputing form is the ZM=0 instantiation)", mf_bwd_saved, dense_bwd, bwd_bytes,
                    kt_step["conv_bwd_k"], prof_traffic("r06_pmc_bwd_kernel.txt", "traffic") or prof_traffic("r05_pmc_bwd_kernel.txt", "traffic"))
    roof_bwd["launch_ms_isolated_loop"] = kt["conv_bwd_k"] * 1e3
    roof_bwd["launch_ms_without_dk_tail"] = kt_step["bwd_fused_saved"] * 1e3      # + dk_ifft as its own launch (round 3 form)
    roof_bwd["extra_bytes_not_in_alg_bytes"] = {"saved_spectra_read": npair * N * 4, "u_not_read_any_more": -B * H * L * 2}
    roof_fwd = roof("conv_kernel<Geo<32,32,32>,bf16,HALF,SZ> (training forward: k -> k_f of the head, convolution, stores the spectra)", mf_fwd, dense_fwd, fwd_bytes,
                    kt_step["conv_fwd_k"], prof_traffic("r06_pmc_conv_kernel.txt", "traffic") or prof_traffic("r05_pmc_conv_kernel.txt", "traffic"))
    roof_fwd["launch_ms_isolated_loop"] = kt["conv_fwd_k"] * 1e3
    roof_fwd["launch_ms_without_kfft_head"] = kt_step["conv_fwd_save"] * 1e3      # + kfft as its own launch (round 3 form)
    roof_fwd["extra_bytes_not_in_alg_bytes"] = {"saved_spectra_write": npair * N * 4}
    for r in (roof_bwd, roof_fwd):      # bytes the kernel really has to move (incl. the spectra) vs the profiled traffic
        r["bytes_to_move"] = r["alg_bytes"] + sum(r["extra_bytes_not_in_alg_bytes"].values())
        r["traffic_over_bytes_to_move"] = round(r["traffic"] / r["bytes_to_move"], 3) if r["traffic"] else None
        # the same launch time against the bytes that REALLY cross the fabric (profiled traffic: the saved spectra and the per-pair k_f
        # re-reads included): the memory system's view of the kernel, next to `frac` = the algorithmic bytes of SURVEY 8(d)
        r["frac_traffic"] = r["traffic"] / (r["launch_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS if r["traffic"] else None
    roof_bwd_rc = roof("bwd_kernel<Geo<32,32,32>,bf16,HALF> recomputing FFT(u) (save_spectrum = False)", mf_bwd, dense_bwd, bwd_bytes,
                       kt["bwd_fused"], prof_traffic("r02_pmc_bwd_kernel.txt", "traffic"))
    out.update({
        "ms_per_step_torch_benchmark_timer": timer_ms,
        "kernel_ms": {n: v * 1e3 for n, v in kt_step.items()},
        "kernel_ms_how": "HIP events between the launches of 20 back-to-back steps: conv_fwd_k + conv_bwd_k = the module's two launches "
                         "(round 4); kfft / conv_fwd_save / bwd_fused_saved / dk_ifft = the same work as round 3's four launches",
        "kernel_sum_check": {"ms_per_step": sec_per_step * 1e3, "sum_isolated_loops_ms": sum(kt[n] for n in order) * 1e3,
                             "sum_event_bracketed_in_step_ms": sum(kt_step[n] for n in order) * 1e3,
                             "four_launch_form_in_step_ms": sum(kt_step[n] for n in order_r03) * 1e3},
        "kernel_ms_isolated_loops": {n: v * 1e3 for n, v in kt.items()},
        "roofline": roof_bwd,
        "roofline_fwd": roof_fwd,
        "roofline_bwd_recompute": roof_bwd_rc,
        "recompute": {"value": world * rows / (el_rc / args.steps), "unit": "seq/s", "ms_per_step": el_rc / args.steps * 1e3,
                      "what": "the same step with module.save_spectrum = False: the backward kernel transforms u again (reference behaviour, "
                              "no spectra kept between forward and backward)"},
        "saved_for_backward_bytes": {"u": B * H * L * 2, "k_f": H * N * 4, "spectra (save_spectrum)": npair * N * 4},
        "peak_measured": peaks,
    })
    if strong is not None:
        # N > 1: the contract value is the FIXED problem (strong), the weak-scaled job rides beside it
        out["weak"] = {"value": seq_s, "unit": "seq/s", "ms_per_step": sec_per_step * 1e3, "scaling": "weak", "heads_per_rank": H}
        out["kernel_ms_scaling"] = "weak"      # kernel_ms / roofline objects below time the full per-GPU shape (768 heads on this rank)
    if strong_rows:
        out["strong_rows"] = strong_rows
    if world == 1 and not args.no_sweep:
        # the rest of the BASELINE metric, timed in this same process with HIP events (benchmarks/sweep.py): the other
        # configs and the L = 1K .. 1M sweep at B=16 H=768 (fwd / bwd ms at module level, incl. k -> k_f and dk)
        del u, k, dout, ud, kd, kf, ws, dk, dk_du, y_buf
        torch.cuda.empty_cache()
        from benchmarks import sweep as SW
        keep = ("row", "fft", "L", "H_run", "rescaled", "fwd_ms", "bwd_ms", "fwd_ms_min", "bwd_ms_min", "fwd_infer_ms", "timing", "seq_per_s", "tflops_fft_equiv", "fwd_alg_GBs",
                "bwd_alg_GBs", "fwd_GBs", "bwd_GBs", "fwd_hbm_frac", "bwd_hbm_frac", "peak_mem_bytes", "graph_step_ms", "fft_run", "fwd_ms_seqlen_points", "bwd_ms_seqlen_points")
        out["configs"] = [{kk: r[kk] for kk in keep if kk in r} for r in SW.config_rows()]
        # peak memory of the headline config (module level: save_spectrum on / off, inference forward, torch.fft form)
        out["peak_mem_bytes"] = out["configs"][0].get("peak_mem_bytes")
        out["sweep"] = [{kk: r[kk] for kk in keep if kk in r} for r in SW.sweep_rows()]
        out["sweep_gated"] = [{kk: r[kk] for kk in keep if kk in r} for r in SW.sweep_gated_rows()]
        # the reference's published table (gated forward, fp16, L = N, scaled to B=64 x H=768; 1 x H100-SXM, README.md:224-230)
        out["readme_table"] = list(SW.readme_rows())
    if world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
    emit(out, os.path.join(ROOT, "bench_out", "bench_full.json"))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
