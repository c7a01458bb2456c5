"""The build switches that select between two forms of the same arithmetic must not change a single bit (round 4's load-scheduling work:
FFC_GATE_BATCH = 0 is the one-load-at-a-time form of the gated rows, FFC_RP_HOIST = 0 the multi-pass rows with the access-width switch
inside every load).  One simulator build with every switch flipped, compared with the
default simulator on forward, backward and the spectrum-saving pair of single-tile, fused and multi-pass sizes, gated and ragged."""
import ctypes, hashlib, os, subprocess, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "flash-fft-conv_amd")
# round 5: FFC_OUTER_QUAD = 0 is the tile-pair form of phases A / C (4-byte LDS accesses), FFC_RP_FASTK = 0 the multi-pass backward with the
# run-time access-width switch in every row access (the default launches a 16-byte-only instantiation on aligned tensors)
# FFC_PK_GATE = 0: fp16 gate multiplies through fp32 (the packed fp16 multiply rounds the exact product once: the same bits)
# round 6: FFC_IP_MERGE = 0 is the fft-2048 forward with one row load / one read-modify-write of the output per PASS (the default keeps the pair's rows
# and the passes' sum in registers: one load, one store)
ALT_FLAGS = ["-DFFC_GATE_BATCH=0", "-DFFC_RP_HOIST=0", "-DFFC_OUTER_QUAD=0", "-DFFC_RP_FASTK=0", "-DFFC_PK_GATE=0", "-DFFC_IP_MERGE=0"]


def _variant_sim(name, flags, so_name="libffcsim.so"):
    """a simulator built with `flags`, in-tree under lib/variants/<name>/ and reused while no source is newer"""
    d = os.path.join(PKG, "lib", "variants", name)
    so = os.path.join(d, so_name)
    csrc = os.path.join(PKG, "csrc")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        os.makedirs(d, exist_ok=True)
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-pthread"] + list(flags) + ["-o", so,
                               os.path.join(csrc, "ffc_sim.cpp"), os.path.join(csrc, "ffc_plan.cpp")])
    return so


def _alt_sim():
    return _variant_sim("sim_alt", ALT_FLAGS)


CASES = [(256, 200, 5, 2, 1, True), (1024, 1024, 3, 2, 0, True), (2048, 1024, 4, 1, 0, True), (2048, 1000, 3, 2, 1, False), (2048, 2048, 2, 1, 0, True), (4096, 2048, 5, 1, 1, True),
         (32768, 16384, 3, 1, 0, False), (32768, 9000, 2, 1, 0, True), (65536, 32768, 3, 1, 0, True), (65536, 40004, 1, 1, 1, False),
         (65536, 65536, 2, 1, 0, True), (131072, 65536, 1, 1, 0, False), (8192, 4096, 3, 1, 1, True), (16384, 16384, 2, 1, 0, False)]
_SCRIPT = r'''
import sys, hashlib, numpy as np
sys.path[:0] = [%r, %r, %r]
import simlib as S
dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]
for (N, L, B, H, dt, gated) in %r:
    rng = np.random.default_rng(N + L)
    u, d, g1, g2 = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(4))
    k = (rng.standard_normal((H, L)) * 0.1).astype(np.float32)
    kf = S.sim_kernel_fft(N, dt, k)
    pre = S.to_bits(g1, dt) if gated else None; post = S.to_bits(g2, dt) if gated else None
    out = [dig(kf), dig(S.sim_conv_fwd(N, dt, S.to_bits(u, dt), kf, pre, post))]
    du, dpre, dk = S.sim_bwd(N, dt, S.to_bits(d, dt), S.to_bits(u, dt), kf, L, pre, post, 1)
    out += [dig(du), dig(dk)] + ([dig(dpre)] if gated else [])
    out += [dig(x) for x in S.sim_fwd_bwd_z(N, dt, S.to_bits(u, dt), S.to_bits(d, dt), kf, pre, post) if x is not None]
    print(N, L, B, H, dt, gated, " ".join(out), flush=True)
'''


def _digests(sim_lib):
    env = dict(os.environ)
    if sim_lib:
        env["FFC_SIM_LIB"] = sim_lib
    else:
        env.pop("FFC_SIM_LIB", None)
    src = _SCRIPT % (HERE, PKG, os.path.dirname(HERE), CASES)
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()


def test_build_switches_do_not_change_a_bit():
    base = _digests(None)
    alt = _digests(_alt_sim())
    assert len(base) == len(CASES) == len(alt)
    for a, b in zip(base, alt):
        assert a == b, (a, b)


# ---------------------------------------------------------------- FFC_FOLD_TW (round 5; measured, not adopted: DESIGN.md section 8)
_FOLD_SCRIPT = r'''
import sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import simlib as S
from oracle import ref_fft_conv as O
rel = lambda a, b: np.linalg.norm(np.asarray(a).astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30)
q = lambda x, dt: S.from_bits(S.to_bits(x, dt), dt).astype(np.float64)
for (N, L, B, H, gated, dt) in [(32768, 16384, 3, 1, False, 0), (32768, 32768, 2, 1, False, 0), (32768, 9000, 2, 1, True, 0), (32768, 16384, 2, 1, True, 1)]:
    rng = np.random.default_rng(N + L + B)
    u, d, g1, g2 = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(4))
    k = (rng.standard_normal((H, L)) * 0.1).astype(np.float32)
    kf = S.sim_kernel_fft(N, dt, k)
    pre = S.to_bits(g1, dt) if gated else None; post = S.to_bits(g2, dt) if gated else None
    y, du, dpre, dpost, ws = S.sim_fwd_bwd_z(N, dt, S.to_bits(u, dt), S.to_bits(d, dt), kf, pre, post, 1, flags=0)
    nt, _, _, _ = S.plan_info(N, dt)
    dk = np.full((H, L), np.nan, np.float32)
    assert S.lib().ffcsim_kernel_ifft_grad(N, dt, S.p(ws), ws.size // (H * nt * 2048), H, L, S.p(dk)) == 0
    ref = O.ref_fft_conv_gated(q(u, dt), k, q(g1, dt), q(g2, dt), N, dtype=("bf16", "fp16")[dt]) if gated else O.ref_fft_conv(q(u, dt), k, N)
    r = O.ref_grads(q(u, dt), k, q(d, dt), N, q(g1, dt), q(g2, dt)) if gated else O.ref_grads(q(u, dt), k, q(d, dt), N)
    print(rel(S.from_bits(y, dt), ref), rel(S.from_bits(du, dt), r[0]), rel(dk, r[1]), dt, flush=True)
'''


def test_folded_outer_twiddle_variant_matches_the_oracle():
    """-DFFC_FOLD_TW=2: the outer twiddle folded into per-tile inner DFT matrices also at fft 32768 (forward kernels + the saved-spectra backward;
    the product folds the forward of fft 16384 only).  The variant simulator is built on first use (a few minutes of g++ -O0) under
    lib/variants/sim_fold/ and reused while no source is newer."""
    so = _variant_sim("sim_fold", ["-DFFC_FOLD_TW=2"], "libffcsim2.so")
    env = dict(os.environ, FFC_SIM_LIB=so)
    r = subprocess.run([sys.executable, "-c", _FOLD_SCRIPT % (HERE, PKG, os.path.dirname(HERE))], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.strip().splitlines()]
    assert len(rows) == 4
    for y, du, dk, dt in rows:
        tol = 1.2e-2 if dt == "0" else 1.5e-3
        assert float(y) < tol and float(du) < tol and float(dk) < 1.8e-2, (y, du, dk, dt)


# ---------------------------------------------------------------- FFC_BIG_CHAIN=0 (csrc/ffc_big.h): the HBM levels with one sin / cos pair per element
# instead of the twiddle chains down the rows -- the documented A/B build of round 5.  Another rounding sequence of the same values, so no bit identity:
# the oracle's gate, and the default simulator to rounding.
NOCHAIN_CASES = [(65536, ((16,), 4096), 30000, False, True), (131072, ((32,), 4096), 131072, True, True),
                 (262144, ((64,), 4096), 131072, False, True), (262144, ((64,), 4096), 131072, False, False),
                 (524288, ((128,), 4096), 100004, True, True), (524288, ((128,), 4096), 100004, True, False)]      # N, fac, L, gated, one_launch
_NOCHAIN_SCRIPT = r'''
import sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import simlib as S
res = {}
for ci, (N, fac, L, gated, one_launch) in enumerate(%r):
    for B in (1, 2):          # a batch of one: the half-row form (BigArgs::half); two rows: the pair form, all rows
        rng = np.random.default_rng(N + L + B)
        dt, H = 0, 2
        ops = S.SimOps(); ops.half = B == 1; ops.one_launch = one_launch
        u, g1, g2, d = (rng.standard_normal((B, H, L)).astype(np.float32) for _ in range(4))
        k = (rng.standard_normal((H, L)) * 0.05).astype(np.float32)
        ub, g1b, g2b, db = (S.to_bits(x, dt) for x in (u, g1, g2, d))
        r = S.big_forward_and_dk(ops, dt, N, fac, ub, db, k, g1b if gated else None, g2b if gated else None)      # (shared with tests/test_sim_kernels.py)
        res["out_%%d_%%d" %% (ci, B)] = S.from_bits(r["out"], dt); res["dk_%%d_%%d" %% (ci, B)] = r["dk"]
        res["in_%%d_%%d" %% (ci, B)] = np.stack([u, g1, g2, d]); res["k_%%d_%%d" %% (ci, B)] = k
        print(ci, B, flush=True)
np.savez(sys.argv[1], **res)
'''


def _nochain_runs(libs_and_paths):
    """the child script once per (simulator library or None = the default build, result file), side by side"""
    src = _NOCHAIN_SCRIPT % (HERE, PKG, os.path.dirname(HERE), NOCHAIN_CASES)
    procs = []
    for sim_lib, path in libs_and_paths:
        env = dict(os.environ)
        env.pop("FFC_SIM_LIB", None)
        if sim_lib:
            env["FFC_SIM_LIB"] = sim_lib
        procs.append(subprocess.Popen([sys.executable, "-c", src, path], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    for pr in procs:
        _, err = pr.communicate(timeout=1800)
        assert pr.returncode == 0, err[-2000:]
    return [np.load(path) for _, path in libs_and_paths]


def test_per_element_twiddle_variant_matches_the_oracle(tmp_path):
    """-DFFC_BIG_CHAIN=0: the per-element twiddle branches of the inverse level (BigBody::stage<false>, the one-launch / per-pass inverse of the factors
    64 and 128) have to weight the stored rows of the half-row form like the chained form does (half_weight: 2, or 1 for the rows k0 = 0 and K / 2) --
    without it the mirror rows are dropped and forward and dk of every batch of one are wrong by ~0.7 with no error raised.  Forward and dk of the
    simulator's levels, half rows (B = 1) and all rows (B = 2), against the float64 oracle and against the default build."""
    from oracle import ref_fft_conv as O
    import simlib as S
    rel = lambda a, b: np.linalg.norm(np.asarray(a).astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30)
    q = lambda x: S.from_bits(S.to_bits(x, 0), 0).astype(np.float64)
    alt, base = _nochain_runs([(_variant_sim("sim_nochain", ["-DFFC_BIG_CHAIN=0"]), str(tmp_path / "nochain.npz")), (None, str(tmp_path / "default.npz"))])
    for ci, (N, fac, L, gated, one_launch) in enumerate(NOCHAIN_CASES):
        for B in (1, 2):
            u, g1, g2, d = base[f"in_{ci}_{B}"]
            k = base[f"k_{ci}_{B}"]
            ref = O.ref_fft_conv_gated(q(u), k, q(g1), q(g2), N, dtype="bf16") if gated else O.ref_fft_conv(q(u), k, N)
            _, dkref = O.ref_grads(q(u), k, q(d), N)
            for nm, want in (("out", ref), ("dk", dkref)):
                a, b = alt[f"{nm}_{ci}_{B}"], base[f"{nm}_{ci}_{B}"]
                what = f"fft {N} = {fac[0][0]} x {fac[1]}, B = {B}, one_launch = {one_launch}: {nm}"
                assert rel(b, want) < 1.5e-2, f"{what}: default build against the oracle {rel(b, want):.3e}"
                assert rel(a, want) < 1.5e-2, f"{what}: FFC_BIG_CHAIN=0 against the oracle {rel(a, want):.3e}"
                assert rel(a, b.astype(np.float64)) < 1e-2, f"{what}: FFC_BIG_CHAIN=0 against the default build {rel(a, b.astype(np.float64)):.3e}"


# ---------------------------------------------------------------- the rule of the code base: a compile-time switch exists only if a test builds its other form
def test_every_switch_is_documented():
    """The names introduced as `#ifndef FFC_X` / `#define FFC_X` in csrc/ are exactly the first column of the switch table of DESIGN.md section 7
    (each row there names the test that builds the switch's other form), and no name of the table's "removed" row is left in csrc/ or build.py."""
    import glob, re
    csrc = os.path.join(PKG, "csrc")
    files = [f for pat in ("*.h", "*.hip", "*.cpp") for f in glob.glob(os.path.join(csrc, pat))]
    text = {f: open(f).read() for f in files}
    defined = {m.group(1) for t in text.values() for m in re.finditer(r"^[ \t]*#[ \t]*ifndef[ \t]+(FFC_\w+)[^\n]*\n[ \t]*#[ \t]*define[ \t]+\1\b", t, re.M)}
    defined.discard("FFC_FN")
    design = open(os.path.join(os.path.dirname(HERE), "DESIGN.md")).read()
    sec = design[design.index("## 7. Build switches"):]
    rows = [l for l in sec[:sec.index("\n## 8.")].splitlines() if l.startswith("|")]
    assert rows[0].startswith("| switch |") and rows[1].startswith("|---"), rows[:2]
    documented, removed = set(), set()
    for row in rows[2:]:
        cell = row.split("|")[1]
        if cell.strip().startswith("(removed"):
            removed |= set(re.findall(r"`(FFC_\w+)`", cell))
            continue
        names = re.findall(r"`(\w+)`", cell)       # `FFC_X` (`_A`, `_B`) stands for FFC_X, FFC_X_A, FFC_X_B
        assert names and names[0].startswith("FFC_"), row
        documented |= {names[0]} | {names[0] + n for n in names[1:] if n.startswith("_")} | {n for n in names[1:] if n.startswith("FFC_")}
    assert defined == documented, (sorted(defined - documented), sorted(documented - defined))
    assert removed and not (removed & documented)
    text[os.path.join(PKG, "build.py")] = open(os.path.join(PKG, "build.py")).read()
    left = sorted((n, os.path.basename(f)) for f, t in text.items() for n in removed if re.search(r"\b%s\b" % n, t))
    assert not left, left
