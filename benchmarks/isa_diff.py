"""Kernel-by-kernel comparison of the gfx950 device assembly of two source trees (for refactors that must not change device code; no GPU needed).

    python benchmarks/isa_diff.py <A> <B>        A, B: a source tree (the directory that holds flash-fft-conv_amd/ and include/) or a git revision

compiles every .hip unit of build.py's HIP_SRCS for both sides with the flags of build.py (isa_view.py's list, checked to be the same) plus `--cuda-device-only -S` (at most 16
compiles at a time), drops comments, .file / .ident / .loc lines and the __hip_cuid_* symbol, splits the text at the `_Z...:` labels up
to the end label of each kernel, and prints per unit: kernels total, kernels identical, and the names of those that differ.  Exit status 1 if any
differ.  The assembly is cached under /tmp/ffc_isa/diff/, keyed by the preprocessed text of the unit, so a unit that an edit does not reach
is compiled once for both sides.  A full run is several minutes of compiling, which is why this is a script and not a test."""
import hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "flash-fft-conv_amd"))
from isa_view import FLAGS, ROOT            # noqa: E402
from build import HIP_FLAGS, HIP_SRCS       # noqa: E402

assert FLAGS == HIP_FLAGS, "isa_view.FLAGS is no longer what build.py compiles with: the comparison would not be of the shipped code"

CACHE = "/tmp/ffc_isa/diff"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = [f for f in HIP_SRCS if f.endswith(".hip")]
JOBS = min(16, os.cpu_count() or 4)


def tree(arg):
    """A directory as it is; a git revision as an export of its two source directories."""
    if os.path.isdir(os.path.join(arg, "flash-fft-conv_amd", "csrc")):
        return os.path.abspath(arg)
    sha = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--verify", arg + "^{commit}"], text=True).strip()
    d = os.path.join(CACHE, "rev_" + sha)
    if not os.path.isdir(d):
        tmp = tempfile.mkdtemp(dir=CACHE)
        tar = subprocess.run(["git", "-C", ROOT, "archive", sha, "flash-fft-conv_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        os.rename(tmp, d)
    return d


def command(root, unit):
    return [HIPCC] + FLAGS + ["--cuda-device-only", "-x", "hip", os.path.join(root, "flash-fft-conv_amd", "csrc", unit)]


def cache_path(root, unit):
    pre = subprocess.run(command(root, unit) + ["-E", "-P", "-o", "-"], check=True, capture_output=True).stdout
    return os.path.join(CACHE, hashlib.sha256(" ".join(FLAGS).encode() + pre).hexdigest()[:24] + "_" + os.path.splitext(unit)[0] + ".s")


def compile_to(asm, root, unit):
    if not os.path.exists(asm):
        subprocess.run(command(root, unit) + ["-S", "-o", asm + ".part"], check=True)
        os.rename(asm + ".part", asm)


def kernels(asm):
    """{mangled name: normalised lines from its label to its .Lfunc_end label} (a kernel may hold several s_endpgm)."""
    out, name, body = {}, None, []
    with open(asm) as fh:
        for line in fh:
            t = line.split(";")[0].rstrip()
            if not t.strip() or re.match(r"\s*\.(file|ident|loc)\b", t) or "__hip_cuid_" in t:
                continue
            m = re.match(r"^(_Z\w+):", t)
            if m and name is not None:
                raise RuntimeError(f"{asm}: {name} has no end label before {m.group(1)}")
            if m:
                name, body = m.group(1), []
            if name is not None:
                if t.startswith(".Lfunc_end"):
                    out[name], name = body, None
                else:
                    body.append(t)
    if name is not None:
        raise RuntimeError(f"{asm}: {name} has no end label")
    return out


if __name__ == "__main__":
    os.makedirs(CACHE, exist_ok=True)
    a, b = tree(sys.argv[1]), tree(sys.argv[2])
    print(f"A = {sys.argv[1]}   B = {sys.argv[2]}   flags: {' '.join(FLAGS)}")
    sides = [(r, u) for r in (a, b) for u in UNITS]
    with ThreadPoolExecutor(max_workers=JOBS) as ex:
        asm = dict(zip(sides, ex.map(lambda ru: cache_path(*ru), sides)))
        todo = {asm[ru]: ru for ru in sides}                       # one compile per distinct preprocessed text
        list(ex.map(lambda item: compile_to(item[0], *item[1]), sorted(todo.items(), key=lambda item: "ffc_k_" not in item[0])))
    differ = 0
    for u in UNITS:
        ka, kb = kernels(asm[a, u]), kernels(asm[b, u])
        bad = sorted(n for n in set(ka) | set(kb) if ka.get(n) != kb.get(n))
        differ += len(bad)
        print(f"{u}: kernels {len(set(ka) | set(kb))}, identical {len(set(ka) | set(kb)) - len(bad)}" + "".join("\n    differs: " + n for n in bad))
    print("every kernel identical" if not differ else f"{differ} kernels differ")
    sys.exit(1 if differ else 0)
