"""Rotated pair loops of the plain-row kernels of fft 32768 at L <= N/2 on the GPU (csrc/ffc_body.h Body::outer_jobs ROT: the next pair's
rows are written to E behind phase C; csrc/ffc_modes.h Modes::bwd ROT: the next pair's row copies are finished behind phase C with a
counted wait that leaves the du stores in flight).  The default route against tuning flag 512 (the direct-store kernels with the run-time
arms and the earlier loop order), bit for bit: the rotation moves instructions and changes no arithmetic.

A wait that is too lax would let phase A read E rows that a copy has not reached yet: that shows up as a mismatch, not as a fault.  Every
case therefore runs three times in one process on fresh random inputs and is compared each time.  This is a parity check of the kernels
as they run in use.

Shapes (B, H, L).  SMALL is the simulator's set (tests/test_pair_loop_rotation_sim.py): one pair / one back edge / an odd batch with three
back edges, a tail inside a row, dead rows, more than one head.  On the GPU the launch rule (ffc_choose_chunks) spreads the pairs of
so few heads over the chip, one pair per workgroup: these cases run the prologues alone.  A workgroup loops over several pairs when there
are at least as many heads as workgroup slots, so WIDE repeats the properties at H = 512 (all pairs of a head in one workgroup, forward
and backward) and H = 256 with B = 8 (the backward in two chunks of two pairs per head: more than one chunk per head, one back edge each),
and adds L = 1032, where whole du / y store instructions of phase C have no active lane while the backward's wait counts them.
B16 H8 L16384 is the benchmark's batch at few heads, B16 H512 L16384 the benchmark's eight pairs per workgroup."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 32768
SMALL = [(B, H, L) for H in (1, 3) for B in (2, 4, 7) for L in (16384, 16376, 8200)]
WIDE = [(4, 512, 8200), (7, 512, 16376), (8, 256, 16384), (4, 512, 1032)]
ONCE = [(16, 8, 16384), (16, 512, 16384)]


def fresh(B, H, L, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.randn(B, H, L, device="cuda", generator=g).to(dtype)
    k = torch.randn(H, L, device="cuda", generator=g) * torch.exp(-0.01 * torch.arange(L, device="cuda")) / 4
    dout = torch.randn(B, H, L, device="cuda", generator=g).to(dtype)
    return u, k, dout


def module_step(u, k, dout, save):
    from flashfftconv import FlashFFTConv
    u, k = u.clone().requires_grad_(True), k.clone().requires_grad_(True)
    conv = FlashFFTConv(N, dtype=u.dtype).to("cuda")
    conv.save_spectrum = save
    y = conv(u, k)
    du, dk = torch.autograd.grad(y, (u, k), dout)
    torch.cuda.synchronize()
    return y.detach(), du, dk


def entry_step(u, k, dout, save):
    """the C entry points of tests/test_plain_rows_gpu.py: ffc_conv_fwd_z + ffc_conv_bwd_z, or the strided forward + recomputing backward"""
    from flashfftconv import FlashFFTConv, conv as C
    from tests.test_plain_rows_gpu import raw_step
    plan = FlashFFTConv(N, dtype=u.dtype).cuda()._get_plan(u.device)
    return raw_step(plan, C._kernel_fft(plan, k), u, dout, save)


def run_all(B, H, L, dtype, reps):
    out = []
    for rep in range(reps):
        u, k, dout = fresh(B, H, L, dtype, 7919 * rep + B * 100003 + H * 1009 + L)
        for save in (True, False):
            out.append((f"module save={save} rep {rep}", module_step(u, k, dout, save)))
            out.append((f"entry points save={save} rep {rep}", entry_step(u, k, dout, save)))
    return out


def compare(B, H, L, dtype, monkeypatch, reps):
    from flashfftconv import conv as C
    new = run_all(B, H, L, dtype, reps)
    monkeypatch.setenv("FFC_FLAGS", "512"); C.reload_env()      # (tuning flags are read when a plan is built or reloaded)
    try:
        old = run_all(B, H, L, dtype, reps)
    finally:
        monkeypatch.delenv("FFC_FLAGS"); C.reload_env()
    for (what, a), (_, b) in zip(new, old):
        for name, x, y in zip(("y", "du", "dk"), a, b):
            assert torch.isfinite(x.float()).all(), f"{what}: {name} not finite"
            assert torch.equal(x, y), f"{what}: {name}: default != flag 512, {int((x != y).sum())} of {x.numel()} elements"


@pytest.mark.parametrize("B,H,L", SMALL + WIDE)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_default_bit_identical_to_flag_512_three_times(B, H, L, dtype, monkeypatch):
    compare(B, H, L, dtype, monkeypatch, reps=3)


@pytest.mark.parametrize("B,H,L", ONCE)
def test_benchmark_batch_once(B, H, L, monkeypatch):
    compare(B, H, L, torch.bfloat16, monkeypatch, reps=1)
