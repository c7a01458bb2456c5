"""overlap_save="direct" without a GPU: the module's state format, the batch-split rule of the step launches and the refusals of the C entry
points, which check their ranges before they touch a device."""
import copy
import pickle

import pytest


def test_module_state_len_pickle_deepcopy():
    from flashfftconv import PartialFFTConv
    mod = PartialFFTConv(64, overlap_save="direct")
    assert mod.state_len == 2048
    for other in (pickle.loads(pickle.dumps(mod)), copy.deepcopy(mod)):
        assert (other.N_partial, other.overlap_save, other.state_len) == (64, "direct", 2048)


# grid = H x slices on 256 CUs: slices = ceil(B / ceil(B / n)), n = max(1, min(ceil(512 / H), B // 4))
@pytest.mark.parametrize("B,H,slices", [(3, 2, 1), (7, 2, 1), (8, 2, 2), (9, 2, 2), (10, 1, 2), (64, 64, 8), (64, 768, 1), (2, 768, 1),
                                        (1024, 1, 256), (4096, 1, 512)])
def test_batch_split_rule(B, H, slices):
    from flashfftconv import _lib
    assert _lib.lib().ffc_partial_step_split(B, H, 256) == slices


@pytest.mark.parametrize("L,S,taps,msg", [(0, 2048, 64, "L must"), (65, 2048, 64, "L must"), (1, 2048, 0, "taps must"), (1, 16384, 16385, "taps must"),
                                          (1, 1024, 64, "S must"), (1, 3000, 64, "S must"), (1, 32768, 64, "S must"), (1, 2048, 2049, "exceed")])
def test_entry_points_refuse_out_of_range_sizes(L, S, taps, msg):
    from flashfftconv import _lib
    lib = _lib.lib()
    assert lib.ffc_partial_step_fwd(0, *[None] * 9, 3, 2, L, S, 20000, taps, None) != 0
    assert msg in lib.ffc_last_error().decode()
    assert lib.ffc_partial_step_bwd(0, *[None] * 13, 1, 3, 2, L, S, 20000, taps, None) != 0
    assert msg in lib.ffc_last_error().decode()
