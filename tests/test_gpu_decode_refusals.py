"""The refusals of the decode and sampler entries that need a live context (n_steps / t_start above `timesteps`, n_q above the codec's
layers, bits below the bins' need, T off the hops, ragged lengths off the quantum or above Tmax, packed_stride below the longest item, the
fp8 engine's ragged refusal, R above a window group's size, a group call that draws with neither tape nor seeds; and what the entries that
look at the context first refuse behind it: tensors, sizes, ddim_schedule's eta and n_steps, with their precedence): every (return code,
ldc_last_error()) pair of the fixed list in tests/decode_refusals.py against tests/golden/decode_refusals.json, recorded from the library
as it stood when the list was written, in front of any rework of the decode entries.  One engine on CASES["r84"] at B = 1 and T = one
ragged quantum (a second one with dtype fp8 for the fp8 line); every call is refused before any GPU work is queued (the buffers are real
all the same)."""
import pytest

import decode_refusals as DR
from gpu_common import engine

pytestmark = pytest.mark.gpu


def _check(got):
    want = DR.load_table()["gpu"]
    for name, pair in got.items():
        assert pair == want[name], name
        assert pair[0] != 0 and pair[1] != "null ctx", name


@pytest.fixture(scope="module")
def bufs():
    return DR.device_buffers()


def test_refusals_with_a_live_context(bufs):
    names = DR.gpu_names()
    assert len(set(names)) == len(names) and set(DR.load_table()["gpu"]) == set(names)
    _check(DR.run(DR.gpu_calls(bufs), engine("r84", "f32")._ctx))


def test_the_fp8_engine_refuses_ragged_batches(bufs):
    _check(DR.run(DR.fp8_calls(bufs), engine("r84", "fp8")._ctx))
