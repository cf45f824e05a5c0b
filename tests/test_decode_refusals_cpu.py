"""Which refusal a decode or sampler entry gives to a NULL context, in which order and with which text: every (return code,
ldc_last_error()) pair of the fixed list in tests/decode_refusals.py against tests/golden/decode_refusals.json, the table recorded from
the library as it stood when the list was written, in front of any rework of the decode entries.  One call per argument of every
context-free check of an entry, one per adjacent pair of its checks with both bad (the earlier check wins), one with everything good
(it stops at `null ctx`)."""
import pytest

import decode_refusals as DR
from ladiffcodec_amd import lib as L

CALLS = dict(DR.cpu_calls())
TABLE = DR.load_table()["cpu"]
ENTRIES = ("ldc_decode", "ldc_decode_ddim", "ldc_decode_ragged", "ldc_decode_codes", "ldc_decode_codes_ddim", "ldc_decode_codes_ragged",
           "ldc_decode_seeded", "ldc_decode_codes_seeded", "ldc_decode_dpm", "ldc_decode_ragged_dpm", "ldc_decode_codes_dpm",
           "ldc_decode_windows", "ldc_decode_ddim_windows", "ldc_decode_dpm_windows", "ldc_decode_codes_windows",
           "ldc_decode_codes_dpm_windows", "ldc_decode_windows_group", "ldc_get_cond_ragged", "ldc_sample_windows_group",
           "ldc_denoise_windows", "ldc_ddim_sample_windows", "ldc_dpm_sample_windows", "ldc_denoise", "ldc_ddim_sample", "ldc_dpm_sample",
           "ldc_sample_seeded")


def test_the_list_covers_every_entry():
    assert {e for e in L.EXPORTS if e.startswith("ldc_decode")} <= set(ENTRIES)
    fns = {fn.__name__ for _, fn, _, _ in DR.CPU_ENTRIES}
    assert fns == {"_" + e[len("ldc_"):] for e in ENTRIES}
    assert len(CALLS) == len(DR.cpu_calls())          # (no id twice)
    assert sorted(TABLE) == sorted(CALLS)


@pytest.mark.parametrize("name", list(CALLS))
def test_refusal_without_context(name):
    rc, msg = DR.run([(name, CALLS[name])])[name]
    assert [rc, msg] == TABLE[name]
    assert rc != 0
    if name.endswith(":good") or name.endswith(":all_bad"):
        assert (rc, msg) == (L.E_INVALID, "null ctx")
    else:
        assert msg != "null ctx"
