"""DPM-Solver++(2M) sampling, host side: the schedule table against the Python restatement (tests/dpm_restatement.py), argument
checks on every entry point with a NULL context, the CLI flags and the sampler routing."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from ladiffcodec_amd import lib as L
from helpers import main_sd_np
import dpm_restatement as R

ENTRIES = ("ldc_dpm_schedule", "ldc_dpm_sample", "ldc_decode_dpm", "ldc_decode_codes_dpm", "ldc_decode_ragged_dpm")
CASES = [(1000, 1000), (100, 10), (40, 8), (37, 5), (10, 10), (1, 1)]


def tables():
    sd = main_sd_np("r84")
    return sd["diffusion.sqrt_recip_alphas_cumprod"], sd["diffusion.sqrt_recipm1_alphas_cumprod"]


def test_dpm_exports_listed_and_bound():
    lib = L.load()
    for name in ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int


@pytest.mark.parametrize("t_start,S", CASES)
def test_dpm_schedule_matches_the_restatement(t_start, S):
    """t exactly; coefficients to relative 1e-6: both sides are double arithmetic on the same float32 tables, rounded once to float."""
    rec, recm1 = tables()
    t_ref, c_ref = R.dpm_table(rec, recm1, t_start, S)
    t_got, c_got = L.dpm_schedule(rec, recm1, t_start, S)
    assert t_got.tolist() == t_ref.tolist() == L.ddim_times(t_start, S)[:-1]
    assert c_got.shape == (S, 3) and c_got.dtype == np.float32
    err = np.abs(c_got.astype(np.float64) - c_ref) / np.maximum(np.abs(c_ref), 1e-300)
    err[c_ref == 0] = np.abs(c_got[c_ref == 0])
    print(f"dpm schedule ({t_start},{S}): largest relative coefficient error {err.max():.3e}")
    assert err.max() <= 1e-6, (t_start, S, err.max())
    # structure: no history on row 0, the final row is x <- x0, every other row is a genuine second-order row
    assert c_got[0, 2] == 0.0
    assert c_got[-1].tolist() == [0.0, 1.0, 0.0]
    if S > 2:
        mid = c_got[1:-1]
        assert (mid[:, 0] > 0).all() and (mid[:, 0] < 1).all() and (mid[:, 1] > 0).all() and (mid[:, 2] < 0).all()
    if S > 1:
        assert 0 < c_got[0, 0] < 1 and c_got[0, 1] > 0


def test_dpm_schedule_single_step_is_the_final_row():
    rec, recm1 = tables()
    for t_start in (1, 40, 1000):
        t, c = L.dpm_schedule(rec, recm1, t_start, 1)
        assert t.tolist() == [t_start - 1] and c.tolist() == [[0.0, 1.0, 0.0]]


def _last_error():
    return L.load().ldc_last_error().decode()


@pytest.mark.parametrize("t_start,S,named", [(0, 1, "0"), (-3, 1, "-3"), (1001, 5, "1001"), (10, 0, "0"), (10, 11, "11"), (10, -2, "-2")])
def test_dpm_schedule_refuses_bad_arguments(t_start, S, named):
    rec, recm1 = tables()
    with pytest.raises(L.LdcError) as ei:
        L.dpm_schedule(rec, recm1, t_start, S)
    assert ei.value.code == L.E_INVALID and named in str(ei.value)


def test_dpm_schedule_refuses_null_pointers():
    lib = L.load()
    rec, recm1 = (np.ascontiguousarray(a, dtype=np.float32) for a in tables())
    t_out, coef = (C.c_int * 4)(), (C.c_float * 12)()
    good = [rec.ctypes.data, recm1.ctypes.data, 1000, 40, 4, t_out, coef]
    assert lib.ldc_dpm_schedule(*good) == 0
    for k in (0, 1, 5, 6):
        a = list(good)
        a[k] = None
        assert lib.ldc_dpm_schedule(*a) == L.E_INVALID, k
    a = list(good)
    a[2] = 0
    assert lib.ldc_dpm_schedule(*a) == L.E_INVALID


@pytest.mark.parametrize("bad,named", [(dict(t_start=0), "t_start 0"), (dict(t_start=-1), "t_start -1"), (dict(S=0), "n_steps 0"),
                                       (dict(S=11), "n_steps 11"), (dict(t_start=1001, S=1001), None), (dict(), None)])
def test_dpm_entries_refuse_before_any_gpu_work_with_a_null_context(bad, named):
    """Every entry point with a NULL context: bad t_start / n_steps are refused with the value named; good ones (and a t_start
    that only a context's timesteps can refuse) stop at the NULL context.  Nothing touches a device."""
    a = dict(t_start=10, S=10)
    a.update(bad)
    lib = L.load()
    lens = (C.c_int32 * 1)(2560)
    calls = [lambda: lib.ldc_dpm_sample(None, None, None, a["t_start"], a["S"], 1, 80, 8, None),
             lambda: lib.ldc_decode_dpm(None, None, 1, 2560, a["t_start"], a["S"], 1, None, None, None, None, None),
             lambda: lib.ldc_decode_ragged_dpm(None, None, lens, 1, 2560, a["t_start"], a["S"], None, None, None, None, None),
             lambda: lib.ldc_decode_codes_dpm(None, None, None, 0, 10, 4, 1, 8, a["t_start"], a["S"], 1, None, None, None, None)]
    for k, call in enumerate(calls):
        assert call() != 0, k
        if named is not None and k < 3:        # (decode_codes checks its code arguments first: both sources are null here)
            assert named in _last_error(), (k, _last_error())


def test_dpm_entries_refuse_null_tensors_with_a_null_context():
    lib = L.load()
    assert lib.ldc_dpm_sample(None, None, None, 10, 5, 1, 80, 8, None) == L.E_INVALID
    assert lib.ldc_decode_dpm(None, None, 1, 2560, 10, 5, 1, None, None, None, None, None) == L.E_INVALID
    assert lib.ldc_decode_ragged_dpm(None, None, None, 1, 2560, 10, 5, None, None, None, None, None) == L.E_INVALID
    assert lib.ldc_decode_codes_dpm(None, None, None, 0, 10, 4, 1, 8, 10, 5, 1, None, None, None, None) == L.E_INVALID


def test_dpm_cli_parses_and_adds_exactly_one_flag(capsys):
    from ladiffcodec_amd import sample, sample_dpm
    base = {a.dest for a in sample.build_parser()._actions}
    mine = {a.dest for a in sample_dpm.build_parser()._actions}
    assert mine - base == {"dpm_steps"} and base <= mine
    a = sample_dpm.build_parser().parse_args([])
    assert a.dpm_steps == 10 and a.midway_t == 100
    s = sample_dpm.sampler_from_args(a)
    assert isinstance(s, sample.DpmSampler) and (s.t_start, s.n_steps, s.draws) == (100, 10, 0)
    s = sample_dpm.sampler_from_args(sample_dpm.build_parser().parse_args(["--midway_t", "20", "--dpm_steps", "6"]))
    assert (s.t_start, s.n_steps) == (20, 6)
    for argv in (["--dpm_steps", "0"], ["--midway_t", "5", "--dpm_steps", "6"], ["--dpm_steps", "-1"]):
        with pytest.raises(SystemExit):
            sample_dpm.sampler_from_args(sample_dpm.build_parser().parse_args(argv))
    with pytest.raises(SystemExit) as ex:
        sample_dpm.build_parser().parse_args(["--help"])
    assert ex.value.code == 0
    assert "--dpm_steps" in capsys.readouterr().out


def test_dpm_cli_help_as_a_module():
    r = subprocess.run([sys.executable, "-m", "ladiffcodec_amd.sample_dpm", "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--dpm_steps" in r.stdout and "--midway_t" in r.stdout


class Stub:
    def __init__(self):
        self.calls = []

    def decode_dpm(self, batch, t_start, n_steps, per_item=False, want_stages=False):
        self.calls.append(("dpm", t_start, n_steps, per_item, want_stages))
        return batch

    def decode_ragged_dpm(self, wav, lengths, t_start, n_steps, want_stages=False):
        self.calls.append(("ragged_dpm", list(lengths), t_start, n_steps))
        return wav

    def decode_codes_dpm(self, **kw):
        self.calls.append(("codes_dpm", sorted(kw)))
        return 0


def test_dpm_sampler_routes_through_decode_with_retry_and_passes_no_noise():
    """decode_with_retry with a DpmSampler calls Engine.decode_dpm(t_start, steps); the stub's signatures take no noise, so one
    passed on would be a TypeError.  A RaggedBatch goes to decode_ragged_dpm; codes to decode_codes_dpm; ragged codes are refused."""
    from ladiffcodec_amd import sample
    e = Stub()
    s = sample.DpmSampler(50, 7)
    assert s.draws == 0
    sample.decode_with_retry(e, 1, 7, "a tape that must not travel", False, s)
    sample.decode_with_retry(e, sample.RaggedBatch(2, [2560, 5120]), 7, None, True, s)
    cs = sample.CodesSampler(s)
    assert cs.draws == 0
    sample.decode_with_retry(e, sample.CodesBatch(packed=3, n_q=4, F=8), 7, None, True, cs)
    assert e.calls == [("dpm", 50, 7, False, False), ("ragged_dpm", [2560, 5120], 50, 7),
                       ("codes_dpm", ["F", "bits", "codes", "n_q", "n_steps", "packed", "per_item", "t_start", "want_stages"])]
    with pytest.raises(ValueError, match="ragged"):
        cs(e, sample.RaggedCodesBatch(3, 4, [8, 16]), None, True)


def test_decompress_takes_dpm_steps_and_refuses_both_samplers():
    from ladiffcodec_amd import decompress, sample
    base = ["--midway_t", "30"]
    p = decompress.build_parser()
    assert decompress.dpm_steps(p.parse_args(base)) == 0
    assert isinstance(decompress.sampler_from_args(p.parse_args(base + ["--dpm_steps", "0"])).inner, sample.DdpmSampler)
    s = decompress.sampler_from_args(p.parse_args(base + ["--dpm_steps", "6"]))
    assert isinstance(s, sample.CodesSampler) and isinstance(s.inner, sample.DpmSampler) and (s.inner.t_start, s.inner.n_steps) == (30, 6)
    for extra in (["--dpm_steps", "6", "--ddim_steps", "5"], ["--dpm_steps", "31"], ["--dpm_steps", "-2"], ["--dpm_steps", "6", "--ragged"]):
        with pytest.raises(SystemExit):
            decompress.sampler_from_args(p.parse_args(base + extra))
    assert "--dpm_steps" in p.format_help()
