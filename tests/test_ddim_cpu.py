"""DDIM sampling, host side: the timestep list against torch.linspace, argument checks, the DDIM CLI's flags."""
import math

import pytest
import torch

from ladiffcodec_amd import lib as L


@pytest.mark.parametrize("t_start", [1000, 100, 50, 37])
def test_ddim_times_match_torch_linspace(t_start):
    """ldc_ddim_times equals the reference's reversed(torch.linspace(-1, t_start - 1, S + 1).int()) for every S."""
    for S in range(1, t_start + 1):
        ref = list(reversed(torch.linspace(-1, t_start - 1, steps=S + 1).int().tolist()))
        assert L.ddim_times(t_start, S) == ref, (t_start, S)


@pytest.mark.parametrize("t_start,S", [(10, 11), (10, 0), (10, -3), (0, 1), (-5, 1)])
def test_ddim_times_refuses_bad_arguments(t_start, S):
    with pytest.raises(L.LdcError):
        L.ddim_times(t_start, S)


def test_ddim_times_null_output_refused():
    assert L.load().ldc_ddim_times(10, 5, None) == L.E_INVALID


@pytest.mark.parametrize("bad", [dict(eta=-0.1), dict(eta=1.5), dict(eta=math.nan), dict(eta=math.inf), dict(S=11), dict(S=0),
                                 dict(t_start=0), dict(t_start=1001)])
def test_ddim_sample_refuses_bad_arguments_before_any_gpu_work(bad):
    """Refused without touching a device (the GPU tests check the schedule arguments on a live context)."""
    a = dict(t_start=10, S=10, eta=0.0)
    a.update(bad)
    lib = L.load()
    rc = lib.ldc_ddim_sample(None, None, None, None, 0, a["t_start"], a["S"], a["eta"], 1, 80, 8, None)
    assert rc != 0
    rc = lib.ldc_decode_ddim(None, None, 1, 2560, a["t_start"], a["S"], a["eta"], None, 1, None, None, None, None, None)
    assert rc != 0


def test_ddim_exports_listed():
    for name in ("ldc_ddim_times", "ldc_ddim_sample", "ldc_decode_ddim"):
        assert name in L.EXPORTS and hasattr(L.load(), name)


def test_ddim_cli_parses_and_adds_exactly_two_flags(capsys):
    from ladiffcodec_amd import sample, sample_ddim
    base = {a.dest for a in sample.build_parser()._actions}
    mine = {a.dest for a in sample_ddim.build_parser()._actions}
    assert mine - base == {"ddim_steps", "ddim_eta"} and base <= mine
    a = sample_ddim.build_parser().parse_args([])
    assert a.ddim_steps == 10 and a.ddim_eta == 0.0 and a.midway_t == 100
    s = sample_ddim.sampler_from_args(a)
    assert (s.t_start, s.n_steps, s.eta, s.draws) == (100, 10, 0.0, 10)
    a = sample_ddim.build_parser().parse_args(["--midway_t", "20", "--ddim_steps", "6", "--ddim_eta", "0.5"])
    s = sample_ddim.sampler_from_args(a)
    assert (s.t_start, s.n_steps, s.eta) == (20, 6, 0.5)
    for argv in (["--midway_t", "5", "--ddim_steps", "6"], ["--ddim_eta", "1.5"], ["--ddim_steps", "0"]):
        with pytest.raises(SystemExit):
            sample_ddim.sampler_from_args(sample_ddim.build_parser().parse_args(argv))
    with pytest.raises(SystemExit) as ex:
        sample_ddim.build_parser().parse_args(["--help"])
    assert ex.value.code == 0
    assert "--ddim_steps" in capsys.readouterr().out


def test_ddim_cli_help_as_a_module():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "ladiffcodec_amd.sample_ddim", "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--ddim_eta" in r.stdout and "--midway_t" in r.stdout


def test_ddim_sampler_routes_to_decode_ddim_through_decode_with_retry():
    """decode_with_retry with a DdimSampler calls Engine.decode_ddim with (t_start, steps, eta); without one, Engine.decode."""
    from ladiffcodec_amd import sample

    class Stub:
        def __init__(self):
            self.calls = []

        def decode(self, batch, n_steps, noise=None, per_item=False):
            self.calls.append(("ddpm", n_steps, per_item))
            return batch

        def decode_ddim(self, batch, t_start, n_steps, eta=0.0, noise=None, per_item=False, want_stages=False):
            self.calls.append(("ddim", t_start, n_steps, eta, per_item))
            return batch

    e = Stub()
    sample.decode_with_retry(e, 1, 7, None, True)
    sample.decode_with_retry(e, 1, 7, None, False, sample.DdimSampler(50, 7, 0.25))
    assert e.calls == [("ddpm", 7, True), ("ddim", 50, 7, 0.25, False)]
