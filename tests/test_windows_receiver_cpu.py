"""Coupled windows for the receiver, without a GPU ("DPM-Solver++ windows and the receiver"): the identities of
the DPM restatement on the CPU oracle (W = 1 is dpm_sample at B = 1, bit for bit; overlap 0 is the batch of independent chunks), the
discrimination conditions the GPU tests rely on -- asserted here on the oracle alone --, the context-free refusals of the four new
entry points with a NULL context, and the CLIs' flag, sampler route and segment plan."""
import pytest
import torch

from ladiffcodec_amd import decompress, lib as L, sample, sample_dpm
from drift_tolerances import TOL
import dpm_restatement as D
import windows_dpm_restatement as WD
import windows_restatement as R

CASES = [("r84", 180, 80, 40), ("r8", 400, 160, 40)]
SCHEDULES = [(40, 8), (100, 12)]
NEW = ["ldc_dpm_sample_windows", "ldc_decode_dpm_windows", "ldc_decode_codes_windows", "ldc_decode_codes_dpm_windows"]


def _last_error():
    return L.load().ldc_last_error().decode()


def test_exports_listed_and_bound():
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTS and getattr(lib, name).argtypes, name


# ------------------------------------------------------------------------------------------------------ the restatement's identities
@pytest.mark.parametrize("t_start,S", SCHEDULES)
def test_one_window_is_dpm_sample_at_batch_one(t_start, S):
    s = R.inputs("r84", 80)
    ref = D.dpm_sample(s["sd"], s["u"], s["img"], s["cond"], t_start, S)
    for lw in (80, 160):                                                   # Ltot == Lw and Ltot < Lw: one window of Ltot frames
        got = WD.dpm_windows(s["sd"], s["u"], s["img"], s["cond"], t_start, S, lw, 40, s["up"])
        assert torch.equal(got, ref), (lw, float((got - ref).abs().max()))


def test_overlap_zero_is_the_batch_of_independent_chunks():
    s = R.inputs("r84", 240)
    got = WD.dpm_windows(s["sd"], s["u"], s["img"], s["cond"], 40, 8, 80, 0, s["up"])
    cut = lambda x, n: torch.cat([x[..., k * n:(k + 1) * n] for k in range(3)], dim=-3)      # noqa: E731  [1, C, 3 n] -> [3, C, n]
    ref = D.dpm_sample(s["sd"], s["u"], cut(s["img"], 80), cut(s["cond"], 8), 40, 8)
    assert torch.equal(got, torch.cat(list(ref[:, None]), dim=-1))
    # and the "end" mutant of an overlap-0 layout is the scheme itself: nothing couples the chunks
    end, _ = WD.dpm_windows(s["sd"], s["u"], s["img"], s["cond"], 40, 8, 80, 0, s["up"], mode="end")
    d = float((end - got).abs().max()) / float(got.abs().max())
    print(f"overlap 0: solo windows blended at the end against the coupled loop {d:.3e}")
    assert d < TOL["f32"]["chain_small"]


# --------------------------------------------------------------------------------------------------- what the GPU bars can tell apart
@pytest.mark.parametrize("t_start,S", SCHEDULES)
@pytest.mark.parametrize("tag,Ltot,Lw,O_", CASES)
def test_discrimination_conditions_on_the_oracle(tag, Ltot, Lw, O_, t_start, S):
    """The coupled DPM result differs from each mutant by at least 10 x the f32 chain bar: (a) windows solved independently and blended
    once at the end, (b) the first-order solver (b1 folded into b0), (c) DDIM windows at eta 0 on the same timesteps."""
    bar = TOL["f32"]["chain_small"]
    ref = WD.reference(tag, Ltot, Lw, O_, t_start, S)
    end, solo = WD.reference(tag, Ltot, Lw, O_, t_start, S, mode="end")
    first = WD.reference(tag, Ltot, Lw, O_, t_start, S, mode="first")
    ddim = WD.reference(tag, Ltot, Lw, O_, t_start, S, mode="ddim")
    m = float(ref.abs().max())
    d = {k: float((ref - v).abs().max()) / m for k, v in (("a", end), ("b", first), ("c", ddim))}
    print(f"{tag} ({t_start}, {S}): coupled DPM windows against (a) blended at the end {d['a']:.3e}, (b) first order {d['b']:.3e}, "
          f"(c) DDIM eta 0 {d['c']:.3e} (10 x bar = {10 * bar:.1e})")
    assert torch.isfinite(ref).all() and len(solo) == len(R.layout(Ltot, Lw, O_)[0])
    for k, v in d.items():
        assert v >= 10 * bar, (k, v)


# ------------------------------------------------------------------------------------------------ refusals with a NULL context
def _calls(lib, t_start=10, S=5, eta=0.0, codes=1, packed=None, bits=10, n_q=4, F=18, stride=0):
    """the four new entry points on a NULL context; `codes` / `packed` are only ever compared with NULL before the context is needed"""
    return dict(
        sample=lambda: lib.ldc_dpm_sample_windows(None, 1, 1, t_start, S, 180, 18, 80, 40, None),
        decode=lambda: lib.ldc_decode_dpm_windows(None, 1, 5760, t_start, S, 80, 40, 1, None, None, None, None),
        codes=lambda: lib.ldc_decode_codes_windows(None, codes, packed, stride, bits, n_q, F, t_start, S, eta, None, 80, 40, 1, None, None, None),
        codes_dpm=lambda: lib.ldc_decode_codes_dpm_windows(None, codes, packed, stride, bits, n_q, F, t_start, S, 80, 40, 1, None, None, None))


@pytest.mark.parametrize("kw,named,who", [
    (dict(t_start=0), "t_start 0", ("sample", "decode", "codes_dpm")),
    (dict(t_start=-1), "t_start -1", ("sample", "decode", "codes", "codes_dpm")),
    (dict(S=0), "n_steps 0", ("sample", "decode", "codes", "codes_dpm")),
    (dict(S=11), "n_steps 11", ("sample", "decode", "codes", "codes_dpm")),
    (dict(eta=1.5), "eta 1.5", ("codes",)),
    (dict(eta=-0.25), "eta -0.25", ("codes",)),
    (dict(eta=float("nan")), "nan: must be a finite value", ("codes",)),
    (dict(codes=None), "exactly one of codes / packed", ("codes", "codes_dpm")),
    (dict(packed=1), "exactly one of codes / packed", ("codes", "codes_dpm")),
    (dict(codes=None, packed=1, bits=0), "bits", ("codes", "codes_dpm")),
    (dict(codes=None, packed=1, stride=3), "packed_stride 3", ("codes", "codes_dpm")),
    (dict(n_q=0), "n_q", ("codes", "codes_dpm")),
    (dict(F=0), "bad arguments", ("codes", "codes_dpm")),
])
def test_bad_arguments_are_refused_before_the_context_is_looked_at(kw, named, who):
    calls = _calls(L.load(), **kw)
    for k in who:
        assert calls[k]() == L.E_INVALID, k
        assert named in _last_error(), (k, _last_error())


def test_good_arguments_stop_at_the_null_context():
    """(t_start 0 is DDPM halfway sampling for ldc_decode_codes_windows; a t_start only a context's timesteps can refuse passes too)"""
    lib = L.load()
    for kw in (dict(), dict(t_start=1001, S=1001), dict(eta=1.0), dict(codes=None, packed=1, stride=10 ** 6)):
        for k, call in _calls(lib, **kw).items():
            assert call() == L.E_INVALID, (kw, k)
            assert "null ctx" in _last_error(), (kw, k, _last_error())
    assert _calls(lib, t_start=0, S=50)["codes"]() == L.E_INVALID and "null ctx" in _last_error()
    # null tensors are refused as bad arguments, not dereferenced
    assert lib.ldc_dpm_sample_windows(None, None, None, 10, 5, 180, 18, 80, 40, None) == L.E_INVALID and "null tensor" in _last_error()
    assert lib.ldc_decode_dpm_windows(None, None, 5760, 10, 5, 80, 40, None, None, None, None, None) == L.E_INVALID
    assert "bad arguments" in _last_error()


# ------------------------------------------------------------------------------------------------------------------ the CLIs
def test_decompress_and_sample_dpm_take_the_flag_with_the_refusals_of_windows_options():
    for mod in (decompress, sample_dpm):
        p = mod.build_parser()
        assert "chunk_overlap_sec" not in vars(p.parse_args([]))              # absent unless given: a run without it is what it was
        assert sample.windows_options(p.parse_args(["--chunk_sec", "2.4"])) is None
        assert sample.windows_options(p.parse_args(["--chunk_sec", "2.4", "--chunk_overlap_sec", "0.4"])) == 0.4
        for bad in (["--chunk_overlap_sec", "0.4"], ["--chunk_sec", "2.4", "--chunk_overlap_sec", "1.3"],
                    ["--chunk_sec", "2.4", "--chunk_overlap_sec", "-0.1"]):
            with pytest.raises(SystemExit):
                sample.windows_options(p.parse_args(bad))
    assert "coupled" in decompress.__doc__.lower() and "chunk_overlap_sec" in sample_dpm.__doc__


class Stub:
    """an engine that records which windows call it was asked for (the DPM signatures take no noise: one passed on is a TypeError)"""

    def __init__(self):
        self.calls = []

    def decode_windows(self, wav, n_steps, Lw, overlap, noise=None, want_stages=False):
        self.calls.append(("windows", n_steps, Lw, overlap, noise, want_stages))

    def decode_ddim_windows(self, wav, t_start, n_steps, Lw, overlap, eta=0.0, noise=None, want_stages=False):
        self.calls.append(("ddim_windows", t_start, n_steps, Lw, overlap, eta, noise, want_stages))

    def decode_dpm_windows(self, wav, t_start, n_steps, Lw, overlap, want_stages=False):
        self.calls.append(("dpm_windows", t_start, n_steps, Lw, overlap, want_stages))

    def decode_codes_windows(self, codes=None, packed=None, n_steps=None, Lw=None, overlap=None, t_start=0, eta=0.0, noise=None,
                             want_stages=False):
        self.calls.append(("codes_windows", codes, n_steps, Lw, overlap, t_start, eta, noise, want_stages))

    def decode_codes_dpm_windows(self, codes=None, packed=None, t_start=100, n_steps=10, Lw=None, overlap=None, want_stages=False):
        self.calls.append(("codes_dpm_windows", codes, t_start, n_steps, Lw, overlap, want_stages))


def test_chunk_overlap_with_dpm_steps_builds_a_dpm_route():
    e = Stub()
    argv = ["--midway_t", "40", "--dpm_steps", "8", "--chunk_sec", "0.16", "--chunk_overlap_sec", "0.08"]
    a = decompress.build_parser().parse_args(argv + ["--ddim_steps", "0"])
    s = decompress.sampler_from_args(a)
    assert isinstance(s, sample.CodesSampler) and isinstance(s.inner, sample.DpmSampler) and sample.windows_options(a) == 0.08
    sample.window_decoder(e, s, 80, 40)("codes", "a tape that must not travel", True)
    a = sample_dpm.build_parser().parse_args(argv)
    s = sample_dpm.sampler_from_args(a)
    assert isinstance(s, sample.DpmSampler) and sample.windows_options(a) == 0.08
    sample.window_decoder(e, s, 80, 40)("wav", "a tape that must not travel", False)
    # decompress without --dpm_steps: the default sampler and DDIM, from codes
    a = decompress.build_parser().parse_args(["--midway_t", "40", "--chunk_sec", "0.16", "--chunk_overlap_sec", "0.08"])
    sample.window_decoder(e, decompress.sampler_from_args(a), 80, 40)("codes", "tape", False)
    a = decompress.build_parser().parse_args(["--midway_t", "40", "--ddim_steps", "8", "--ddim_eta", "0.5"])
    sample.window_decoder(e, decompress.sampler_from_args(a), 80, 40)("codes", "tape", False)
    sample.window_decoder(e, sample.DdimSampler(40, 8, 1.0), 80, 40)("wav", "tape", False)
    sample.window_decoder(e, sample.DdpmSampler(40), 80, 40)("wav", "tape", True)
    assert e.calls == [("codes_dpm_windows", "codes", 40, 8, 80, 40, True), ("dpm_windows", 40, 8, 80, 40, False),
                       ("codes_windows", "codes", 40, 80, 40, 0, 0.0, "tape", False),
                       ("codes_windows", "codes", 8, 80, 40, 40, 0.5, "tape", False),
                       ("ddim_windows", 40, 8, 80, 40, 1.0, "tape", False), ("windows", 40, 80, 40, "tape", True)]
    with pytest.raises(SystemExit):
        sample.window_decoder(e, object(), 80, 40)


def test_segments_of_codes_fall_on_condition_frames_and_sum_to_the_recording():
    up, hop = 10, 32
    seg = 80 + 31 * 40
    for Ltot in (180, seg, seg + 30, seg + 200, 2 * seg + 70, 3 * seg):
        plan = sample.plan_window_segments(Ltot, 80, 40, up)
        assert plan[0][0] == 0 and sum(n for _, n in plan) == Ltot
        assert all(a + n == b for (a, n), (b, _) in zip(plan, plan[1:]))
        # in condition frames (what a segment of codes is cut at): whole frames that sum to the recording's
        frames = [((a * hop) // 320, ((a + n) * hop) // 320) for a, n in plan]
        assert all(a % up == 0 and n % up == 0 and n >= 80 for a, n in plan)
        assert frames[0][0] == 0 and frames[-1][1] == Ltot // up and all(x[1] == y[0] for x, y in zip(frames, frames[1:]))
        assert all(len(L.window_layout(n, 80, 40, up)[0]) <= 32 for _, n in plan)


def test_engine_takes_one_recording_of_codes_per_call():
    from ladiffcodec_amd.model import Engine
    e = Engine.__new__(Engine)                                             # no context: the ValueError comes before any library call
    with pytest.raises(ValueError, match="one recording per call"):
        Engine.decode_codes_windows(e, codes=torch.zeros(4, 2, 18, dtype=torch.int64), n_steps=3, Lw=80, overlap=40)
    with pytest.raises(ValueError, match="one recording per call"):
        Engine.decode_codes_dpm_windows(e, codes=torch.zeros(4, 2, 18, dtype=torch.int64), t_start=10, n_steps=3, Lw=80, overlap=40)
    with pytest.raises(ValueError, match="required"):
        Engine.decode_codes_windows(e, codes=torch.zeros(4, 1, 18, dtype=torch.int64), n_steps=3)
