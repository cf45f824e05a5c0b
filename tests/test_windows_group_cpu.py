"""Window groups ("Several recordings per call") without a GPU: the host-only layout entry against the
single-recording layout bit for bit, the cap, every refusal with its value, the context-free refusals of the calls, and -- on the CPU
oracle alone -- the two mutants the GPU comparisons must be able to see (tests/windows_group_restatement.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ladiffcodec_amd import lib as L, sample, sample_ddim, sample_dpm
from drift_tolerances import TOL
import windows_group_restatement as G
import windows_restatement as R

NEW = ["ldc_window_group_layout", "ldc_unet_forward_windows_group", "ldc_sample_windows_group", "ldc_decode_windows_group"]
GROUPS = [((180, 80, 240), 80, 40, 10), ((400, 160), 160, 40, 40), ((80,), 80, 40, 10), ((200, 200, 80, 120), 80, 20, 10),
          ((240, 80, 160), 80, 0, 10), (tuple([80] * 32), 80, 40, 10), (tuple([180] * 8), 80, 40, 10), ((80 + 31 * 40,), 80, 40, 10)]


def _last_error():
    return L.load().ldc_last_error().decode()


def test_exports_listed_and_bound():
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTS and getattr(lib, name).argtypes, name


@pytest.mark.parametrize("lens,Lw,O_,up", GROUPS)
def test_group_layout_is_every_recordings_own_layout(lens, Lw, O_, up):
    w0, starts, w = L.window_group_layout(lens, Lw, O_, up)
    rw0, rstarts = G.layout(lens, Lw, O_, up)
    assert w0 == rw0 and starts == rstarts
    assert w.shape == (w0[-1], Lw)
    for r, Ltot in enumerate(lens):
        s1, w1 = L.window_layout(Ltot, Lw, O_, up)
        assert starts[w0[r]:w0[r + 1]] == s1
        assert np.array_equal(w[w0[r]:w0[r + 1]].view(np.uint32), w1.view(np.uint32)), r     # bit for bit


def test_the_cap_is_32_windows_in_all():
    w0, starts, _ = L.window_group_layout([180] * 8, 80, 40, 10)          # 8 x 4 windows
    assert w0 == list(range(0, 33, 4)) and len(starts) == 32
    with pytest.raises(L.LdcError) as ei:
        L.window_group_layout([180] * 9, 80, 40, 10)                      # a ninth recording
    assert ei.value.code == L.E_INVALID and "36 windows" in str(ei.value) and "at most 32" in str(ei.value)
    with pytest.raises(ValueError):
        G.layout([180] * 9, 80, 40, 10)


@pytest.mark.parametrize("lens,Lw,O_,up,word", [
    ((), 80, 40, 10, "R 0"), (tuple([80] * 33), 80, 40, 10, "R 33"),
    ((180, 70, 240), 80, 40, 10, "recording 1: Ltot 70"),                 # shorter than the window: it would shrink it
    ((180, 40), 80, 40, 10, "recording 1: Ltot 40"),
    ((180, 185), 80, 40, 10, "recording 1: Ltot 185"), ((0, 180), 80, 40, 10, "recording 0: Ltot 0"),
    ((180, 80), 85, 40, 10, "Lw 85"), ((180, 80), 0, 0, 10, "Lw 0"),
    ((180, 80), 80, 45, 10, "overlap 45"), ((180, 80), 80, 50, 10, "overlap 50"), ((180, 80), 80, -10, 10, "overlap -10"),
    ((180, 80), 80, 40, 0, "up 0"),
    ((80, 80 + 32 * 40), 80, 40, 10, "recording 1: Ltot 1360 needs 33 windows"),
    ((180, 80, 240, 80 + 22 * 40), 80, 40, 10, "33 windows"),
])
def test_layout_refusals_name_the_value(lens, Lw, O_, up, word):
    with pytest.raises(L.LdcError) as ei:
        L.window_group_layout(lens, Lw, O_, up)
    assert ei.value.code == L.E_INVALID and word in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        G.layout(lens, Lw, O_, up)


def test_null_lists_and_outputs():
    lib = L.load()
    assert lib.ldc_window_group_layout(2, None, 80, 40, 10, None, None, None) == L.E_INVALID and "null" in _last_error()
    arr = (C.c_int * 3)(180, 80, 240)
    assert lib.ldc_window_group_layout(3, arr, 80, 40, 10, None, None, None) == 10     # every output is optional


# ------------------------------------------------------------------------------------------ refusals that need no context, in their order
def _sample(lib, sampler, t_start, S, eta=0.0, img=1, noise=None, seeds=None):
    return lib.ldc_sample_windows_group(None, img, 1, sampler, t_start, S, eta, noise, seeds, 1, (C.c_int * 1)(180), (C.c_int * 1)(18), 80, 40, None)


def _decode(lib, sampler, t_start, S, eta=0.0, wav=1):
    return lib.ldc_decode_windows_group(None, wav, 1, (C.c_int * 1)(5760), sampler, t_start, S, eta, None, None, 80, 40, 1, None, None, None, None)


def test_sampler_front_refusals_follow_the_single_calls():
    lib = L.load()
    for call in (_sample, _decode):
        assert call(lib, 3, 10, 5) == L.E_INVALID and "sampler 3" in _last_error()
        # DPM: the schedule's arguments first, also with a NULL context (ldc_dpm_sample_windows)
        assert call(lib, 2, 0, 5) == L.E_INVALID and "t_start 0" in _last_error()
        assert call(lib, 2, 10, 11) == L.E_INVALID and "n_steps 11" in _last_error()
        assert call(lib, 2, 10, 5) == L.E_INVALID and "null ctx" in _last_error()
        # DDPM, DDIM: the context first (ldc_denoise_windows, ldc_ddim_sample_windows)
        assert call(lib, 0, 0, 0) == L.E_INVALID and "null ctx" in _last_error()
        assert call(lib, 1, 10, 11, 1.5) == L.E_INVALID and "null ctx" in _last_error()
    assert _sample(lib, 2, 10, 5, img=None) == L.E_INVALID and "null tensor" in _last_error()
    assert _decode(lib, 2, 10, 5, wav=None) == L.E_INVALID and "bad arguments" in _last_error()
    assert lib.ldc_unet_forward_windows_group(None, 1, 5, 1, 1, (C.c_int * 1)(180), (C.c_int * 1)(18), 80, 40, 1, None) == L.E_INVALID
    assert "null ctx" in _last_error()


# ------------------------------------------------------------------------------------------------- the restatement's own consistency
def test_the_joint_loop_without_a_mutant_is_every_recording_alone():
    """one batch of all windows per step, blended per recording, gives what the single-recording restatement gives (6 steps)"""
    s = G.inputs("r84", 6)
    a = (s[0]["sd"], s[0]["u"], [i["img"] for i in s], [i["cond"] for i in s], 6, [i["noise"] for i in s], 80, 40, s[0]["up"])
    d = G.rel_group([x.numpy() for x in G.joint_denoise(*a)], [x.numpy() for x in G.denoise_windows_group(*a)])
    print(f"joint loop against every recording alone: {d:.3e}")
    assert d < TOL["f32"]["chain_small"]                                   # (another batch size: another summation order inside the oracle)


def test_packing():
    xs = [torch.arange(2 * n, dtype=torch.float32).reshape(1, 2, n) + 100 * r for r, n in enumerate((3, 2))]
    p = G.pack(xs)
    assert p.tolist() == [0, 1, 2, 3, 4, 5, 100, 101, 102, 103]           # [C][Ltot_r] blocks at C * off_r
    tapes = [x[None].repeat(2, 1, 1, 1) for x in xs]
    assert G.pack_tapes(tapes).shape == (2, 10) and torch.equal(G.pack_tapes(tapes)[1], p)
    m = G.mutant_tapes(tapes)                                              # c * Lsum + off_r + l on the packed step
    assert m[0][0, 0].tolist() == [[0, 1, 2], [5, 100, 101]] and m[1][0, 0].tolist() == [[3, 4], [102, 103]]


# ------------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_flag_and_the_group_planner():
    base = ["--model_path", "m", "--input_dir", "i/", "--output_dir", "o/", "--chunk_sec", "0.16"]
    for mod in (sample, sample_ddim, sample_dpm):
        a = mod.build_parser().parse_args(base)
        assert not hasattr(a, "window_group") and sample.window_group_option(a) is False        # absent unless given, like --ragged
        a = mod.build_parser().parse_args(base + ["--chunk_overlap_sec", "0.08", "--window_group"])
        assert a.window_group is True and sample.window_group_option(a) is True
        with pytest.raises(SystemExit) as ei:
            sample.window_group_option(mod.build_parser().parse_args(base + ["--window_group"]))
        assert "--chunk_overlap_sec" in str(ei.value)
    # file order, first fit, at most 32 windows per group
    assert sample.plan_window_groups([4, 1, 5]) == [[0, 1, 2]]
    assert sample.plan_window_groups([20, 15, 12, 17, 1]) == [[0, 2], [1, 3], [4]]               # 12 fills the first group, 17 the second
    assert sample.plan_window_groups([20, 15, 2, 1]) == [[0, 2, 3], [1]]
    assert sample.plan_window_groups([32, 32, 1]) == [[0], [1], [2]]
    assert sample.plan_window_groups([]) == []
    with pytest.raises(ValueError):
        sample.plan_window_groups([4, 33])


# --------------------------------------------------------------------------------------------------- what the GPU bars can tell apart
def test_discrimination_conditions_on_the_oracle():
    """At the GPU test's shapes (r84: Lw 80, overlap 40, recordings of 180, 80 and 240 frames, 40 steps on seeded tapes) each mutant lies
    at least 10 x the f32 chain bar from the contract: (a) a recording's cover read without w0_r, (b) the tape indexed on the packed
    axis.  Recording 0 has w0 = 0, so (a) leaves it alone; (b) moves every recording."""
    bar = TOL["f32"]["chain_small"]
    ref = G.reference("r84")
    d = {}
    for mode in ("cover", "noise"):
        other = G.reference("r84", mode=mode)
        d[mode] = [float((a - b).abs().max()) / float(a.abs().max()) for a, b in zip(ref, other)]
    print(f"window group r84 against (a) cover without w0_r {['%.3e' % v for v in d['cover']]}, (b) noise on the packed axis "
          f"{['%.3e' % v for v in d['noise']]} (10 x bar = {10 * bar:.1e})")
    assert d["cover"][0] < bar
    assert min(d["cover"][1:]) >= 10 * bar
    assert min(d["noise"]) >= 10 * bar
    assert all(torch.isfinite(x).all() for x in ref)
