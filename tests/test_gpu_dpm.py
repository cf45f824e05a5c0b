"""DPM-Solver++(2M) sampling on the GPU against the Python restatement of the published update (tests/dpm_restatement.py, on the CPU
oracle's UNet), the bf16 / fp8 engines, the x0 history across captured graphs and across calls, graph-cache separation from DDPM and
DDIM, the noise epoch, ragged batches, the decodes' composition and the CLI.

Bars.  f32 latents: TOL["f32"]["chain_small"] (1e-5; on the CPU the float32-state restatement is 3.6e-7 ... 4.8e-7 from a float64-state
one at these shapes, the DDIM chains on MI355X sit at 3.6e-7 ... 5.4e-7 from `oracle_ddim`).  bf16 latents had no bar, so the parent
path was measured: `Engine.ddim_sample(eta=0)` of the commit before this sampler against `oracle_ddim` on the items and schedules of
test 1, on MI355X, two runs each: (40, 8) 9.4e-4 / 9.6e-4 (`r84`), 9.8e-4 / 9.2e-4 (`r8`); (100, 12) 2.15e-3 / 1.89e-3 (`r84`),
2.09e-3 / 2.09e-3 (`r8`).  DDIM_BF16_MEASURED holds the worst; DPM is held to 2 x it, the rule of tests/drift_tolerances.py and
RAGGED_B1_DDIM_LATENTS (DESIGN.md section 5f quotes it).  "Equal" is TOL[dtype]["repeat"]: the step kernels sum GroupNorm statistics
with float atomics.  Every comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402
import dpm_restatement as R  # noqa: E402

SAME = TOL["f32"]["repeat"]
DDIM_BF16_MEASURED = 2.15e-3   # Engine.ddim_sample(eta 0), bf16, against oracle_ddim: `r84`, (100, 12); see the module docstring
# Two runs of ONE bf16 ragged decode differ by more than TOL["bf16"]["repeat"] (3.6e-4, recorded on the rectangular DDPM decode): the
# parent path, `Engine.decode_ragged(t_start 40, S 8, eta 0)` on the items of test 8 (`r84`), run five times against its first run on
# MI355X, clean or with 1e30 / NaN behind the lengths, on the commit before this sampler and on this one: latents 5.5e-4 ... 6.84e-4
# (waveforms 9.8e-5 ... 1.35e-4; f32 3.0e-7 ... 3.6e-7).  The padding test holds bf16 to twice the worst, like every measured bar here.
RAGGED_DDIM_BF16_REPEAT = 6.84e-4
SCHEDULES = [(40, 8), (100, 12)]
_REF = {}


def lat_bar(dtype):
    return TOL["f32"]["chain_small"] if dtype == "f32" else 2.0 * DDIM_BF16_MEASURED


def _wav(B=4, T=5120, seed=31):
    return torch.from_numpy(synth.synthetic_wav(B, T, seed=seed)) * 0.5


def inputs(tag, seed=31):
    """the oracle's condition and start image (per-item normalisation) of _wav(B=2, seed), computed once"""
    key = (tag, "in", seed)
    if key not in _REF:
        mc, u, _ = CASES[tag]
        sdm = synth.to_torch(main_sd_np(tag))
        cond = O.get_cond(synth.to_torch(cond_sd_np()), COND_CFG, _wav(2, seed=seed))[0]
        _REF[key] = dict(sdm=sdm, u=u, cond=cond, img=O.start_image(sdm, u, cond, True))
    return _REF[key]


def restated(tag, t_start, S):
    key = (tag, t_start, S)
    if key not in _REF:
        i = inputs(tag)
        _REF[key] = R.dpm_sample(i["sdm"], i["u"], i["img"], i["cond"], t_start, S)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------ 1, 2: the restatement
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("t_start,S", SCHEDULES)
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_dpm_sample_against_the_restatement(tag, t_start, S, dtype):
    i = inputs(tag)
    ref = restated(tag, t_start, S)
    got = engine(tag, dtype).dpm_sample(i["cond"].cuda(), t_start, S, i["img"].cuda())
    assert torch.isfinite(got).all()
    err = rel(got.cpu().numpy(), ref.numpy())
    print(f"dpm {tag} {dtype} ({t_start},{S}): latents rel {err:.3e} (bar {lat_bar(dtype):.3e})")
    assert err < lat_bar(dtype), (tag, dtype, t_start, S, err)


@pytest.mark.parametrize("t_start,S", SCHEDULES)
def test_dpm_fp8_within_decode_drift(t_start, S):
    i = inputs("r84")
    got = engine("r84", "fp8").dpm_sample(i["cond"].cuda(), t_start, S, i["img"].cuda())
    assert torch.isfinite(got).all()
    err = rel(got.cpu().numpy(), restated("r84", t_start, S).numpy())
    print(f"dpm r84 fp8 ({t_start},{S}): latents rel {err:.3e} (tolerance {TOL['fp8']['lat_50_act8']:.3e})")
    assert err < TOL["fp8"]["lat_50_act8"], err


# ------------------------------------------------------------------------------------------------------------ 3: history across graphs
@pytest.mark.parametrize("part_graphs", [1, 0])
def test_dpm_history_survives_graph_boundaries(part_graphs):
    """12 iterations replayed from captured graphs (two 5-step graphs and two single steps: iteration 5, 10 and 11 read a history
    that another replay wrote) against the same iterations run eagerly (serial_parts)."""
    e = engine("r84", "f32")
    wav = _wav().cuda()
    try:
        e.set_option("part_graphs", part_graphs)
        first = e.decode_dpm(wav, 100, 12, per_item=True, want_stages=True)["latents"].clone()     # (captures on its first use)
        replayed = e.decode_dpm(wav, 100, 12, per_item=True, want_stages=True)["latents"].clone()
        again = e.decode_dpm(wav, 100, 12, per_item=True, want_stages=True)["latents"].clone()
        e.set_option("serial_parts", 1)
        eager = e.decode_dpm(wav, 100, 12, per_item=True, want_stages=True)["latents"].clone()
    finally:
        e.set_option("serial_parts", 0)
        e.set_option("part_graphs", 1)
    assert torch.isfinite(replayed).all()
    errs = [rel(x.cpu().numpy(), eager.cpu().numpy()) for x in (first, replayed, again)]
    print(f"dpm graphs part_graphs {part_graphs}: first / replayed / again against eager {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e} (bar {SAME:.3e})")
    assert max(errs) < SAME, (part_graphs, errs)


# ------------------------------------------------------------------------------------------------------------ 4: history never leaks
def test_dpm_history_never_leaks_between_calls():
    e = engine("r84", "f32")
    a, b = inputs("r84"), inputs("r84", seed=35)
    ca, ia, cb, ib = a["cond"].cuda(), a["img"].cuda(), b["cond"].cuda(), b["img"].cuda()
    e.dpm_sample(ca, 100, 12, ia)                                  # leaves its x0 in the plans' history
    one = e.dpm_sample(cb, 60, 1, ib)                              # the only iteration is the last: the clipped x0
    ref = e.ddim_sample(cb, 60, 1, 0.0, img=ib)
    err1 = rel(one.cpu().numpy(), ref.cpu().numpy())
    print(f"dpm S=1 against ddim S=1: {err1:.3e} (bar {SAME:.3e})")
    assert float(one.abs().max()) <= 1.0
    assert err1 < SAME, err1
    first = e.dpm_sample(ca, 100, 10, ia).clone()
    e.dpm_sample(cb, 40, 8, ib)                                    # another call's history in between
    second = e.dpm_sample(ca, 100, 10, ia)
    err2 = rel(second.cpu().numpy(), first.cpu().numpy())
    print(f"dpm 10 steps, twice with another call in between: {err2:.3e} (bar {SAME:.3e})")
    assert err2 < SAME, err2


# ------------------------------------------------------------------------------------------------------------ 5: graph kinds
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_sampler_graphs_do_not_mix(tag):
    """DDPM -> DDIM -> DPM -> DDIM -> DPM -> DDPM on one engine and shape, reseeded before each: the repeats agree, so no call
    replayed another sampler's graph; DPM is a different result from DDIM at eta 0 (CPU oracle: 4.4e-3 `r84`, 5.8e-3 `r8`)."""
    e = engine(tag, "f32")
    wav = _wav(seed=31).cuda()

    def run(kind):
        e.reseed(77)
        if kind == "ddpm":
            r = e.decode(wav, 8, per_item=True, want_stages=True)
        elif kind == "ddim":
            r = e.decode_ddim(wav, 100, 10, 0.0, per_item=True, want_stages=True)
        else:
            r = e.decode_dpm(wav, 100, 10, per_item=True, want_stages=True)
        return r["latents"].clone().cpu().numpy()

    p1, i1, m1, i2, m2, p2 = (run(k) for k in ("ddpm", "ddim", "dpm", "ddim", "dpm", "ddpm"))
    errs = rel(p2, p1), rel(i2, i1), rel(m2, m1)
    print(f"sampler kinds {tag}: repeats ddpm {errs[0]:.3e} ddim {errs[1]:.3e} dpm {errs[2]:.3e} (bar {SAME:.3e}); dpm against ddim {rel(m1, i1):.3e}")
    assert max(errs) < SAME, errs
    assert rel(m1, i1) > 1e-3 and rel(m1, p1) > 1e-3


# ------------------------------------------------------------------------------------------------------------ 6, 7: split, epoch
def test_dpm_split_on_off_unchanged():
    e = engine("r84", "f32")
    wav = _wav(seed=33).cuda()
    try:
        e.set_option("split", 1)
        one = e.decode_dpm(wav, 40, 10, per_item=True, want_stages=True)["latents"].clone()
        e.set_option("split", 2)
        two = e.decode_dpm(wav, 40, 10, per_item=True, want_stages=True)["latents"].clone()
    finally:
        e.set_option("split", 2)
    err = rel(one.cpu().numpy(), two.cpu().numpy())
    print(f"dpm split 1 against split 2: {err:.3e} (bar 1e-4)")
    assert err < 1e-4, err


def test_dpm_leaves_the_noise_epoch_alone():
    """reseed; decode == reseed; decode_dpm; decode, with device-drawn (Philox) noise: a DPM call draws nothing and moves no epoch."""
    e = engine("r84", "f32")
    wav = _wav(seed=36).cuda()
    e.reseed(5)
    plain = e.decode(wav, 8, per_item=True, want_stages=True)["latents"].clone()
    e.reseed(5)
    e.decode_dpm(wav, 40, 8, per_item=True)
    e.dpm_sample(inputs("r84")["cond"].cuda(), 40, 8, inputs("r84")["img"].cuda())
    after = e.decode(wav, 8, per_item=True, want_stages=True)["latents"].clone()
    err = rel(after.cpu().numpy(), plain.cpu().numpy())
    print(f"decode after a DPM call against decode alone: {err:.3e} (bar {SAME:.3e})")
    assert err < SAME, err


# ------------------------------------------------------------------------------------------------------------ 8: ragged
def ragged_refs(tag, t_start=40, S=8):
    from test_gpu_ragged import setup
    s = setup(tag)
    key = (tag, "ragged", t_start, S)
    if key not in _REF:
        refs = []
        for b, n in enumerate(s["lens"]):
            r = s["solo"][b]
            lat = R.dpm_sample(s["sdm"], s["u"], r["img0"], r["cond"], t_start, S)
            refs.append(dict(r, latents=lat, wav=O.output_normalise(O.seanet_decode(s["sdm"], s["mc"], lat), True)))
        _REF[key] = refs
    return s, _REF[key]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_decode_ragged_dpm(tag, dtype):
    """The four lengths of tests/test_gpu_ragged.py in one call against every item's solo restatement: codes, waveforms under that
    file's ragged bar, exact zeros behind every length.  Latents under "chain_small" on f32; bf16 latents are printed and held to the
    bf16 bar of test 1 (tests/test_gpu_ragged.py's DDIM test has no bf16 latents bar either: its "chain_small" was recorded on DDPM)."""
    from test_gpu_ragged import check_items
    s, refs = ragged_refs(tag)
    e = engine(tag, dtype)
    got = e.decode_ragged_dpm(s["wav"].cuda(), s["lens"], 40, 8, want_stages=True)
    for b, n in enumerate(s["lens"]):
        v = rel(got["latents"][b:b + 1, :, :n // s["hop"]].cpu().numpy(), refs[b]["latents"].numpy())
        print(f"ragged dpm {tag} {dtype} item {b}: latents {v:.3e} (bar {lat_bar(dtype):.3e})")
        assert v < lat_bar(dtype), (tag, dtype, b, v)
    check_items(dtype, s, got, refs, keys=("latents", "wav") if dtype == "f32" else ("wav",))


@pytest.mark.parametrize("fill", [1e30, float("nan")])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dpm_padding_never_reaches_a_valid_value(dtype, fill):
    """1e30 / NaN behind every length of `wav`: finite, exactly zero behind the lengths, and unchanged within the run-to-run drift
    (f32: "repeat", 1e-5; bf16: twice the parent path's own run-to-run figure, RAGGED_DDIM_BF16_REPEAT)."""
    from test_gpu_ragged import setup
    bar = TOL["f32"]["repeat"] if dtype == "f32" else max(TOL["bf16"]["repeat"], 2.0 * RAGGED_DDIM_BF16_REPEAT)
    s = setup("r84")
    e = engine("r84", dtype)
    base = {k: v.clone() for k, v in e.decode_ragged_dpm(s["wav"].cuda(), s["lens"], 40, 8, want_stages=True).items()}
    wav = s["wav"].clone()
    for b, n in enumerate(s["lens"]):
        wav[b, :, n:] = fill
    got = e.decode_ragged_dpm(wav.cuda(), s["lens"], 40, 8, want_stages=True)
    for b, n in enumerate(s["lens"]):
        for k, m in (("latents", n // s["hop"]), ("wav", n), ("cond", n // COND_CFG.hop_length)):
            a, r = got[k][b, :, :m].cpu(), base[k][b, :, :m].cpu()
            assert torch.isfinite(a).all(), (k, b)
            v = rel(a.numpy(), r.numpy())
            print(f"dpm padding {fill} {dtype} item {b} {k}: {v:.3e} (bar {bar:.3e})")
            assert v < bar, (k, b, v)
            assert not got[k][b, :, m:].any(), (k, b)


def test_ragged_dpm_refused_on_the_fp8_engine_and_off_the_quantum():
    from test_gpu_ragged import setup
    s = setup("r84")
    with pytest.raises(L.LdcError) as ei:
        engine("r84", "fp8").decode_ragged_dpm(s["wav"].cuda(), s["lens"], 40, 8)
    assert ei.value.code == L.E_INVALID and "fp8" in str(ei.value)
    e = engine("r84", "f32")
    for bad in (dict(lengths=[s["q"] + 320] + s["lens"][1:]), dict(t_start=1001), dict(n_steps=41), dict(n_steps=0)):
        a = dict(lengths=s["lens"], t_start=40, n_steps=8)
        a.update(bad)
        with pytest.raises(L.LdcError) as ei:
            e.decode_ragged_dpm(s["wav"].cuda(), a["lengths"], a["t_start"], a["n_steps"])
        assert ei.value.code == L.E_INVALID, bad


# ------------------------------------------------------------------------------------------------------------ 9: composition
def test_decode_dpm_equals_staged_composition_and_the_decode_from_codes():
    e = engine("r84", "f32")
    wav = _wav(seed=34).cuda()
    t_start, S = 30, 6
    got = e.decode_dpm(wav, t_start, S, per_item=True, want_stages=True)
    got = {k: v.clone() for k, v in got.items()}
    cond = e.get_cond(wav)
    up = e.cond_upsample(cond, 0)
    start = up / (up.abs().amax(dim=(1, 2), keepdim=True) + 1e-8)
    lat = e.dpm_sample(cond, t_start, S, start)
    out = e.output_normalise(e.decode_latents(L.MODEL_MAIN, lat), per_item=True)
    errs = (rel(got["cond"].cpu().numpy(), cond.cpu().numpy()), rel(got["latents"].cpu().numpy(), lat.cpu().numpy()),
            rel(got["wav"].cpu().numpy(), out.cpu().numpy()))
    print(f"decode_dpm against its stages: cond {errs[0]:.3e} latents {errs[1]:.3e} wav {errs[2]:.3e}")
    assert errs[0] < SAME and errs[1] < 1e-4 and errs[2] < 1e-3, errs
    from_codes = e.decode_codes_dpm(codes=got["codes"], t_start=t_start, n_steps=S, per_item=True, want_stages=True)
    errs = rel(from_codes["latents"].cpu().numpy(), got["latents"].cpu().numpy()), rel(from_codes["wav"].cpu().numpy(), got["wav"].cpu().numpy())
    print(f"decode_codes_dpm against decode_dpm: latents {errs[0]:.3e} wav {errs[1]:.3e} (bar {SAME:.3e})")
    assert max(errs) < SAME, errs


# ------------------------------------------------------------------------------------------------------------ 10: the CLI
def test_dpm_cli_end_to_end_equals_engine(tmp_path):
    """`python -m ladiffcodec_amd.sample_dpm` on a tiny tree (one batch of three equal-length files) writes what Engine.decode_dpm
    returns for the same batch."""
    from scipy.io import wavfile
    from ladiffcodec_amd import sample_dpm
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind, outd = tmp_path / "in", tmp_path / "out"
    (ind / "spk1").mkdir(parents=True)
    names = ["spk1/a.wav", "spk1/b.wav", "c.wav"]
    xs = [(synth.synthetic_wav(1, 5120, seed=40 + k)[0, 0] * 0.5).astype(np.float32) for k in range(3)]
    for n, x in zip(names, xs):
        wavfile.write(str(ind / n), 16000, x)
    written = sample_dpm.main([
        "--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff",
        "--scaling_global", "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
        "--diff_dims", "32", "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", "30", "--dtype", "f32",
        "--dpm_steps", "7", "--seed", "3"])
    assert len(written) == 3
    order = sorted(str(ind / n) for n in names)           # the CLI batches equal lengths in sorted file order
    batch = torch.from_numpy(np.stack([xs[names.index(p[len(str(ind)) + 1:])] for p in order])[:, None, :]).cuda()
    ref = engine("r84", "f32").decode_dpm(batch, 30, 7, per_item=True).cpu().numpy()
    for k, p in enumerate(order):
        sr, y = wavfile.read(str(outd / p[len(str(ind)) + 1:]))
        assert sr == 16000 and y.shape == (5120,)
        err = rel(y, ref[k, 0])
        print(f"dpm cli {p[len(str(ind)) + 1:]}: {err:.3e} (bar 1e-4)")
        assert err < 1e-4, p
