"""DDIM sampling on the GPU: parity with the reference's ddim_sample (tests/golden/ddim_r84.npz, tools/gen_golden_ddim.py), the
bf16 / fp8 engines, graph replay against eager steps, graph-cache separation from DDPM, the decode and the DDIM CLI.

The step kernels accumulate GroupNorm statistics with float atomics, so two runs of one configuration may differ in the last
bits: "equal" below is within the f32 run-to-run drift (tests/drift_tolerances.py, key "repeat": 1e-5 relative)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, load_golden, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402

SAME = TOL["f32"]["repeat"]


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ddim_inputs(g, row):
    """(t_start, S, eta, start image or None, noise [S, B, C, L]) of fixture case `row`, regenerated as the generator drew them."""
    t_start, S, eta_m, seed_img, seed_noise = (int(v) for v in g["cases"][row])
    B, C, Lx = g["out_a"].shape
    img = None if seed_img < 0 else torch.randn(B, C, Lx, generator=torch.Generator().manual_seed(seed_img))
    gn = torch.Generator().manual_seed(seed_noise)
    noise = torch.stack([torch.randn(B, C, Lx, generator=gn) for _ in range(S)])
    return t_start, S, eta_m / 1000.0, img, noise


@pytest.mark.parametrize("row,name,tol", [(0, "a", 2e-3), (1, "b", 1e-4), (2, "c", 1e-4), (3, "d", 1e-4)])
def test_ddim_f32_against_reference(row, name, tol):
    """Case a is ill-conditioned: its first iteration (t = 999, eta 0) computes x0 = 20291 (x - eps)
    (sqrt_recip_alphas_cumprod[999] = sqrt_recipm1_alphas_cumprod[999] = 20291), so eps's last-bit differences reach 1e-4 of
    the result (measured 1.5e-4 and 3.7e-4 on two runs on MI355X); it gets the bar of the 1000-step p_sample_loop fixture,
    which starts at the same t."""
    g = load_golden("ddim_r84")
    e = engine("r84", "f32")
    t_start, S, eta, img, noise = ddim_inputs(g, row)
    if img is None:
        img = torch.from_numpy(g["start_c"])
    got = e.ddim_sample(cu(g["cond"]), t_start, S, eta, img=img.cuda(), noise=noise.cuda())
    err = rel(got.cpu().numpy(), g["out_" + name])
    print(f"ddim f32 case {name}: rel {err:.3e}")
    assert err < tol, (name, err)


def test_ddim_facade_dispatch():
    """_Diffusion: the reference's attributes, ddim_sample on them, sample() dispatching on is_ddim_sampling."""
    from ladiffcodec_amd.model import DiffAudioRep
    g = load_golden("ddim_r84")
    e = engine("r84", "f32")
    d = DiffAudioRep(e, L.MODEL_MAIN).diffusion
    assert (d.sampling_timesteps, d.ddim_sampling_eta, d.is_ddim_sampling) == (1000, 0.0, False)
    t_start, S, eta, _, noise = ddim_inputs(g, 2)
    cond, start = cu(g["cond"]), cu(g["start_c"])
    d.num_timesteps, d.sampling_timesteps, d.ddim_sampling_eta = t_start, S, eta
    try:
        got = d.ddim_sample(tuple(start.shape), cond, img=start, noise=noise.cuda())
        assert rel(got.cpu().numpy(), g["out_c"]) < 1e-4
        with pytest.raises(NotImplementedError):
            d.ddim_sample(tuple(start.shape), cond, clip_denoised=False)
        d.seq_length = start.shape[2]
        d.is_ddim_sampling = True
        s = d.sample(batch_size=2, condition=cond)
        assert s.shape == start.shape and torch.isfinite(s).all() and float(s.abs().max()) <= 1.0
    finally:
        d.num_timesteps, d.sampling_timesteps, d.ddim_sampling_eta, d.is_ddim_sampling = 1000, 1000, 0.0, False
    with pytest.raises(L.LdcError):
        e.ddim_sample(cond, 20, 21, 0.0, img=start)          # S > t_start
    with pytest.raises(L.LdcError):
        e.ddim_sample(cond, 20, 6, 1.5, img=start)           # eta > 1
    with pytest.raises(L.LdcError):
        e.ddim_sample(cond, 1001, 6, 0.0, img=start)         # t_start > timesteps


@pytest.mark.parametrize("dtype,key", [("bf16", "lat_200"), ("fp8", "lat_50_act8")])
def test_ddim_bf16_fp8_within_decode_drift(dtype, key):
    """The halfway case (c) and the eta = 1 case (d) on the bf16 / fp8 engines: finite, and within the drift the bf16 / fp8
    decode tests allow for the latents."""
    g = load_golden("ddim_r84")
    e = engine("r84", dtype)
    for row, name in ((2, "c"), (3, "d")):
        t_start, S, eta, img, noise = ddim_inputs(g, row)
        if img is None:
            img = torch.from_numpy(g["start_c"])
        got = e.ddim_sample(cu(g["cond"]), t_start, S, eta, img=img.cuda(), noise=noise.cuda())
        assert torch.isfinite(got).all()
        err = rel(got.cpu().numpy(), g["out_" + name])
        print(f"ddim {dtype} case {name}: rel {err:.3e} (tolerance {TOL[dtype][key]:.3e})")
        assert err < TOL[dtype][key], (dtype, name, err)


def _wav(B=4, T=5120, seed=31):
    return torch.from_numpy(synth.synthetic_wav(B, T, seed=seed)).cuda() * 0.5


@pytest.mark.parametrize("part_graphs", [1, 0])
def test_ddim_graph_replay_equals_eager(part_graphs):
    """10 steps replayed from captured graphs (per-part graphs or one fork / join graph) against the same steps run eagerly
    (serial_parts), Philox draws with eta 0.6: the same draws, the same result."""
    e = engine("r84", "f32")
    wav = _wav()
    try:
        e.set_option("part_graphs", part_graphs)
        e.reseed(123)
        replayed = e.decode_ddim(wav, 40, 10, 0.6, per_item=True, want_stages=True)["latents"].clone()
        e.reseed(123)
        again = e.decode_ddim(wav, 40, 10, 0.6, per_item=True, want_stages=True)["latents"].clone()
        e.set_option("serial_parts", 1)
        e.reseed(123)
        eager = e.decode_ddim(wav, 40, 10, 0.6, per_item=True, want_stages=True)["latents"].clone()
    finally:
        e.set_option("serial_parts", 0)
        e.set_option("part_graphs", 1)
    assert torch.isfinite(replayed).all()
    assert rel(again.cpu().numpy(), replayed.cpu().numpy()) < SAME
    assert rel(eager.cpu().numpy(), replayed.cpu().numpy()) < SAME, part_graphs


def test_ddpm_and_ddim_graphs_do_not_mix():
    """DDPM -> DDIM(S=10) -> DDIM(S=7) -> DDIM(S=10) -> DDPM on one engine and shape, reseeded before each: the repeats agree,
    so no call replayed the other sampler's graph."""
    e = engine("r84", "f32")
    wav = _wav(seed=32)

    def run(kind, S=0):
        e.reseed(77)
        if kind == "ddpm":
            r = e.decode(wav, 8, per_item=True, want_stages=True)
        else:
            r = e.decode_ddim(wav, 40, S, 0.5, per_item=True, want_stages=True)
        return r["latents"].clone().cpu().numpy()

    p1, d10, d7, d10b, p2 = run("ddpm"), run("ddim", 10), run("ddim", 7), run("ddim", 10), run("ddpm")
    assert rel(p2, p1) < SAME and rel(d10b, d10) < SAME
    assert rel(d7, d10) > 1e-3 and rel(d10, p1) > 1e-3


def test_ddim_split_on_off_unchanged():
    """One chain (split 1) or two parts (split 2): the Philox draws are addressed by the global element, so the result is the same
    up to the kernels' own per-shape differences."""
    e = engine("r84", "f32")
    wav = _wav(seed=33)
    try:
        e.set_option("split", 1)
        e.reseed(5)
        one = e.decode_ddim(wav, 40, 10, 0.8, per_item=True, want_stages=True)["latents"].clone()
        e.set_option("split", 2)
        e.reseed(5)
        two = e.decode_ddim(wav, 40, 10, 0.8, per_item=True, want_stages=True)["latents"].clone()
    finally:
        e.set_option("split", 2)
    assert rel(one.cpu().numpy(), two.cpu().numpy()) < 1e-4


def test_decode_ddim_equals_staged_composition():
    """decode_ddim = get_cond -> cond_upsample (per-item max normalisation) -> ddim_sample -> decode_latents -> output_normalise."""
    e = engine("r84", "f32")
    mc = CASES["r84"][0]
    wav = _wav(seed=34)
    B, _, T = wav.shape
    S, t_start, eta = 6, 30, 0.7
    noise = torch.randn(S, B, 128, T // mc.hop_length, generator=torch.Generator().manual_seed(8)).cuda()
    got = e.decode_ddim(wav, t_start, S, eta, noise=noise, per_item=True, want_stages=True)
    cond = e.get_cond(wav)
    up = e.cond_upsample(cond, 0)
    start = up / (up.abs().amax(dim=(1, 2), keepdim=True) + 1e-8)
    lat = e.ddim_sample(cond, t_start, S, eta, img=start, noise=noise)
    out = e.output_normalise(e.decode_latents(L.MODEL_MAIN, lat), per_item=True)
    assert rel(got["cond"].cpu().numpy(), cond.cpu().numpy()) < SAME
    assert rel(got["latents"].cpu().numpy(), lat.cpu().numpy()) < 1e-4
    assert rel(got["wav"].cpu().numpy(), out.cpu().numpy()) < 1e-3


def test_ddim_cli_end_to_end_equals_engine(tmp_path):
    """`python -m ladiffcodec_amd.sample_ddim` on a tiny tree (one batch of three equal-length files) writes what Engine.decode_ddim
    returns for the same batch and seed."""
    from scipy.io import wavfile
    from ladiffcodec_amd import sample_ddim
    from ladiffcodec_amd.model import Engine
    mc, u, _ = CASES["r84"]
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind, outd = tmp_path / "in", tmp_path / "out"
    (ind / "spk1").mkdir(parents=True)
    names = ["spk1/a.wav", "spk1/b.wav", "c.wav"]
    xs = [(synth.synthetic_wav(1, 5120, seed=40 + k)[0, 0] * 0.5).astype(np.float32) for k in range(3)]
    for n, x in zip(names, xs):
        wavfile.write(str(ind / n), 16000, x)
    written = sample_ddim.main([
        "--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff",
        "--scaling_global", "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
        "--diff_dims", "32", "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", "30", "--dtype", "f32",
        "--ddim_steps", "7", "--ddim_eta", "0.5", "--seed", "3"])
    assert len(written) == 3
    eng = Engine(mc, u, COND_CFG, dtype="f32", noise_seed=3 + 0 + 7919 * 0)
    eng.load_state_dict(L.MODEL_MAIN, main_sd_np("r84"))
    eng.load_state_dict(L.MODEL_COND, cond_sd_np())
    eng.finalize(strict=True)
    # the CLI batches equal lengths in sorted file order (glob of the tree, sorted)
    order = sorted(str(ind / n) for n in names)
    batch = torch.from_numpy(np.stack([xs[names.index(p[len(str(ind)) + 1:])] for p in order])[:, None, :]).cuda()
    ref = eng.decode_ddim(batch, 30, 7, 0.5, per_item=True).cpu().numpy()
    eng.close()
    for k, p in enumerate(order):
        sr, y = wavfile.read(str(outd / p[len(str(ind)) + 1:]))
        assert sr == 16000 and y.shape == (5120,)
        assert rel(y, ref[k, 0]) < 1e-4, p
