"""Coupled windows on the GPU against the Python restatement on the CPU oracle (tests/windows_restatement.py) and
against the engine's own B = 1 and independent-chunk calls.

Shapes (Ltot, Lw, overlap) in latent frames: `r84` (180, 80, 40) -- four windows, a triple-covered stretch, Ltot no multiple of the
32-frame tile -- and (200, 80, 20); `r8` (400, 160, 40).  Halfway runs take 40 steps, DDIM (40, 8) at eta 0 and 1.  The references are
computed once per process and shared (windows_restatement.reference / _REF below); nothing writes to them.

Bars: tests/drift_tolerances.py; every test prints its figure before it asserts.  The generic bf16 bars were recorded on 10-step chains;
where a bf16 figure of these 40-step chains exceeds one (the windows gave 1.2e-3 ... 1.8e-3 against `chain_small` 6.4e-4, and 3.2e-4 ...
4.9e-4 run to run against `repeat` 3.6e-4), the bar is twice what the PARENT's path shows on the same items, two runs on MI355X, held in
PARENT_MEASURED below (DESIGN.md section 5g records both sides).  f32 keeps the generic bars throughout.  The bf16 chain bar cannot see
windows that are blended once at the end (8.2e-4 from the scheme, tests/test_windows_cpu.py); the f32 engine's does, and both see a hard
switch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, sample, synth  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
from oracle import ldc_oracle as O, philox_oracle as P  # noqa: E402
import windows_restatement as R  # noqa: E402

SHAPES = [("r84", 180, 80, 40), ("r84", 200, 80, 20), ("r8", 400, 160, 40)]
MAIN = [("r84", 180, 80, 40), ("r8", 400, 160, 40)]            # one shape per checkpoint where a case needs a reference of its own
N, T_START, S = 40, 40, 8
SEED = 0x5EED0123
C = 128

# bf16 only, worst of two runs on MI355X of the PARENT's path on the same items (see the module docstring); a figure without an entry
# keeps the generic bar.
#   ("chain", tag, Ltot)        Engine.denoise, 40 steps, of the W windows as independent items against the oracle's solo runs
#   ("ddim", tag, Ltot, eta)    Engine.ddim_sample (40, 8) of the same items against the DDIM restatement of the ragged tests
#   ("decode_lat" | "decode_wav", tag, Ltot)   Engine.decode of the windows' stretches of the recording against the oracle's solo decodes
#   ("repeat", tag, B)          Engine.denoise, 40 steps, run to run: B = 1 and the three chunks of the identity tests; B = 4: graphs
#                               against eager steps on the items of the graph test
PARENT_MEASURED = {
    ("chain", "r84", 180): 1.63e-3, ("chain", "r84", 200): 1.66e-3, ("chain", "r8", 400): 1.86e-3,
    ("ddim", "r84", 180, 0.0): 8.98e-4, ("ddim", "r84", 180, 1.0): 1.70e-3, ("ddim", "r8", 400, 0.0): 1.12e-3, ("ddim", "r8", 400, 1.0): 1.82e-3,
    ("decode_lat", "r84", 180): 1.69e-3, ("decode_lat", "r8", 400): 2.18e-3, ("decode_wav", "r8", 400): 1.39e-3,
    ("repeat", "r84", 1): 3.25e-4, ("repeat", "r84", 3): 3.46e-4, ("repeat", "r8", 1): 5.09e-4, ("repeat", "r8", 3): 4.50e-4,
    ("repeat", "r84", 4): 4.07e-4,
}
_REF = {}


def bar(dtype, key, measured=None):
    m = PARENT_MEASURED.get(measured) if dtype == "bf16" else None
    return max(TOL[dtype][key], 2.0 * m) if m else TOL[dtype][key]


def close(dtype, key, value, what, measured=None):
    b = bar(dtype, key, measured)
    print(f"windows {dtype} {what}: {value:.3e} ({key} bar {b:.3e})")
    assert value < b, (dtype, key, what, value, b)


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32) if isinstance(x, np.ndarray) else x).float().cuda()


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def cover_count(Ltot, Lw, O_):
    starts, Lw = R.layout(Ltot, Lw, O_)
    n = np.zeros(Ltot, np.int64)
    for s in starts:
        n[s:s + Lw] += 1
    return n


# ------------------------------------------------------------------------------------------------------------ 1. one UNet pass
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", SHAPES)
def test_unet_forward_windows(tag, Ltot, Lw, O_, dtype):
    s = R.inputs(tag, Ltot, N)
    x = s["noise"][3] * 0.5 + s["img"]                                   # a state that is neither the start image nor noise alone
    ref = cached(("eps", tag, Ltot, Lw, O_), lambda: R.unet_forward_windows(s["sd"], s["u"], x, 37, s["cond"], Lw, O_, s["up"]))
    got = engine(tag, dtype).unet_forward_windows(x.cuda(), 37, s["cond"].cuda(), Lw, O_).cpu()
    close(dtype, "eps_small", rel(got.numpy(), ref.numpy()), f"{tag} {(Ltot, Lw, O_)} eps at t = 37")


# ------------------------------------------------------------------------------------------------------- 2. the loop, on a tape
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", SHAPES)
def test_denoise_windows_with_a_tape(tag, Ltot, Lw, O_, dtype):
    s = R.inputs(tag, Ltot, N)
    ref = R.reference(tag, Ltot, Lw, O_, N).numpy()
    got = engine(tag, dtype).denoise_windows(s["img"].cuda(), s["cond"].cuda(), N, Lw, O_, noise=s["noise"].cuda()).cpu().numpy()
    n = cover_count(Ltot, Lw, O_)
    scale = np.abs(ref).max()
    for what, m in (("singly covered", n == 1), ("multiply covered", n > 1)):
        print(f"windows {dtype} {tag} {(Ltot, Lw, O_)} {what} frames: {np.abs(got - ref)[..., m].max() / scale:.3e}")
    close(dtype, "chain_small", rel(got, ref), f"{tag} {(Ltot, Lw, O_)} {N}-step chain", ("chain", tag, Ltot))
    if (tag, Ltot) == ("r84", 180):
        # what the bar must see (tests/test_windows_cpu.py asserts the reference side): a hard switch on either engine; windows that
        # do not couple (8.2e-4 from the scheme) on the f32 engine -- the bf16 chain's own drift is of that size
        end, _ = R.reference(tag, Ltot, Lw, O_, N, mode="end")
        hard = R.reference(tag, Ltot, Lw, O_, N, mode="hard")
        for what, other in (("blended once at the end", end), ("hard switch", hard)):
            d = rel(got, other.numpy())
            print(f"windows {dtype} against the mutant '{what}': {d:.3e}")
            if dtype == "f32" or what == "hard switch":
                assert d > bar(dtype, "chain_small", ("chain", tag, Ltot)), (what, d)


# ---------------------------------------------------------------------------------------------------------- 3. the loop, Philox
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", MAIN)
def test_denoise_windows_draws_the_noise_of_one_item_of_Ltot_frames(tag, Ltot, Lw, O_, dtype):
    s = R.inputs(tag, Ltot, N)
    tape = cached(("philox", Ltot), lambda: torch.from_numpy(P.tape_steps(P.call_key(SEED, 0), N, 1, C, Ltot).astype(np.float32)))
    ref = cached(("philox ref", tag, Ltot, Lw, O_),
                 lambda: R.denoise_windows(s["sd"], s["u"], s["img"], s["cond"], N, tape, Lw, O_, s["up"])).numpy()
    e = engine(tag, dtype)
    img, cond = s["img"].cuda(), s["cond"].cuda()
    e.reseed(SEED)
    got = e.denoise_windows(img, cond, N, Lw, O_).cpu().numpy()
    close(dtype, "chain_small", rel(got, ref), f"{tag} {(Ltot, Lw, O_)} Philox against the reference's tape", ("chain", tag, Ltot))
    # the epoch moved on once, as for denoise: the next call draws what a B = 1 denoise of Ltot frames draws at epoch 1
    again = e.denoise_windows(img, cond, 6, Lw, O_).cpu().numpy()
    tape1 = cu(P.tape_steps(P.call_key(SEED, 1), 6, 1, C, Ltot))
    own = e.denoise_windows(img, cond, 6, Lw, O_, noise=tape1).cpu().numpy()
    close(dtype, "chain_small", rel(again, own), f"{tag} second call against the epoch-1 tape")
    tape0 = cu(P.tape_steps(P.call_key(SEED, 0), 6, 1, C, Ltot))
    assert rel(again, e.denoise_windows(img, cond, 6, Lw, O_, noise=tape0).cpu().numpy()) > 10 * TOL[dtype]["chain_small"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_drawing_windows_call_advances_the_epoch_once(dtype):
    """The windows call draws under the key of the context's epoch (it travels through the recording table) and moves the epoch on by
    one, as ldc_denoise does: the call and a plain decode behind it repeat after another reseed, and the decode draws at epoch 1."""
    tag, Ltot, Lw, O_ = MAIN[0]
    s = R.inputs(tag, Ltot, N)
    e = engine(tag, dtype)
    img, cond = s["img"].cuda(), s["cond"].cuda()
    wav = (torch.from_numpy(synth.synthetic_wav(1, Lw * CASES[tag][0].hop_length, seed=83)) * 0.5).cuda()

    def pair():
        e.reseed(SEED)
        return e.denoise_windows(img, cond, 6, Lw, O_).cpu().numpy(), e.decode(wav, 6, None).cpu().numpy()
    win0, dec0 = pair()
    win1, dec1 = pair()
    close(dtype, "repeat", rel(win1, win0), "the drawing windows call after another reseed", ("repeat", tag, 4))
    close(dtype, "repeat", rel(dec1, dec0), "the decode behind it after another reseed", ("repeat", tag, 1))
    e.reseed(SEED)
    at0 = e.decode(wav, 6, None).cpu().numpy()
    at1 = e.decode(wav, 6, None).cpu().numpy()
    close(dtype, "repeat", rel(dec0, at1), "the decode behind it against a decode at epoch 1", ("repeat", tag, 1))
    assert rel(dec0, at0) > 10 * bar(dtype, "repeat", ("repeat", tag, 1))       # (epoch 0 draws other noise)


# ------------------------------------------------------------------------------------------------------------ 4. the identities
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Lw", [("r84", 80), ("r8", 160)])
def test_one_window_is_denoise_at_batch_one(tag, Lw, dtype):
    s = R.inputs(tag, Lw, N)
    e = engine(tag, dtype)
    img, cond, noise = s["img"].cuda(), s["cond"].cuda(), s["noise"].cuda()
    ref = e.denoise(img, cond, N, noise).cpu().numpy()
    for lw in (Lw, 2 * Lw):                                               # Ltot == Lw and Ltot < Lw: one window of Ltot frames
        got = e.denoise_windows(img, cond, N, lw, 40, noise=noise).cpu().numpy()
        close(dtype, "repeat", rel(got, ref), f"{tag} W = 1 (Lw {lw}) against denoise at B = 1", ("repeat", tag, 1))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Lw", [("r84", 80), ("r8", 160)])
def test_overlap_zero_is_the_batch_of_independent_chunks(tag, Lw, dtype):
    s = R.inputs(tag, 3 * Lw, N)
    e = engine(tag, dtype)
    up = s["up"]
    cut = lambda x, n: torch.cat([x[..., k * n:(k + 1) * n] for k in range(3)], dim=-3).contiguous()      # noqa: E731
    ref = e.denoise(cut(s["img"], Lw).cuda(), cut(s["cond"], Lw // up).cuda(), N, cut(s["noise"], Lw).cuda()).cpu()
    ref = torch.cat(list(ref[:, None]), dim=-1).numpy()
    got = e.denoise_windows(s["img"].cuda(), s["cond"].cuda(), N, Lw, 0, noise=s["noise"].cuda()).cpu().numpy()
    close(dtype, "repeat", rel(got, ref), f"{tag} overlap 0 against denoise of the three chunks at B = 3", ("repeat", tag, 3))


# ------------------------------------------------------------------------------------------------------------------ 5. graphs
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replays_equal_eager_steps_and_stay_with_their_layout(dtype):
    tag, Ltot, Lw, O_ = "r84", 220, 80, 20                                # (a layout no other test uses: its first use is here)
    s, s2 = R.inputs(tag, Ltot, N), R.inputs(tag, 180, N)
    e = engine(tag, dtype)
    img, cond, noise = s["img"].cuda(), s["cond"].cuda(), s["noise"].cuda()
    img2, cond2, noise2 = s2["img"].cuda(), s2["cond"].cuda(), s2["noise"].cuda()
    W = len(R.layout(Ltot, Lw, O_)[0])
    assert W == len(R.layout(180, 80, 40)[0]) == 4                        # the other layout has the plan's (B, L, F) too
    # an ordinary denoise of the windows' shape (W, Lw), before and after
    ximg = torch.cat([img[..., k * Lw // 2:k * Lw // 2 + Lw] for k in range(W)]).contiguous()
    xcond = torch.cat([cond[..., k * 4:k * 4 + Lw // s["up"]] for k in range(W)]).contiguous()
    xnoise = torch.cat([noise[..., k * Lw // 2:k * Lw // 2 + Lw] for k in range(W)], dim=1).contiguous()
    plain0 = e.denoise(ximg, xcond, N, xnoise).clone()
    e.set_option("serial_parts", 1)
    try:
        eager = e.denoise_windows(img, cond, N, Lw, O_, noise=noise).clone()
        eager2 = e.denoise_windows(img2, cond2, N, 80, 40, noise=noise2).clone()
    finally:
        e.set_option("serial_parts", 0)
    first = e.denoise_windows(img, cond, N, Lw, O_, noise=noise).clone()  # the eager first step, the capture, replays
    other = e.denoise_windows(img2, cond2, N, 80, 40, noise=noise2).clone()
    torch.cuda.synchronize()
    syncs = L.load().ldc_debug_sync_count()
    replay = e.denoise_windows(img, cond, N, Lw, O_, noise=noise).clone()
    other2 = e.denoise_windows(img2, cond2, N, 80, 40, noise=noise2).clone()
    again = e.denoise_windows(img, cond, N, Lw, O_, noise=noise).clone()
    plain1 = e.denoise(ximg, xcond, N, xnoise).clone()
    torch.cuda.synchronize()
    assert L.load().ldc_debug_sync_count() == syncs                       # warm calls: no device-wide synchronisation
    for what, a, b in (("first use", first, eager), ("replay", replay, eager), ("replay again", again, eager),
                       ("the other layout", other, eager2), ("the other layout, replayed", other2, eager2),
                       ("an ordinary denoise of (W, Lw) before and after", plain1, plain0)):
        close(dtype, "repeat", rel(a.cpu().numpy(), b.cpu().numpy()), f"graphs: {what}", ("repeat", tag, 4))
    assert rel(eager.cpu().numpy()[..., :180], eager2.cpu().numpy()) > 10 * TOL[dtype]["repeat"]      # (two recordings, two results)


# -------------------------------------------------------------------------------------------------------------------- 6. DDIM
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", MAIN)
def test_ddim_sample_windows(tag, Ltot, Lw, O_, dtype, eta):
    s = R.inputs(tag, Ltot, N)
    times = L.ddim_times(T_START, S)
    ref = cached(("ddim", tag, Ltot, Lw, O_, eta),
                 lambda: R.ddim_windows(s["sd"], s["u"], s["img"], s["cond"], times, eta, s["noise"], Lw, O_, s["up"])).numpy()
    e = engine(tag, dtype)
    got = e.ddim_sample_windows(s["img"].cuda(), s["cond"].cuda(), T_START, S, Lw, O_, eta=eta, noise=s["noise"][:S].cuda()).cpu().numpy()
    close(dtype, "chain_small", rel(got, ref), f"{tag} {(Ltot, Lw, O_)} DDIM ({T_START}, {S}) eta {eta}", ("ddim", tag, Ltot, eta))
    if eta == 1.0:   # the draws are those of the tape: a run on another tape is another result
        off = e.ddim_sample_windows(s["img"].cuda(), s["cond"].cuda(), T_START, S, Lw, O_, eta=eta, noise=s["noise"][S:2 * S].cuda())
        assert rel(off.cpu().numpy(), ref) > 10 * bar(dtype, "chain_small", ("ddim", tag, Ltot, eta))


# ------------------------------------------------------------------------------------------------------------------ 7. decode
def decode_setup(tag, Ltot, Lw, O_):
    def make():
        mc, u, _ = CASES[tag]
        sdc, sdm = synth.to_torch(cond_sd_np()), synth.to_torch(main_sd_np(tag))
        wav = torch.from_numpy(synth.synthetic_wav(1, Ltot * mc.hop_length, seed=83)) * 0.5
        noise = R.inputs(tag, Ltot, N)["noise"]
        cond, codes, margins, _ = O.get_cond(sdc, COND_CFG, wav, None)
        img0 = O.start_image(sdm, u, cond)
        lat = R.denoise_windows(sdm, u, img0, cond, N, noise, Lw, O_, int(np.prod(u.upsampling_ratios)))
        out = O.output_normalise(O.seanet_decode(sdm, mc, lat))
        return dict(mc=mc, wav=wav, noise=noise, codes=codes, margins=margins, latents=lat, out=out)
    return cached(("decode", tag, Ltot, Lw, O_), make)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", MAIN)
def test_decode_windows(tag, Ltot, Lw, O_, dtype):
    d = decode_setup(tag, Ltot, Lw, O_)
    e = engine(tag, dtype)
    wav, noise = d["wav"].cuda(), d["noise"].cuda()
    got = e.decode_windows(wav, N, Lw, O_, noise=noise, want_stages=True)
    got = {k: v.clone() for k, v in got.items()}
    # the staged calls: get_cond and the normalised start image over the whole recording, the coupled loop, decoder, normalisation
    cond, codes = e.get_cond(wav, return_codes=True)
    lat = e.denoise_windows(e.cond_upsample(cond, 1), cond, N, Lw, O_, noise=noise)
    staged = e.output_normalise(e.decode_latents(L.MODEL_MAIN, lat))
    assert torch.equal(got["codes"], codes)
    safe = np.logical_and.accumulate(d["margins"].numpy() > 1e-3, axis=0)
    assert np.array_equal(got["codes"].cpu().numpy()[safe], d["codes"].numpy()[safe])
    close(dtype, "repeat", rel(got["cond"].cpu().numpy(), cond.cpu().numpy()), f"{tag} decode: cond against get_cond")
    close(dtype, "wav_small", rel(got["wav"].cpu().numpy(), staged.cpu().numpy()), f"{tag} decode: waveform against the staged calls")
    close(dtype, "chain_small", rel(got["latents"].cpu().numpy(), d["latents"].numpy()), f"{tag} decode: latents against the restatement", ("decode_lat", tag, Ltot))
    close(dtype, "wav_small", rel(got["wav"].cpu().numpy(), d["out"].numpy()), f"{tag} decode: waveform against the restatement", ("decode_wav", tag, Ltot))


def test_decode_ddim_windows_against_the_staged_calls():
    tag, Ltot, Lw, O_ = MAIN[0]
    d = decode_setup(tag, Ltot, Lw, O_)
    e = engine(tag, "f32")
    wav, noise = d["wav"].cuda(), d["noise"][:S].cuda()
    got = e.decode_ddim_windows(wav, T_START, S, Lw, O_, eta=1.0, noise=noise, want_stages=True)
    got = {k: v.clone() for k, v in got.items()}
    cond = e.get_cond(wav)
    lat = e.ddim_sample_windows(e.cond_upsample(cond, 1), cond, T_START, S, Lw, O_, eta=1.0, noise=noise)
    close("f32", "chain_small", rel(got["latents"].cpu().numpy(), lat.cpu().numpy()), "decode_ddim: latents against the staged calls")
    staged = e.output_normalise(e.decode_latents(L.MODEL_MAIN, lat))
    close("f32", "wav_small", rel(got["wav"].cpu().numpy(), staged.cpu().numpy()), "decode_ddim: waveform against the staged calls")


# --------------------------------------------------------------------------------------------------------------------- 8. CLI
def test_cli_chunk_overlap_writes_what_decode_windows_gives(tmp_path, capfd):
    from scipy.io import wavfile
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"))
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    steps, n = 10, 180 * 32 + 100                                         # trimmed to 5760 samples: 180 latent frames
    x = (synth.synthetic_wav(1, n, seed=84)[0, 0] * 0.5).astype(np.float32)
    wavfile.write(str(ind / "long.wav"), 16000, x)
    tape = torch.randn(steps, 1, 128, 180, generator=torch.Generator().manual_seed(9200))
    args = sample.build_parser().parse_args([
        "--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff", "--scaling_global",
        "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2", "--diff_dims", "32",
        "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", str(steps), "--dtype", "f32",
        "--chunk_sec", "0.16", "--chunk_overlap_sec", "0.08"])
    asked = []
    args.noise_provider = lambda keys, n_steps, Lz: (asked.append((keys, n_steps, Lz)), tape[:n_steps, :, :, :Lz])[1]
    assert len(sample.synthesis(args)) == 1
    assert asked == [([(0, 0)], steps, 180)]                              # one call, the whole recording: no independent chunks
    y = wavfile.read(str(outd / "long.wav"))[1]
    ref = engine("r84", "f32").decode_windows(torch.from_numpy(x[None, None, :5760]).cuda(), steps, 80, 40, noise=tape.cuda())
    assert y.shape == (5760,)
    close("f32", "wav_small", rel(y, ref.cpu().numpy()[0, 0]), "the CLI's file against Engine.decode_windows")
    assert "hard-joined" not in capfd.readouterr().err                    # four windows: one segment


# --------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_engine_usable():
    tag, Ltot, Lw, O_ = MAIN[0]
    s = R.inputs(tag, Ltot, N)
    e = engine(tag, "f32")
    img, cond, noise = s["img"].cuda(), s["cond"].cuda(), s["noise"].cuda()
    good = e.denoise_windows(img, cond, 3, Lw, O_, noise=noise).clone()
    calls = [
        (lambda: e.denoise_windows(img, cond, 3, Lw, 45, noise=noise), "overlap 45"),
        (lambda: e.denoise_windows(img, cond, 3, Lw, 50, noise=noise), "overlap 50"),
        # Ltot < Lw, Lw / 2 < overlap <= Ltot: refused on the caller's Lw, not on the one window of Ltot frames the call would run as
        (lambda: e.denoise_windows(img, cond, 3, 200, 110, noise=noise), "overlap 110: must be a multiple of up = 10 in [0, Lw / 2 = 100]"),
        (lambda: e.denoise_windows(img, cond, 3, 90, 40, noise=noise), "Lw 90"),                     # a multiple of up, not of the quantum
        (lambda: e.denoise_windows(img, cond[..., :17].contiguous(), 3, Lw, O_, noise=noise), "Ftot (17)"),
        (lambda: e.denoise_windows(img, cond, 0, Lw, O_, noise=noise), "n_steps 0"),
        (lambda: e.ddim_sample_windows(img, cond, 40, 41, Lw, O_), "n_steps"),
        (lambda: e.ddim_sample_windows(img, cond, 40, 8, Lw, O_, eta=1.5), "eta"),
        (lambda: e.unet_forward_windows(img, 1000, cond, Lw, O_), "t 1000"),
        (lambda: e.decode_windows(torch.zeros(1, 1, 180 * 32 + 32).cuda(), 3, Lw, O_), "T 5792"),
        (lambda: e.decode_windows(torch.zeros(1, 1, 180 * 32).cuda(), 3, Lw, 45), "overlap 45"),
    ]
    for call, word in calls:
        with pytest.raises(L.LdcError) as ei:
            call()
        assert ei.value.code == L.E_INVALID and word in str(ei.value), (word, str(ei.value))
        again = e.denoise_windows(img, cond, 3, Lw, O_, noise=noise)
        assert rel(again.cpu().numpy(), good.cpu().numpy()) < TOL["f32"]["repeat"], word
    long = torch.zeros(1, 128, 80 + 32 * 40).cuda()
    with pytest.raises(L.LdcError) as ei:
        e.unet_forward_windows(long, 5, torch.zeros(1, 128, long.shape[2] // 10).cuda(), 80, 40)
    assert ei.value.code == L.E_INVALID and "33 windows" in str(ei.value)
    with pytest.raises(ValueError):
        e.denoise_windows(torch.cat([img, img]), torch.cat([cond, cond]), 3, Lw, O_)                # one recording per call
    with pytest.raises(L.LdcError) as ei:
        engine(tag, "fp8").denoise_windows(img, cond, 3, Lw, O_, noise=noise)
    assert ei.value.code == L.E_INVALID and "fp8 engine" in str(ei.value)
