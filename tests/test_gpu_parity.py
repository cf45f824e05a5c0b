"""GPU parity tests: the HIP path, called through the C ABI (ctypes), against (a) the golden vectors
made by running the reference (tests/golden/) and (b) the CPU oracle on fresh seeded inputs.

Tolerances (relative to the max |reference|) are 2x the drift measured on MI355X (tests/drift_tolerances.py):
  f32 engine (exact-fp32 MFMA, v_mfma_f32_32x32x2_f32), bf16 engine (bf16 storage + MFMA, fp32 accumulate/state).
  The short chains here start at t <= 3 where eps hardly matters (they pin the golden vectors and the plumbing);
  tests/test_gpu_bench_shape.py holds the eps-sensitive and bench-shape checks.
  RVQ codes: bit-exact wherever the oracle's top-2 margin exceeds 1e-3 (all codec stages run fp32
  in both engines precisely so that the codes do not depend on the UNet dtype).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402
from helpers import CASES, COND_CFG, T, cond_sd_np, load_golden, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL, check  # noqa: E402


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------- L1 primitives
def test_sconv1d_against_reference_vectors():
    g = load_golden("primitives")
    e = engine("r84", "f32")
    names = sorted({k.split(".")[0] for k in g if k.startswith("c_")})
    ran = 0
    for n in names:
        k, s, d, causal = (int(v) for v in g[n + ".cfg"])
        w = O.fold_weight_norm(T(g[n + ".g"]), T(g[n + ".v"])).numpy()
        if g[n + ".x"].shape[-1] <= (k - 1) * d:
            with pytest.raises(L.LdcError):      # inputs shorter than the reflect pad: refused loudly
                e.sconv1d(cu(g[n + ".x"]), w, g[n + ".b"], stride=s, dilation=d, causal=bool(causal))
            continue
        y = e.sconv1d(cu(g[n + ".x"]), w, g[n + ".b"], stride=s, dilation=d, causal=bool(causal))
        assert y.shape == g[n + ".y"].shape
        assert rel(y.cpu().numpy(), g[n + ".y"]) < 1e-5, n
        ran += 1
    assert ran == 6


def test_sconvtranspose1d_against_reference_vectors():
    g = load_golden("primitives")
    e = engine("r84", "f32")
    for n in sorted({k.split(".")[0] for k in g if k.startswith("t_")}):
        k, s, d, causal = (int(v) for v in g[n + ".cfg"])
        w = O.fold_weight_norm(T(g[n + ".g"]), T(g[n + ".v"])).numpy() if (n + ".g") in g else g[n + ".w"]
        y = e.sconvtr1d(cu(g[n + ".x"]), w, g[n + ".b"], s, bool(causal))
        assert rel(y.cpu().numpy(), g[n + ".y"]) < 1e-5, n


@pytest.mark.parametrize("H,Tn,Bn", [(16, 11, 3), (64, 300, 3), (128, 160, 3), (512, 24, 3), (512, 120, 1), (256, 33, 2), (512, 17, 2), (512, 130, 32), (512, 40, 37),
                                     (256, 50, 20), (192, 9, 2)])
def test_slstm_all_kernel_variants(H, Tn, Bn):
    """H=64/128 take the register-resident kernel, H=256/512 the cooperative weight-stationary one (one or two
    16-item MFMA tiles, >32 items = two launches), anything else the L2-streaming one (seanet.hip)."""
    g = torch.Generator().manual_seed(H + Bn)
    b = 1.0 / np.sqrt(H)
    ws, sd = [], {}
    for layer in range(2):
        for nm, shape in (("weight_ih_l", (4 * H, H)), ("weight_hh_l", (4 * H, H)), ("bias_ih_l", (4 * H,)), ("bias_hh_l", (4 * H,))):
            w = (torch.rand(*shape, generator=g) * 2 - 1) * b
            ws.append(w.numpy()); sd[f"p.lstm.{nm}{layer}"] = w
    x = torch.randn(Bn, H, Tn, generator=g)
    ref = O.lstm_skip(x, sd, "p", 2)
    e = engine("r84", "f32")
    y = e.slstm(x.cuda(), ws, 2)
    assert rel(y.cpu().numpy(), ref.numpy()) < 2e-5
    if H in (256, 512):
        # round 5: one or two items take the XCD-local form by default (sixteen 1024-thread workgroups of one XCD, lstm_xcd_kernel); the
        # placement-independent cooperative kernel and the streamed one give the same sequence
        try:
            for opt, val in (("lstm_xcd", 0), ("lstm_stream", 1)):
                e.set_option(opt, val)
                y2 = e.slstm(x.cuda(), ws, 2)
                assert rel(y2.cpu().numpy(), ref.numpy()) < 2e-5, (opt, val)
        finally:
            e.set_option("lstm_xcd", 1)
            e.set_option("lstm_stream", 0)
    if H == 16:
        gold = load_golden("primitives")
        gw = [gold[f"lstm.sd.lstm.{nm}{layer}"] for layer in range(2) for nm in ("weight_ih_l", "weight_hh_l", "bias_ih_l", "bias_hh_l")]
        y = engine("r84", "f32").slstm(cu(gold["lstm.x"]), gw, 2)
        assert rel(y.cpu().numpy(), gold["lstm.y"]) < 1e-5


# ------------------------------------------------------------------------------------------- codec (config C1)
def test_codec_encode_rvq_decode_golden():
    g = load_golden("codec_c1")
    e = engine("r84", "f32")
    wav = cu(g["wav"])
    assert rel(e.encode(L.MODEL_COND, wav).cpu().numpy(), g["z"]) < 1e-4
    _, _, margins = O.rvq_forward(synth.to_torch(cond_sd_np()), T(g["z"]), 6)
    safe = margins.numpy() > 1e-3
    q, codes = e.rvq(cu(g["z"]), 6)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == g["codes"].shape
    assert np.array_equal(codes.cpu().numpy()[safe], g["codes"][safe])
    assert np.array_equal(codes.cpu().numpy(), g["codes"])          # and in fact everywhere on this fixture
    assert rel(q.cpu().numpy(), g["quantized"]) < 1e-6
    cond, codes2 = e.get_cond(wav, return_codes=True)
    assert np.array_equal(codes2.cpu().numpy()[safe], g["codes"][safe])
    cond15, codes15 = e.get_cond(wav, bandwidth=1.5, return_codes=True)
    assert codes15.shape[0] == 3 and np.array_equal(codes15.cpu().numpy(), g["codes_1p5"])
    assert rel(cond15.cpu().numpy(), g["quantized_1p5"]) < 1e-4
    assert rel(e.decode_latents(L.MODEL_COND, cu(g["quantized"])).cpu().numpy(), g["decoded"]) < 1e-4
    assert rel(e.rvq_decode(cu(g["codes"])).cpu().numpy(), g["quantized"]) < 1e-6


def test_codec_round_trip_full_size_c1():
    """BASELINE configs[0] at its full size: encode -> RVQ -> cond-codec decode of one 2.4 s clip (F = 120 frames) against the
    REFERENCE (tests/golden/codec_c1_full.npz, tools/gen_golden_c1.py; model.py:223-231, seanet.py:157-248).  The 0.4 s fixture
    never ran the decoder's cooperative LSTM (H = 512) over 120 frames or the k16 s8 transposed conv at that length."""
    g = load_golden("codec_c1_full")
    e = engine("r84", "f32")
    _, Tn, seed_in = (int(v) for v in g["meta"])
    wav = (torch.from_numpy(synth.synthetic_wav(1, Tn, seed=seed_in)) * 0.5).cuda()
    z = e.encode(L.MODEL_COND, wav)
    assert rel(z.cpu().numpy(), g["z"]) < 1e-4
    cond, codes = e.get_cond(wav, return_codes=True)
    assert tuple(codes.shape) == g["codes"].shape and np.array_equal(codes.cpu().numpy(), g["codes"]), "RVQ codes must be bit-exact"
    assert rel(cond.cpu().numpy(), g["quantized"]) < 1e-5
    dec = e.decode_latents(L.MODEL_COND, cu(g["quantized"]))
    assert dec.shape[-1] == Tn and rel(dec.cpu().numpy(), g["decoded"]) < 1e-4
    # and the streamed LSTM kernel (the fallback of the cooperative one) at the same length
    e.set_option("lstm_stream", 1)
    try:
        assert rel(e.decode_latents(L.MODEL_COND, cu(g["quantized"])).cpu().numpy(), g["decoded"]) < 1e-4
    finally:
        e.set_option("lstm_stream", 0)
    # round 5: the few-tile long-K convs (k16 s8 256 -> 512, k7 512 -> 128, the first transposed convs) split K on the generic
    # kernel (conv_splitk_reduce_kernel adds the slices in order); the unsplit launches must agree with them and with the reference
    e.set_option("sea_splitk", 0)
    try:
        z0 = e.encode(L.MODEL_COND, wav)
        dec0 = e.decode_latents(L.MODEL_COND, cu(g["quantized"]))
        assert rel(z0.cpu().numpy(), g["z"]) < 1e-4 and rel(dec0.cpu().numpy(), g["decoded"]) < 1e-4
        assert not torch.equal(z0, z), "split-K did not engage (or the option is ignored)"
        assert rel(z0.cpu().numpy(), z.cpu().numpy()) < 1e-5 and rel(dec0.cpu().numpy(), dec.cpu().numpy()) < 1e-5
    finally:
        e.set_option("sea_splitk", 1)


def test_rvq_ties_take_first_index():
    """Duplicate code vectors: the reference's argmax returns the first maximum (core_vq.py:181)."""
    e = engine("r84", "f32")
    sd = synth.to_torch(cond_sd_np())
    emb = sd["quantizer.vq.layers.0._codebook.embed"]
    z = emb[[5, 900, 17]].t().reshape(1, 128, 3).contiguous()       # exactly on code vectors
    _, codes = e.rvq(z.cuda(), 1)
    assert codes.cpu().numpy().reshape(-1).tolist() == [5, 900, 17]


@pytest.mark.parametrize("Bn,Fn,n_q", [(1, 120, 6), (3, 121, 5), (16, 120, 6), (2, 7, 3)])
def test_rvq_tiled_kernel_equals_the_round1_kernel_bit_for_bit(Bn, Fn, n_q):
    """Round 5: the LDS-tiled search (rvq_tiled_kernel: lane = code, the rows' residual as v_readlane scalars; one or two rows per
    wave by row count) keeps the arithmetic of the round-1 kernel per (row, code) -- same FMA chain, same distance expression, first
    maximum -- so codes AND quantised rows are identical, ragged row counts included; and both follow the oracle where its margin
    between the best two codes is not a rounding matter (core_vq.py:174-189, 324-342)."""
    e = engine("r84", "f32")
    gen = torch.Generator().manual_seed(100 + Bn * Fn)
    z = torch.randn(Bn, 128, Fn, generator=gen) * 0.7
    q1, c1 = e.rvq(z.cuda(), n_q)
    e.set_option("rvq_tiled", 0)
    try:
        q0, c0 = e.rvq(z.cuda(), n_q)
    finally:
        e.set_option("rvq_tiled", 1)
    assert torch.equal(c0, c1) and torch.equal(q0, q1)
    qo, co, margins = O.rvq_forward(synth.to_torch(cond_sd_np()), z, n_q)
    safe = np.logical_and.accumulate(margins.numpy() > 1e-3, axis=0)     # (a code picked differently changes every later stage of its row)
    assert safe.mean() > 0.9 and np.array_equal(c1.cpu().numpy()[safe], co.numpy()[safe])


# ------------------------------------------------------------------------------------------- UNet / diffusion
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_unet_forward_and_taps(tag, dtype):
    g = load_golden("ladiff_" + tag)
    mc, u, _ = CASES[tag]
    e = engine(tag, dtype)
    cond, x = cu(g["cond"]), cu(g["x"])
    for t in (0, 37):
        check(dtype, "eps_small", rel(e.unet_forward(x, t, cond).cpu().numpy(), g[f"eps_t{t}"]), (tag, t))
    taps = {}
    O.unet_forward(synth.to_torch(main_sd_np(tag)), u, T(g["x"]), torch.full((2,), 37, dtype=torch.long), T(g["cond"]), taps=taps)
    for name in ["cond_proc", "init", "down0", "down4", "mid", "up0", "up4"]:
        check(dtype, "eps_small", rel(e.debug_tap(name, taps[name].shape).cpu().numpy(), taps[name].numpy()), (tag, name))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_sampler_chain_and_stage_tensors(tag, dtype):
    g = load_golden("ladiff_" + tag)
    mc, u, _ = CASES[tag]
    e = engine(tag, dtype)
    cond, x = cu(g["cond"]), cu(g["x"])
    n = int(g["meta"][2])
    noises = cu(g["noises"])
    assert rel(e.cond_upsample(cond, 0).cpu().numpy(), g["img_up"]) < 1e-5
    assert rel(e.cond_upsample(cond, 1).cpu().numpy(), g["img0"]) < 1e-5
    check(dtype, "chain_small", rel(e.p_sample(x, 5, cond, noises[n - 1]).cpu().numpy(), g["p_sample_t5"]), tag)
    lat = e.denoise(cu(g["img0"]), cond, n, noises)                   # first call: eager step + graph capture
    check(dtype, "chain_small", rel(lat.cpu().numpy(), g["latents"]), tag)
    lat2 = e.denoise(cu(g["img0"]), cond, n, noises)                  # second call: graph replay
    check(dtype, "repeat", rel(lat2.cpu().numpy(), lat.cpu().numpy()), tag)
    assert rel(e.decode_latents(L.MODEL_MAIN, cu(g["latents"])).cpu().numpy(), g["wav_raw"]) < 1e-4
    assert rel(e.output_normalise(cu(g["wav_raw"])).cpu().numpy(), g["wav_out"]) < 1e-5
    out = e.decode(cu(g["wav"]), n, noises, per_item=False, want_stages=True)
    assert rel(out["cond"].cpu().numpy(), g["cond"]) < 1e-4
    check(dtype, "chain_small", rel(out["latents"].cpu().numpy(), g["latents"]), tag)
    check(dtype, "wav_small", rel(out["wav"].cpu().numpy(), g["wav_out"]), tag)


def test_graph_replay_equals_eager_many_steps():
    """hipGraph replay (n>=3) vs per-step eager calls through ldc_p_sample, same injected noise."""
    tag = "r84"
    g = load_golden("ladiff_" + tag)
    e = engine(tag, "f32")
    cond = cu(g["cond"])
    n = 9
    noises = torch.randn(n, *g["x"].shape, generator=torch.Generator().manual_seed(3)).cuda()
    x = cu(g["img0"]).clone()
    ref = x.clone()
    for j, t in enumerate(reversed(range(n))):
        ref = e.p_sample(ref, t, cond, noises[j])
    got = e.denoise(x, cond, n, noises)
    assert rel(got.cpu().numpy(), ref.cpu().numpy()) < 1e-6


def test_philox_noise_is_standard_normal_and_seeded():
    tag = "r84"
    g = load_golden("ladiff_" + tag)
    e = engine(tag, "f32")
    cond = cu(g["cond"])
    x0 = cu(g["img0"])
    e.reseed(0)
    a = e.denoise(x0, cond, 6, None)
    e.reseed(0)
    b = e.denoise(x0, cond, 6, None)
    # same seed, same call counter, same step indices -> same draws (fp32 atomics in the GroupNorm / attention
    # reductions make the two runs agree to rounding, not bit for bit)
    assert rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
    assert torch.isfinite(a).all()
    # one step from zeros with eps-independent part removed: x_new - mean = sigma * z
    x = torch.zeros_like(x0)
    y1 = e.p_sample(x, 500, cond, None)
    y0 = e.p_sample(x, 500, cond, torch.zeros_like(x))
    sched = synth.cosine_schedule_buffers(1000)
    z = ((y1 - y0) / float(np.exp(0.5 * sched["posterior_log_variance_clipped"][500]))).cpu().numpy().ravel()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert abs(((z ** 4).mean()) - 3.0) < 0.15


# ------------------------------------------------------------------------------------------- full-size properties (BASELINE configs[1] shapes)
def test_full_size_items_are_independent():
    """C2 shapes at reduced width: decoding a batch equals decoding each utterance alone (per-item
    normalisation) -- the property the data-parallel sharding relies on."""
    tag = "r84"
    mc, u, _ = CASES[tag]
    e = engine(tag, "f32")
    Tn = 38400
    wav = torch.from_numpy(synth.synthetic_wav(3, Tn, seed=9)).cuda()
    n = 3
    noise = torch.randn(n, 3, 128, Tn // mc.hop_length, generator=torch.Generator().manual_seed(1)).cuda()
    full = e.decode(wav, n, noise, per_item=True, want_stages=True)
    for i in range(3):
        one = e.decode(wav[i:i + 1], n, noise[:, i:i + 1].contiguous(), per_item=True, want_stages=True)
        assert torch.equal(one["codes"], full["codes"][:, i:i + 1])
        assert rel(one["latents"].cpu().numpy(), full["latents"][i:i + 1].cpu().numpy()) < 1e-5
        assert rel(one["wav"].cpu().numpy(), full["wav"][i:i + 1].cpu().numpy()) < 1e-4
    w = full["wav"].cpu().numpy()
    assert np.allclose(np.abs(w).reshape(3, -1).max(1), 1.0, atol=1e-5)      # sample.py:134 leaves max|x| = 1


def test_error_behaviour():
    e = engine("r84", "f32")
    g = load_golden("ladiff_r84")
    with pytest.raises(L.LdcError):                      # L != F * prod(upsampling_ratios)
        e.unet_forward(cu(g["x"])[:, :, :150].contiguous(), 3, cu(g["cond"]))
    with pytest.raises(L.LdcError):                      # t outside the 1000-step schedule
        e.unet_forward(cu(g["x"]), 1000, cu(g["cond"]))
    from ladiffcodec_amd.model import Engine
    mc, u, _ = CASES["r84"]
    bad = Engine(mc, u, COND_CFG, dtype="f32")
    sd = main_sd_np("r84")
    sd.pop("diff_model.final_conv.bias"); sd.pop("diffusion.model.final_conv.bias")
    bad.load_state_dict(L.MODEL_MAIN, sd)
    bad.load_state_dict(L.MODEL_COND, cond_sd_np())
    with pytest.raises(L.LdcError, match="final_conv.bias"):   # strict load names the missing key
        bad.finalize(strict=True)
    bad.close()


@pytest.mark.parametrize("code,tag,option", [(1, "[coop_lstm]", "lstm_stream"), (2, "[gn_wait]", "fuse_gn_epi"), (4, "[ctx_range]", "fold_ctx")])
def test_device_side_failure_fallback(code, tag, option):
    """A kernel whose bounded in-launch wait gave up raises the host-mapped flag; the next call fails with LDC_E_HIP and a
    tagged message, and the CLI's decode_with_retry applies the matching fallback and decodes the batch again (ADVICE r3:
    the fallback keyed on a string the message did not contain).  The flag is raised through the debug hook."""
    from ladiffcodec_amd import sample as cli
    from ladiffcodec_amd.model import Engine
    mc, u, _ = CASES["r84"]
    e = Engine(mc, u, COND_CFG, dtype="f32")
    e.load_state_dict(L.MODEL_MAIN, main_sd_np("r84"))
    e.load_state_dict(L.MODEL_COND, cond_sd_np())
    e.finalize(strict=True)
    wav = torch.from_numpy(synth.synthetic_wav(2, 5120, seed=5)).cuda()
    ref = e.decode(wav, 2, noise=None, per_item=True).cpu()
    e.reseed(0)
    e.debug_raise_failure(code)
    with pytest.raises(L.LdcError, match="device-side failure") as ei:
        e.decode(wav, 2, noise=None, per_item=True)
    assert ei.value.code == L.E_HIP and tag in str(ei.value)
    # the flag was consumed by that call; raise it again and let the CLI helper recover
    e.debug_raise_failure(code)
    calls = []
    real = e.set_option
    e.set_option = lambda n, v: (calls.append((n, v)), real(n, v))[1]
    out = cli.decode_with_retry(e, wav, 2, None, True).cpu()
    assert calls == [(option, 1 if option == "lstm_stream" else 0)]
    assert bool(torch.isfinite(out).all()) and out.shape == ref.shape
    e.close()


def test_cli_synthesis_end_to_end(tmp_path):
    """`python -m srcs.sample`-equivalent run: .amlt checkpoints (one DDP-prefixed), wav files in a tree,
    batching by length; with --midway_t 1 the sampler draws no noise (t = 0), so the written audio must equal
    the oracle's decode of the same file."""
    from scipy.io import wavfile
    from ladiffcodec_amd import sample as cli
    mc, u, seed = CASES["r84"]
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind, outd = tmp_path / "in", tmp_path / "out"
    (ind / "spk1").mkdir(parents=True)
    wavs = {"spk1/a.wav": synth.synthetic_wav(1, 5120 + 100, seed=1)[0, 0], "spk1/b.wav": synth.synthetic_wav(1, 5120, seed=2)[0, 0],
            "c.wav": synth.synthetic_wav(1, 2560, seed=3)[0, 0]}   # lengths: multiples of lcm(640, 32*16) so that L survives 4 halvings
    for name, x in wavs.items():
        wavfile.write(str(ind / name), 16000, (x * 0.5).astype(np.float32))
    args = cli.build_parser().parse_args([
        "--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff",
        "--scaling_global", "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
        "--diff_dims", "32", "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", "1", "--dtype", "f32"])
    written = cli.synthesis(args)
    assert len(written) == 3
    sd_c, sd_m = synth.to_torch(cond_sd_np()), synth.to_torch(main_sd_np("r84"))
    for name, x in wavs.items():
        sr, y = wavfile.read(str(outd / name))
        n = len(x) // 640 * 640
        assert sr == 16000 and y.shape == (n,) and y.dtype == np.float32
        ref = O.decode_utterances(sd_c, COND_CFG, sd_m, mc, u, T((x[:n] * 0.5).astype(np.float32)).reshape(1, 1, n), 1, None)
        assert rel(y, ref["wav"].numpy().reshape(-1)) < 5e-3, name


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_full_width_unet_step_against_oracle(dtype):
    """BASELINE configs[1] widths (diff_dims=256: 256/512/1024 channels, all-128-wide tiles, 2-chunk 1x1 units,
    64x64 small-grid tiles), short latent so that the CPU oracle finishes in seconds."""
    from ladiffcodec_amd.model import Engine
    from ladiffcodec_amd.spec import CodecConfig, UnetConfig
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
    sd = synth.ladiff_state_dict(mc, u, seed=5)
    e = Engine(mc, u, COND_CFG, dtype=dtype)
    e.load_state_dict(L.MODEL_MAIN, {k: v for k, v in sd.items() if not k.startswith("diffusion.model.")})
    e.load_state_dict(L.MODEL_COND, cond_sd_np())
    e.finalize(strict=True)
    g = torch.Generator().manual_seed(17)
    B, Lz, F = 3, 320, 32
    x = torch.randn(B, 128, Lz, generator=g) * 0.7
    cond = torch.randn(B, 128, F, generator=g)
    t = 23
    ref = O.unet_forward(synth.to_torch(sd), u, x, torch.full((B,), t, dtype=torch.long), cond)
    got = e.unet_forward(x.cuda(), t, cond.cuda()).cpu()
    check(dtype, "eps_bench", rel(got.numpy(), ref.numpy()), "B3_L320")
    # two sampler steps with injected noise through the captured-graph path (n >= 3 steps)
    n = 3
    noise = torch.randn(n, B, 128, Lz, generator=g)
    img = torch.randn(B, 128, Lz, generator=g).clamp(-1, 1) * 0.5
    want = O.halfway_sampling(synth.to_torch(sd), u, img, cond, n, noise)
    have = e.denoise(img.cuda(), cond.cuda(), n, noise.cuda()).cpu()
    check(dtype, "chain_small", rel(have.numpy(), want.numpy()), "full width")
    e.close()


# ------------------------------------------------------------------------------------------- other samplers
def test_p_sample_loop_and_infilling_drivers():
    """diffusion.p_sample_loop (1000 steps, 5 per replayed graph) and diffusion.infilling through the C ABI against the
    reference's runs (tests/golden/drivers_r84.npz) with injected start images and noise tapes; then the device-drawn
    (Philox) variants: finite, bounded, reproducible."""
    from helpers import driver_noises
    g = load_golden("drivers_r84")
    e = engine("r84", "f32")
    loop_noise, fill_noise, midway_t = driver_noises(g)
    cond = cu(g["cond"])
    got = e.p_sample_loop(cond, img=cu(g["loop_img0"]), noise=loop_noise.cuda())
    assert rel(got.cpu().numpy(), g["loop_out"]) < 2e-3
    img, infill = e.infilling(cu(g["fill_infill0"]), cond, midway_t, lam=0.8, img=cu(g["fill_img0"]), noise=fill_noise.cuda())
    assert rel(img.cpu().numpy(), g["fill_out"]) < 1e-4
    # facade with the reference's names
    from ladiffcodec_amd.model import DiffAudioRep
    m = DiffAudioRep(e, L.MODEL_MAIN)
    same = m.diffusion.infilling(cu(g["fill_infill0"]), cond, midway_t=midway_t, lam=0.8, img=cu(g["fill_img0"]), noises=fill_noise.cuda())
    assert torch.equal(same, img) or rel(same.cpu().numpy(), img.cpu().numpy()) < 1e-5
    # device-side start images and draws
    e.reseed(5)
    a = e.infilling(cu(g["fill_infill0"]), cond, 4)[0]
    e.reseed(5)
    b = e.infilling(cu(g["fill_infill0"]), cond, 4)[0]
    assert torch.isfinite(a).all() and rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
    m.diffusion.seq_length = g["loop_img0"].shape[2]
    s1 = m.diffusion.sample(batch_size=1, condition=cond)
    assert s1.shape == (1, 128, g["loop_img0"].shape[2]) and torch.isfinite(s1).all() and float(s1.abs().max()) <= 1.0 + 1e-4


def test_long_utterance_beyond_one_attention_chunk():
    """17.9 s in one piece: latent L = 8960, bottleneck attention over n = 560 positions (three K/V chunks in LDS),
    1792 LSTM steps in the cond codec; one UNet call against the oracle, then a short decode end to end."""
    mc, u, _ = CASES["r84"]
    e = engine("r84", "f32")
    Tn = 286720
    Lz, F = Tn // mc.hop_length, Tn // COND_CFG.hop_length
    g = torch.Generator().manual_seed(99)
    x = torch.randn(1, 128, Lz, generator=g) * 0.7
    cond = torch.randn(1, 128, F, generator=g)
    sd = synth.to_torch(main_sd_np("r84"))
    ref = O.unet_forward(sd, u, x, torch.full((1,), 11, dtype=torch.long), cond)
    got = e.unet_forward(x.cuda(), 11, cond.cuda()).cpu()
    assert rel(got.numpy(), ref.numpy()) < 2e-4
    wav = torch.from_numpy(synth.synthetic_wav(1, Tn, seed=5))
    out = e.decode(wav.cuda(), 3, per_item=True)
    assert out.shape == (1, 1, Tn) and torch.isfinite(out).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bench_workload_items_against_oracle(dtype):
    """The exact bench.py workload shape (BASELINE configs[1]: diff_dims 256, enc_ratios 8 4, 32 x 2.4 s, two batch
    parts of 16) with 2 denoise steps and injected noise: two of the 32 decoded utterances (one from each part)
    against the CPU oracle decoding them alone.  This runs every kernel configuration the benchmark runs
    (128x64 / 64x64 tiles, split-K at the L=75 level, fused statistics, MFMA attention, cooperative LSTM)."""
    from ladiffcodec_amd.model import Engine
    from ladiffcodec_amd.spec import CodecConfig, UnetConfig
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
    sd = synth.ladiff_state_dict(mc, u, seed=1)
    sdc = cond_sd_np()
    e = Engine(mc, u, COND_CFG, dtype=dtype)
    e.load_state_dict(L.MODEL_MAIN, {k: v for k, v in sd.items() if not k.startswith("diffusion.model.")})
    e.load_state_dict(L.MODEL_COND, sdc)
    e.finalize(strict=True)
    B, Tn, n = 32, 38400, 3
    wav = torch.from_numpy(synth.synthetic_wav(B, Tn, seed=1234))
    noise = torch.randn(n, B, 128, Tn // mc.hop_length, generator=torch.Generator().manual_seed(8))
    got = e.decode(wav.cuda(), n, noise.cuda(), per_item=True, want_stages=True)
    sd_t, sdc_t = synth.to_torch(sd), synth.to_torch(sdc)
    for i in (3, 29):
        ref = O.decode_utterances(sdc_t, COND_CFG, sd_t, mc, u, wav[i:i + 1], n, noise[:, i:i + 1], per_item=True)
        assert torch.equal(got["codes"][:, i:i + 1].cpu(), ref["codes"]), "RVQ codes must be bit-exact"
        check(dtype, "chain_small", rel(got["latents"][i:i + 1].cpu().numpy(), ref["latents"].numpy()), i)
        check(dtype, "wav_small", rel(got["wav"][i:i + 1].cpu().numpy(), ref["wav"].numpy()), i)
    e.close()


# ------------------------------------------------------------------------------------------- pipelined conv-GEMM vs generic kernel
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_conv_fast_every_tile_shape_against_generic_kernel(dtype):
    """ldc_conv_compare: the same layer and pseudo-random operands through conv_fast.inc with every tile shape forced
    (64x64, 128x64, and the launcher's own choice incl. split-K; the 128x128 tiles were removed in round 6) and through the generic kernel (conv_gemm.hip, which
    the SConv1d vectors of the reference pin): outputs, fused GroupNorm statistics (unet.py:142-147), fused k column maxima
    (unet.py:214) and the residual epilogue.  Shapes: the UNet's layer classes incl. two-input (concatenated) convs, k = 1/3/4/7,
    stride 2, folded nearest upsampling, ragged row counts (B * L not a multiple of any tile)."""
    import ctypes as C
    e = engine("r84", dtype)
    lib, ctx = e.lib, e._ctx
    dt = L.LDC_F32 if dtype == "f32" else L.LDC_BF16
    tol_out = 1e-5 if dtype == "f32" else 1.0 / 128          # one bf16 ulp of the largest output
    shapes = [  # L, cin1, cin2, cout, k, stride, ups
        (1200, 256, 0, 256, 3, 1, 0), (600, 512, 256, 512, 3, 1, 0), (150, 1024, 512, 1024, 3, 1, 0), (75, 1024, 1024, 1024, 3, 1, 0),
        (75, 1024, 0, 1024, 3, 1, 0), (1200, 256, 0, 384, 1, 1, 0), (300, 512, 512, 512, 1, 1, 0), (1200, 128, 128, 256, 7, 1, 0),
        (600, 256, 0, 512, 4, 2, 0), (75, 1024, 0, 1024, 3, 1, 1), (77, 256, 0, 128, 1, 1, 0), (53, 512, 0, 512, 3, 1, 0),
    ]
    for Lx, c1, c2, co, k, st, ups in shapes:
        for cfg in (-1, 0, 1):
            for B in (3, 16):
                if B == 16 and (cfg != -1 or Lx > 300):
                    continue
                d, m, r = C.c_double(), C.c_double(), C.c_double()
                L.check(lib.ldc_conv_compare(ctx, dt, B, Lx, c1, c2, co, k, st, ups, cfg, 1 if k == 3 and st == 1 else 0, 1 if k == 1 else 0,
                                             1 if cfg in (-1, 1) and st == 1 and not ups else 0, C.byref(d), C.byref(m), C.byref(r)))
                assert m.value > 0.1 and d.value <= tol_out * m.value, (dtype, Lx, c1, c2, co, k, st, ups, cfg, B, d.value, m.value)
                assert r.value < 1e-4, ("fused statistics", dtype, Lx, c1, c2, co, k, cfg, B, r.value)


def test_conv_fp8_x_fp8_mfma_against_bf16_path_on_the_e4m3_grid():
    """ldc_conv_compare_fp8: the fp8 x fp8 conv-GEMM (v_mfma_scale_f32_32x32x64_f8f6f4, 64 channels per LDS row) against the
    bf16-activation x fp8-weight kernel on operands drawn ON the e4m3 grid -- both compute the same products exactly and may
    differ by the fp32 summation order only: at most one bf16 ulp of the largest output, fused statistics to 1e-4."""
    import ctypes as C
    e = engine("r84", "bf16")
    lib, ctx = e.lib, e._ctx
    shapes = [  # L, cin1, cin2, cout, k, stride, ups
        (1200, 256, 0, 256, 3, 1, 0), (300, 512, 0, 512, 3, 1, 0), (75, 1024, 0, 1024, 3, 1, 0), (1200, 256, 0, 384, 1, 1, 0),
        (75, 1024, 0, 384, 1, 1, 0), (1200, 256, 0, 128, 1, 1, 0), (160, 64, 0, 64, 3, 1, 0), (53, 128, 64, 128, 3, 1, 0),
    ]
    for Lx, c1, c2, co, k, st, ups in shapes:
        for B in (3, 16):
            if B == 16 and Lx > 300:
                continue
            d, m, r = C.c_double(), C.c_double(), C.c_double()
            L.check(lib.ldc_conv_compare_fp8(ctx, B, Lx, c1, c2, co, k, st, ups, 1 if k == 3 else 0, 1 if k == 1 else 0,
                                             C.byref(d), C.byref(m), C.byref(r)))
            assert m.value > 0.1 and d.value <= m.value / 128, (Lx, c1, c2, co, k, B, d.value, m.value)
            # GroupNorm sums agree to 1e-4; a column MAXIMUM is one of the (bf16-rounded) outputs and may differ by their one ulp
            assert r.value < (1.0 / 128 if k == 1 else 1e-4), ("fused statistics", Lx, c1, c2, co, k, B, r.value)


def test_rccl_world_size_one_group_runs_every_collective_path():
    """The RCCL code paths of parallel.py -- flat checkpoint broadcast, result all_gather, and the training row's
    reduce_scatter + all_gather of a flat gradient buffer whose length needs padding -- on a world-size-1 `nccl` group on the
    GPU: no 8-GPU node has been available to any round, so this is the first time these exact calls run on the hardware
    (the 2-rank semantics are covered under gloo in tests/test_cli_and_parallel_cpu.py).  Own process: a failed RCCL
    bring-up must not take the suite's CUDA context with it."""
    import os, subprocess, sys, textwrap
    code = textwrap.dedent("""
        import os, sys
        import numpy as np, torch, torch.distributed as dist
        sys.path.insert(0, os.getcwd())
        from ladiffcodec_amd import parallel
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29631")
        rank, local_rank, world = parallel.init_process_group("nccl")
        assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(0)
        layout = [("a.weight", (7, 5, 3)), ("a.bias", (7,)), ("scalar", ())]
        sd = {k: rng.standard_normal(s).astype(np.float32) for k, s in layout}
        out = parallel.broadcast_state_dict(sd, layout, device=dev)
        assert all(np.array_equal(out[k], sd[k]) for k, _ in layout)
        x = torch.randn(3, 1, 1000, device=dev)
        got = parallel.gather_results(x, world)
        assert len(got) == 1 and torch.equal(got[0], x)
        g = torch.randn(1003, device=dev)                 # 1003 % 4 != 0: the padded reduce_scatter / all_gather path
        ref = g.clone()
        parallel.allreduce_gradients(g, average=True, force_collective=True)
        assert torch.equal(g, ref), float((g - ref).abs().max())
        assert abs(parallel.max_over_ranks(3.25, device=dev) - 3.25) < 1e-12
        dist.barrier()
        dist.destroy_process_group()
        print("RCCL_OK")
    """)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_warm_decode_never_waits_for_the_device():
    """include/ladiffcodec.h: asynchronous stage calls on a caller's stream issue no device-wide synchronisation once the plans of a
    shape are built and its step graphs captured (eleven hipDeviceSynchronize sites in ldc_api.cpp, all claimed to be
    cold paths, nothing tested it).  Every such call goes through a counter: it must not move across warm decodes -- single UNet
    calls, sampler calls and whole decodes, on both graph arrangements' default."""
    e = engine("r84", "bf16")
    lib = L.load()
    wav = torch.from_numpy(synth.synthetic_wav(4, 5120, seed=9)).cuda()
    g = load_golden("ladiff_r84")
    x, cond = cu(g["x"]), cu(g["cond"])
    for _ in range(2):                                   # cold: plans, graphs, scratch
        e.decode(wav, 7, noise=None, per_item=True)
        e.unet_forward(x, 5, cond)
        e.denoise(cu(g["img0"]), cond, 6)
    torch.cuda.synchronize()
    before = lib.ldc_debug_sync_count()
    for _ in range(3):
        e.decode(wav, 7, noise=None, per_item=True)
        e.unet_forward(x, 5, cond)
        e.denoise(cu(g["img0"]), cond, 6)
    torch.cuda.synchronize()
    assert lib.ldc_debug_sync_count() == before, (before, lib.ldc_debug_sync_count())


def test_folded_layernorm_on_rows_with_a_large_mean():
    """the PreNorm LayerNorm folded into to_qkv (unet.py:82-101: biased variance ABOUT THE MEAN) took its variance as
    E[x^2] - mean^2 from single-pass fp32 sums, which cancels where |mean| >> std.  The statistics are centred now (two passes
    over rows read by the conv itself, Chan-merged (sum, M2) partials per 32-column block from the producing conv): rows with
    mean / std ~ 170 through the folded conv, against launch_ln_rows + a plain conv.  The fold's own rearrangement
    rstd * (W x - mean * s_n) loses log10(mean / std) digits of an fp32 accumulator, hence 2e-3 rather than 2e-5 at dc = 100
    (the single-pass variance was off by 10 % there).
    Both pipelined kernels take the row statistics, the LayerNorm apply and the split-K sum from the same functions (conv_device.h),
    so the tests that hold one kernel against the other cannot see a mistake there: the fold runs on conv_fast_kernel (option
    conv_lean 0) and on conv_lean_kernel (1), each against launch_ln_rows + a plain conv, and so does one split-K conv (B = 1,
    L = 75, 1024 -> 1024, k = 3 on the 128 x 64 tile, both dtypes) against the generic kernel, with the bounds of
    test_conv_fast_every_tile_shape_against_generic_kernel.  ldc_debug_lean_launches says which kernel ran."""
    import ctypes as C
    e = engine("r84", "f32")
    lib = L.load()
    K3, K1_LN = 0, 2                                     # ldc_debug_lean_launches: unit kinds (conv_lean.inc)

    def lean_counts():
        return [lib.ldc_debug_lean_launches(i) for i in range(7)]

    try:
        for lean in (0, 1):
            e.set_option("conv_lean", lean)
            for dtype, dc, tol in ((L.LDC_F32, 0.0, 2e-5), (L.LDC_F32, 100.0, 2e-3), (L.LDC_BF16, 2.0, 3e-2)):
                for C_, n_out in ((256, 384), (1024, 384)):
                    d = (C.c_double * 2)()
                    m = C.c_double()
                    before = lean_counts()
                    L.check(lib.ldc_ln_fold_compare(e._ctx, dtype, 300, C_, n_out, dc, d, C.byref(m)))
                    ran = [a - b for a, b in zip(lean_counts(), before)]
                    print("ln fold", lean, dtype, dc, C_, d[0], d[1], m.value, ran)
                    # (conv_lean 1: both folded convs on the lean kernel; 0: no lean launch at all)
                    assert ran[K1_LN] == 2 if lean else sum(ran) == 0, (lean, dtype, C_, ran)
                    assert m.value > 0.1 and d[0] < tol * m.value and d[1] < tol * m.value, (lean, dtype, dc, C_, d[0], d[1], m.value)
            for dt, tol_out in ((L.LDC_F32, 1e-5), (L.LDC_BF16, 1.0 / 128)):
                d, m, r = C.c_double(), C.c_double(), C.c_double()
                before = lean_counts()
                L.check(lib.ldc_conv_compare(e._ctx, dt, 1, 75, 1024, 0, 1024, 3, 1, 0, 1, 0, 0, 0, C.byref(d), C.byref(m), C.byref(r)))
                ran = [a - b for a, b in zip(lean_counts(), before)]
                print("split-K conv", lean, dt, d.value, m.value, r.value, ran)
                assert (ran[K3] == 1 and sum(ran[:5]) == 1) if lean else sum(ran) == 0, (lean, dt, ran)
                assert m.value > 0.1 and d.value <= tol_out * m.value, (lean, dt, d.value, m.value)
                assert r.value < 1e-4, (lean, dt, r.value)
    finally:
        e.set_option("conv_lean", 1)
