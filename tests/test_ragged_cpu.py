"""Ragged decode without a GPU: the exports, the refusals that come before any GPU work, the CLI flags and the batch planner, and
the prefix-exactness of the codec ends that lets a right-padded batch stand for its items: the cond encoder,
RVQ and the main decoder are causal, so the first F_b frames / T_b samples of a right-padded item are the item's own."""
import ctypes as C

import numpy as np
import pytest
import torch

from ladiffcodec_amd import lib as L, sample, synth
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np
from oracle import ldc_oracle as O


def _err():
    return L.load().ldc_last_error().decode()


def test_ragged_exports_listed():
    for name in ("ldc_decode_ragged", "ldc_unet_forward_ragged"):
        assert name in L.EXPORTS and hasattr(L.load(), name)


def test_ragged_calls_refuse_a_null_context():
    lib = L.load()
    lens = (C.c_int32 * 2)(2560, 5120)
    assert lib.ldc_decode_ragged(None, None, lens, 2, 5120, 0, 4, 0.0, None, None, None, None, None, None) != 0
    assert lib.ldc_unet_forward_ragged(None, None, 0, None, lens, 2, 160, 16, None, None) != 0


def test_parser_has_the_ragged_flags():
    assert sample.ragged_options(sample.build_parser().parse_args([])) == (False, 0.25)
    assert sample.ragged_options(sample.build_parser().parse_args(["--ragged"])) == (True, 0.25)
    assert sample.ragged_options(sample.build_parser().parse_args(["--ragged", "--ragged_waste", "0.5"])) == (True, 0.5)
    from ladiffcodec_amd import sample_ddim
    assert sample.ragged_options(sample_ddim.build_parser().parse_args(["--ragged"])) == (True, 0.25)


def _corpus(n=200, seed=3):
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(300, 16000 * 20, size=n)]
    channels = [1] * n
    for k in (5, 17, 40):
        channels[k] = 2
    return lengths, channels


@pytest.mark.parametrize("quantum", [2560, 640])
@pytest.mark.parametrize("waste", [0.0, 0.1, 0.25, 0.5])
@pytest.mark.parametrize("world", [1, 3])
def test_planner_properties(quantum, waste, world):
    lengths, channels = _corpus()
    bs = 8
    seen = []
    for rank in range(world):
        for idxs, joint in sample.plan_ragged_batches(lengths, channels, rank, world, bs, waste, quantum):
            seen += idxs
            assert 0 < len(idxs) <= bs
            if joint:
                assert len(idxs) == 1 and channels[idxs[0]] > 1
                continue
            assert all(channels[i] == 1 for i in idxs)
            trimmed = [lengths[i] // quantum * quantum for i in idxs]
            if trimmed[0] == 0:                       # shorter than a quantum: the equal-length batches of plan_batches
                assert len({lengths[i] // 640 * 640 for i in idxs}) == 1
                continue
            assert all(n > 0 and n % quantum == 0 for n in trimmed)
            assert len(idxs) * max(trimmed) <= (1.0 + waste) * sum(trimmed) * (1 + 1e-12), (idxs, trimmed)
    assert sorted(seen) == list(range(len(lengths)))       # every file in exactly one batch


def test_planner_packs_and_plan_batches_is_unchanged():
    lengths, channels = _corpus()
    mono = sum(1 for c, n in zip(channels, lengths) if c == 1 and n >= 2560)
    rag = [w for w in sample.plan_ragged_batches(lengths, channels, 0, 1, 8, 0.25, 2560) if not w[1] and lengths[w[0][0]] >= 2560]
    assert len(rag) < mono / 3                                  # different lengths do share batches
    # the equal-length plan: grouped by the 640-sample trim, longest first, batch_size at most -- as before this flag existed
    work = sample.plan_batches(lengths, channels, 0, 1, 8)
    from ladiffcodec_amd import parallel
    by_len, want = {}, []
    for i in parallel.shard_utterances(lengths, 0, 1):
        if channels[i] > 1:
            want.append(([i], True))
        else:
            by_len.setdefault(lengths[i] // 640 * 640, []).append(i)
    for _, idxs in sorted(by_len.items(), reverse=True):
        want += [(idxs[s:s + 8], False) for s in range(0, len(idxs), 8)]
    assert work == want


def test_padded_batch_builder(tmp_path):
    from scipy.io import wavfile
    xs = [(synth.synthetic_wav(1, n, seed=60 + k)[0, 0] * 0.5).astype(np.float32) for k, n in enumerate((6000, 3000))]
    files = []
    for k, x in enumerate(xs):
        files.append(str(tmp_path / f"{k}.wav"))
        wavfile.write(files[-1], 16000, x)
    wavs = sample.LazyWavs(files, eng=None)
    b = wavs.padded_batch([0, 1], [5120, 2560])
    assert tuple(b.shape) == (2, 1, 5120)
    assert np.array_equal(b[0, 0].numpy(), xs[0][:5120]) and np.array_equal(b[1, 0, :2560].numpy(), xs[1][:2560])
    assert not b[1, 0, 2560:].any()
    rb = sample.RaggedBatch(b, [5120, 2560]).to("cpu")
    assert rb.lengths == [5120, 2560] and rb.wav.shape == b.shape


@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_codec_ends_are_prefix_exact(tag):
    """Encoder + RVQ of a right-padded waveform = the solo result on the first F_b frames (same codes); the decoder of right-padded
    latents = the solo result on the first T_b samples.  T_b on the chunk quantum, so get_extra_padding_for_conv1d adds nothing.
    One exception, which the engine handles by encoding such an item on its own: with F_b <= 6 frames the encoder's last conv
    (k = 7) pads more than the item is long and the reference's reflect padding changes form (conv.py:81-98) -- checked last."""
    mc, u, _ = CASES[tag]
    q = sample.chunk_quantum(mc.enc_ratios)
    sdc, sdm = synth.to_torch(cond_sd_np()), synth.to_torch(main_sd_np(tag))
    Tb, Tmax = max(2 * q, 2560), max(5 * q, 6400)
    wav = torch.from_numpy(synth.synthetic_wav(1, Tmax, seed=91)) * 0.5
    solo = wav[..., :Tb].clone()
    for fill in (0.0, 0.3):                                    # zeros behind the item, or anything else
        padded = wav.clone()
        padded[..., Tb:] = fill
        cond_s, codes_s, _, z_s = O.get_cond(sdc, COND_CFG, solo)
        cond_p, codes_p, _, z_p = O.get_cond(sdc, COND_CFG, padded)
        Fb = Tb // COND_CFG.hop_length
        assert cond_s.shape[-1] == Fb
        assert torch.equal(codes_p[..., :Fb], codes_s)
        assert float((z_p[..., :Fb] - z_s).abs().max()) <= 1e-5 * float(z_s.abs().max())
        assert float((cond_p[..., :Fb] - cond_s).abs().max()) <= 1e-6 * float(cond_s.abs().max())
    Lb, Lmax = Tb // mc.hop_length, Tmax // mc.hop_length
    lat = torch.randn(1, mc.rep_dims, Lmax, generator=torch.Generator().manual_seed(4)) * 0.3
    for fill in (0.0, 0.7):
        lp = lat.clone()
        lp[..., Lb:] = fill
        y_s = O.seanet_decode(sdm, mc, lat[..., :Lb].clone())
        y_p = O.seanet_decode(sdm, mc, lp)
        assert y_s.shape[-1] == Tb and y_p.shape[-1] == Tmax
        assert float((y_p[..., :Tb] - y_s).abs().max()) <= 1e-5 * float(y_s.abs().max())
    # the exception: 4 frames
    short = wav[..., :1280].clone()
    z_s = O.get_cond(sdc, COND_CFG, short)[3]
    z_p = O.get_cond(sdc, COND_CFG, wav)[3]
    assert float((z_p[..., :4] - z_s).abs().max()) > 1e-3 * float(z_s.abs().max())
