"""Decode from RVQ codes on the GPU: the dequantisation front end (Engine.rvq_decode, Engine.decode_codes[_ddim]) against the
reference's quantised condition and against the waveform decode, out-of-range codes, and the compress / decompress CLIs.

The step kernels accumulate GroupNorm statistics with float atomics, so two runs of one configuration may differ in the last bits:
"equal" below is within the f32 run-to-run drift (tests/drift_tolerances.py, key "repeat"), as in test_gpu_ddim.py."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from ladiffcodec_amd.bitstream import Bitstream, packed_bytes, read_ecdc_header  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, load_golden, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL, check  # noqa: E402

SAME = TOL["f32"]["repeat"]


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _wav(B=4, T=5120, seed=50):
    return (torch.from_numpy(synth.synthetic_wav(B, T, seed=seed)) * 0.5).cuda()


def _noise(n, B, T, seed, hop=32):
    return torch.randn(n, B, 128, T // hop, generator=torch.Generator().manual_seed(seed)).cuda()


def test_condition_rows_from_codes():
    """rvq_decode / decode_codes' condition = the reference's quantized; bit-identical to get_cond's; packed = int64 source."""
    g = load_golden("codec_c1")
    e = engine("r84", "f32")
    bs = Bitstream(e)
    wav = cu(g["wav"])
    Fd = 16        # the decodes take the first 16 frames (T = 5120, the fixtures' length); rows are per frame
    for codes_key, q_key, bw in (("codes", "quantized", 0.0), ("codes_1p5", "quantized_1p5", 1.5)):
        codes = cu(g[codes_key])
        n_q, B, F = codes.shape
        assert rel(e.rvq_decode(codes).cpu().numpy(), g[q_key]) < 1e-6
        st = e.decode_codes(codes=codes[:, :, :Fd], n_steps=2, per_item=True, want_stages=True)
        assert rel(st["cond"].cpu().numpy(), g[q_key][..., :Fd]) < 1e-6
        assert st["wav"].shape == (B, 1, Fd * 320) and bool(torch.isfinite(st["wav"]).all())
        cond_w, codes_w = e.get_cond(wav, bandwidth=bw, return_codes=True)
        assert codes_w.shape == (n_q, B, F)
        assert torch.equal(e.rvq_decode(codes_w), cond_w)
        a = e.decode_codes(codes=codes_w[:, :, :Fd], n_steps=2, per_item=True, want_stages=True)["cond"]
        assert torch.equal(a, cond_w[..., :Fd])
        packed = bs.pack_codes(codes_w[:, :, :Fd].contiguous(), 10)
        b = e.decode_codes(packed=packed, n_q=n_q, F=Fd, n_steps=2, per_item=True, want_stages=True)["cond"]
        assert torch.equal(b, a)
        full = bs.pack_codes(codes_w, 10)     # a row stride beyond the frames decoded: the payload's first Fd frames
        c = e.decode_codes(packed=full, n_q=n_q, F=Fd, n_steps=2, per_item=True, want_stages=True)["cond"]
        assert torch.equal(c, a)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_decode_codes_against_fixture(tag, dtype):
    g = load_golden("ladiff_" + tag)
    e = engine(tag, dtype)
    n = int(g["meta"][2])
    _, codes = e.get_cond(cu(g["wav"]), return_codes=True)
    out = e.decode_codes(codes=codes, n_steps=n, noise=cu(g["noises"]), per_item=False, want_stages=True)
    assert rel(out["cond"].cpu().numpy(), g["cond"]) < 1e-4
    check(dtype, "chain_small", rel(out["latents"].cpu().numpy(), g["latents"]), tag)
    check(dtype, "wav_small", rel(out["wav"].cpu().numpy(), g["wav_out"]), tag)


def _same(a, b):
    assert rel(a["latents"].cpu().numpy(), b["latents"].cpu().numpy()) < SAME
    assert rel(a["wav"].cpu().numpy(), b["wav"].cpu().numpy()) < 1e-4


def test_decode_codes_equals_waveform_decode():
    """Same noise tape: decode_codes(get_cond's codes) = decode(wav), per_item 0 and 1, split ends on and off (B = 4: two parts);
    decode_codes_ddim = decode_ddim."""
    e = engine("r84", "f32")
    wav = _wav()
    B, _, T = wav.shape
    _, codes = e.get_cond(wav, return_codes=True)
    n = 5
    noise = _noise(n, B, T, 9)
    try:
        for split_ends in (1, 0):
            e.set_option("split_ends", split_ends)
            for per_item in (False, True):
                ref = e.decode(wav, n, noise, per_item=per_item, want_stages=True)
                got = e.decode_codes(codes=codes, n_steps=n, noise=noise, per_item=per_item, want_stages=True)
                assert torch.equal(got["cond"], ref["cond"]), (split_ends, per_item)
                _same(got, ref)
        e.set_option("split_ends", 1)
        S, t_start, eta = 6, 30, 0.7
        dn = _noise(S, B, T, 10)
        ref = e.decode_ddim(wav, t_start, S, eta, noise=dn, per_item=True, want_stages=True)
        got = e.decode_codes_ddim(codes=codes, t_start=t_start, n_steps=S, eta=eta, noise=dn, per_item=True, want_stages=True)
        _same(got, ref)
        packed = Bitstream(e).pack_codes(codes, 10)
        got_p = e.decode_codes_ddim(packed=packed, n_q=codes.shape[0], F=codes.shape[2], t_start=t_start, n_steps=S, eta=eta,
                                    noise=dn, per_item=True, want_stages=True)
        _same(got_p, ref)
    finally:
        e.set_option("split_ends", 1)


def test_bad_codes_are_refused():
    """A code outside [0, bins) never indexes a codebook: the call (or the next one) fails with LDC_E_INVALID "[bad_code]", no
    device fallback keys on it, and the context decodes valid codes as before.  (The codebooks are one contiguous [n_q][bins][D]
    buffer, so even an unguarded kernel would read inside the allocation here.)"""
    from ladiffcodec_amd import sample
    g = load_golden("ladiff_r84")
    e = engine("r84", "f32")
    n = int(g["meta"][2])
    noise = cu(g["noises"])
    _, codes = e.get_cond(cu(g["wav"]), return_codes=True)
    good = e.decode_codes(codes=codes, n_steps=n, noise=noise, want_stages=True)
    good = {k: v.clone() for k, v in good.items()}
    bad = codes.clone()
    bad[0, 0, 3] = 1024
    bad[1, 1, 5] = -1

    def refused(fn):
        with pytest.raises(L.LdcError) as ei:
            fn()
            torch.cuda.synchronize()
            e.rvq_decode(codes)                  # asynchronous calls: the next call on the context reports
        assert ei.value.code == L.E_INVALID and "[bad_code]" in str(ei.value), str(ei.value)
        assert "codebook" in str(ei.value) and "frame" in str(ei.value)
        assert not sample.apply_device_fallback(e, ei.value)

    refused(lambda: e.decode_codes(codes=bad, n_steps=n, noise=noise))
    refused(lambda: e.rvq_decode(bad))
    refused(lambda: e.decode_codes_ddim(codes=bad, t_start=20, n_steps=3, noise=None))
    # 11-bit payloads can hold 1024 .. 2047 (-1 packs as 2047): the packed source is checked as well
    p11 = Bitstream(e).pack_codes(bad, 11)
    refused(lambda: e.decode_codes(packed=p11, bits=11, n_q=codes.shape[0], F=codes.shape[2], n_steps=n, noise=noise))
    again = e.decode_codes(codes=codes, n_steps=n, noise=noise, want_stages=True)
    assert torch.equal(again["cond"], good["cond"])
    assert rel(again["latents"].cpu().numpy(), good["latents"].cpu().numpy()) < SAME
    assert rel(again["wav"].cpu().numpy(), good["wav"].cpu().numpy()) < 1e-4


# ------------------------------------------------------------------------------------------------------------------- CLIs
MIDWAY = 8


def _flags(tmp_path, ind, outd, *extra):
    return ["--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff",
            "--scaling_global", "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
            "--diff_dims", "32", "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", str(MIDWAY),
            "--dtype", "f32", "--seed", "3", *extra]


def _tree(tmp_path):
    from scipy.io import wavfile
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind = tmp_path / "in"
    (ind / "spk1").mkdir(parents=True)
    files = {"spk1/a.wav": (1, 5120), "spk1/b.wav": (1, 5120), "c.wav": (1, 5120), "odd.wav": (1, 5120 + 300), "st.wav": (2, 5120)}
    data = {}
    for k, (name, (ch, T)) in enumerate(files.items()):
        x = (synth.synthetic_wav(ch, T, seed=60 + k)[:, 0] * 0.5).astype(np.float32)     # [ch, T]
        wavfile.write(str(ind / name), 16000, x[0] if ch == 1 else np.ascontiguousarray(x.T))
        data[name] = x
    return ind, data


def _read(path):
    from scipy.io import wavfile
    sr, y = wavfile.read(str(path))
    assert sr == 16000
    return y


def test_cli_compress_decompress_equals_sample(tmp_path):
    from ladiffcodec_amd import compress, decompress, sample, sample_ddim
    from ladiffcodec_amd.model import Engine
    ind, data = _tree(tmp_path)
    enc = tmp_path / "enc"
    written = compress.main(_flags(tmp_path, ind, enc))
    assert sorted(os.path.relpath(p, enc) for p in written) == sorted(n[:-4] + ".ecdc" for n in data)
    ref_d, got_d = tmp_path / "ref", tmp_path / "got"
    sample.main(_flags(tmp_path, ind, ref_d))
    got = decompress.main(_flags(tmp_path, enc, got_d))
    assert len(got) == len(data)
    for name in data:
        a, b = _read(got_d / name), _read(ref_d / name)
        assert a.shape == b.shape and rel(a, b) < 1e-4, name
    # containers: exactly header + ch x packed bytes; mono ones read back (Bitstream.decompress_codes) to get_cond's codes
    mc, u, _ = CASES["r84"]
    eng = Engine(mc, u, COND_CFG, dtype="f32")
    eng.load_state_dict(L.MODEL_MAIN, main_sd_np("r84"))
    eng.load_state_dict(L.MODEL_COND, cond_sd_np())
    eng.finalize(strict=True)
    try:
        bs = Bitstream(eng)
        # the batches compress encodes: the mono files of equal trimmed length in sorted path order, the stereo file alone
        mono = sorted(n for n, x in data.items() if x.shape[0] == 1)
        _, mono_codes = eng.get_cond(cu(np.stack([data[n][0, :5120] for n in mono])[:, None, :]), bandwidth=3.0, return_codes=True)
        for name, x in data.items():
            blob = (enc / (name[:-4] + ".ecdc")).read_bytes()
            fo = io.BytesIO(blob)
            meta = read_ecdc_header(fo)
            n = x.shape[1] // 640 * 640
            F = n // 320
            assert meta["al"] == n and meta["nc"] == 6 and meta["lm"] is False and meta["hop"] == 320
            assert meta["m"] == "ladiffcodec_16khz" and meta.get("ch", 1) == x.shape[0]
            assert len(blob) == fo.tell() + x.shape[0] * packed_bytes(6, F, 10), name
            if x.shape[0] == 1:
                back, _ = bs.decompress_codes([blob])
                k = mono.index(name)
                assert torch.equal(back, mono_codes[:, k:k + 1]), name
            else:
                _, codes = eng.get_cond(cu(x[:, None, :n]), bandwidth=3.0, return_codes=True)
                rows = np.frombuffer(blob[fo.tell():], np.uint8).reshape(x.shape[0], -1)
                assert torch.equal(bs.unpack_codes(torch.from_numpy(rows.copy()), 6, F, 10), codes), name
    finally:
        eng.close()
    # DDIM flags: decompress --ddim_steps = sample_ddim
    ref_dd, got_dd = tmp_path / "ref_ddim", tmp_path / "got_ddim"
    ddim = ["--ddim_steps", "5", "--ddim_eta", "0.5"]
    sample_ddim.main(_flags(tmp_path, ind, ref_dd, *ddim))
    decompress.main(_flags(tmp_path, enc, got_dd, *ddim))
    for name in data:
        a, b = _read(got_dd / name), _read(ref_dd / name)
        assert a.shape == b.shape and rel(a, b) < 1e-4, name


def test_cli_decompress_refuses_bad_container(tmp_path):
    from ladiffcodec_amd import decompress
    from ladiffcodec_amd.bitstream import ecdc_container
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    enc, out = tmp_path / "enc", tmp_path / "out"
    enc.mkdir()
    (enc / "ok.ecdc").write_bytes(ecdc_container([bytes(packed_bytes(6, 16, 10))], 5120, 6))
    (enc / "short.ecdc").write_bytes(ecdc_container([bytes(packed_bytes(6, 16, 10) - 1)], 5120, 6))
    with pytest.raises(ValueError, match="short.ecdc"):
        decompress.main(_flags(tmp_path, enc, out))
    assert not out.exists()


def test_cli_decompress_long_file_is_the_chunk_composition(tmp_path):
    """--chunk_sec: the chunks' decode_codes raw outputs (codes of the whole-file encode), joined, output_normalise(per_item=False)."""
    from scipy.io import wavfile
    from ladiffcodec_amd import compress, decompress
    from ladiffcodec_amd.model import Engine
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind, enc, outd = tmp_path / "in", tmp_path / "enc", tmp_path / "out"
    ind.mkdir()
    T = 48000 + 200
    x = (synth.synthetic_wav(1, T, seed=70)[0, 0] * 0.5).astype(np.float32)
    wavfile.write(str(ind / "long.wav"), 16000, x)
    compress.main(_flags(tmp_path, ind, enc))

    def provider(keys, steps, L_lat):
        return torch.stack([torch.randn(steps, 128, L_lat, generator=torch.Generator().manual_seed(1000 * i + k)) for i, k in keys], 1)

    a = decompress.build_parser().parse_args(_flags(tmp_path, enc, outd, "--chunk_sec", "1.0"))
    a.noise_provider = provider
    decompress.decompress(a)
    got = _read(outd / "long.wav")
    # the composition, on an engine of its own
    mc, u, _ = CASES["r84"]
    eng = Engine(mc, u, COND_CFG, dtype="f32")
    eng.load_state_dict(L.MODEL_MAIN, main_sd_np("r84"))
    eng.load_state_dict(L.MODEL_COND, cond_sd_np())
    eng.finalize(strict=True)
    try:
        n = T // 640 * 640
        _, codes = eng.get_cond(cu(x[None, None, :n]), bandwidth=3.0, return_codes=True)
        chunk = 16000 // 2560 * 2560                                    # chunk_quantum(8 4) = 2560 samples = 8 frames
        starts = list(range(0, n - chunk + 1, chunk))
        tail = (n - starts[-1] - chunk) // 2560 * 2560
        pieces = [(st, chunk) for st in starts] + ([(starts[-1] + chunk, tail)] if tail else [])
        raw = [None] * len(pieces)
        for ln in sorted({p[1] for p in pieces}, reverse=True):
            ks = [k for k, p in enumerate(pieces) if p[1] == ln]
            cc = torch.stack([codes[:, 0, pieces[k][0] // 320:(pieces[k][0] + ln) // 320] for k in ks], 1).contiguous()
            st = eng.decode_codes(codes=cc, n_steps=MIDWAY, noise=provider([(0, k) for k in ks], MIDWAY, ln // 32).cuda(), per_item=True,
                                  want_stages=True)
            r = eng.decode_latents(L.MODEL_MAIN, st["latents"])
            for j, k in enumerate(ks):
                raw[k] = r[j:j + 1]
        ref = eng.output_normalise(torch.cat(raw, -1), per_item=False).cpu().numpy()[0, 0]
    finally:
        eng.close()
    assert got.shape == ref.shape and rel(got, ref) < 1e-4
