"""Stream sessions on the GPU: chunks pushed through ldc_get_cond_stream / ldc_seanet_encode_stream / ldc_seanet_decode_stream give,
joined, what the whole-sequence calls give.  f32 engines on the synthetic checkpoints.  The bar is the project's own for "same fp32
arithmetic, another kernel or summation order" (test_gpu_parity.py): a chunk may take another split-K factor or LSTM kernel than the whole
call.  tests/test_stream_cpu.py shows on the oracle that an implementation without state misses that bar by far more than 100 x."""
import ctypes as C

import numpy as np
import pytest
import torch

from ladiffcodec_amd import lib as L, synth
from gpu_common import engine, rel
from helpers import COND_CFG, cond_sd_np, main_sd_np
from oracle import ldc_oracle as O

pytestmark = pytest.mark.gpu

BAR = 1e-5
SCHEDULE = (7, 1, 1, 5, 10)          # cond frames: the minimum first chunk, single frames, uneven pieces
_CACHE = {}


def wav3():
    if "wav" not in _CACHE:
        _CACHE["wav"] = torch.from_numpy(synth.synthetic_wav(3, 7680, seed=300)) * 0.5
    return _CACHE["wav"]


def whole(key, fn):
    """a whole-sequence reference, computed once and shared"""
    if key not in _CACHE:
        _CACHE[key] = fn().cpu()
    return _CACHE[key]


def pieces(total, first):
    """min_first, then 1, then the rest in two uneven pieces"""
    rest = total - first - 1
    a = rest // 3
    assert first >= 1 and a >= 1
    return [first, 1, a, rest - a]


def push(fn, x, sched, unit):
    outs, at = [], 0
    for n in sched:
        outs.append(fn(x[..., at:at + n * unit]))
        at += n * unit
    assert at == x.shape[-1]
    return outs


def check(name, got, ref):
    err = rel(got.cpu().numpy(), ref.cpu().numpy())
    print(f"{name}: streamed vs whole {err:.3e}")
    assert err <= BAR, (name, err)


@pytest.mark.parametrize("lstm_stream_only", [0, 1])
def test_cond_encoder_and_rvq(lstm_stream_only):
    e = engine("r84", "f32")
    wav = wav3().cuda()
    quant_o, codes_o, margins_o, _ = O.get_cond(synth.to_torch(cond_sd_np()), COND_CFG, wav3())
    safe = np.minimum.accumulate(margins_o.numpy(), axis=0) > 1e-3
    assert safe.all(), float(margins_o.min())          # this input leaves no code out
    assert safe.mean() >= 0.99
    e.set_option("lstm_stream", lstm_stream_only)
    try:
        z_w = e.encode(L.MODEL_COND, wav)
        cond_w, codes_w = e.get_cond(wav, return_codes=True)
        st = e.open_stream(L.MODEL_COND, L.STREAM_ENCODER, 3)
        assert st.min_first == 7 * 320
        z_s = torch.cat(push(st.encode, wav, SCHEDULE, 320), dim=-1)
        st.reset()
        outs = push(lambda x: st.get_cond(x, return_codes=True), wav, SCHEDULE, 320)
        st.close()
    finally:
        e.set_option("lstm_stream", 0)
    tag = "stream" if lstm_stream_only else "coop"
    check(f"cond encoder z ({tag} LSTM)", z_s, z_w)
    check(f"cond_out ({tag} LSTM)", torch.cat([o[0] for o in outs], dim=-1), cond_w)
    codes_s = torch.cat([o[1] for o in outs], dim=-1).cpu().numpy()
    assert np.array_equal(codes_s[safe], codes_w.cpu().numpy()[safe])
    assert np.array_equal(codes_s[safe], codes_o.numpy()[safe])


def test_cond_encoder_one_item():
    """B = 1: the LSTM of one or two items takes the XCD-local cooperative kernel"""
    e = engine("r84", "f32")
    wav = wav3()[:1].cuda()
    z_w = e.encode(L.MODEL_COND, wav)
    st = e.open_stream(L.MODEL_COND, L.STREAM_ENCODER, 1)
    z_s = torch.cat(push(st.encode, wav, SCHEDULE, 320), dim=-1)
    st.close()
    check("cond encoder z, one item", z_s, z_w)


def test_decoders():
    e = engine("r84", "f32")
    wav = wav3().cuda()
    cond = whole("cond", lambda: e.get_cond(wav)).cuda()                    # [3, 128, 24]
    z_main = whole("z_main", lambda: e.encode(L.MODEL_MAIN, wav)).cuda()     # [3, 128, 240]
    for name, which, z in (("cond decoder", L.MODEL_COND, cond), ("r84 main decoder", L.MODEL_MAIN, z_main)):
        ref = e.decode_latents(which, z)
        st = e.open_stream(which, L.STREAM_DECODER, 3)
        got = torch.cat(push(st.decode, z, pieces(z.shape[-1], st.min_first), 1), dim=-1)
        st.close()
        check(name, got, ref)


@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_main_encoders(tag):
    e = engine(tag, "f32")
    wav = wav3().cuda()
    ref = e.encode(L.MODEL_MAIN, wav)
    st = e.open_stream(L.MODEL_MAIN, L.STREAM_ENCODER, 3)
    hop = st.hop
    assert st.min_first % hop == 0
    got = torch.cat(push(st.encode, wav, pieces(wav.shape[-1] // hop, st.min_first // hop), hop), dim=-1)
    st.close()
    check(f"{tag} main encoder", got, ref)


def test_mixed_freshness():
    e = engine("r84", "f32")
    wav = wav3().cuda()
    other = (torch.from_numpy(synth.synthetic_wav(1, 7680, seed=301)) * 0.5).cuda()
    z_w = whole("z_cond", lambda: e.encode(L.MODEL_COND, wav)).cuda()
    z_o = e.encode(L.MODEL_COND, other[..., :16 * 320])
    st = e.open_stream(L.MODEL_COND, L.STREAM_ENCODER, 3)
    outs = push(st.encode, wav[..., :8 * 320], (7, 1), 320)
    st.reset([False, True, False])                     # item 1 starts a different signal; items 0 and 2 go on
    new = []
    for a, n in ((0, 7), (7, 1), (8, 8)):              # all items advance by the same length
        x = wav[..., (8 + a) * 320:(8 + a + n) * 320].clone()
        x[1] = other[0, :, a * 320:(a + n) * 320]
        new.append(st.encode(x))
    st.close()
    new = torch.cat(new, dim=-1)
    cont = torch.cat(outs + [new], dim=-1)
    for b in (0, 2):
        check(f"item {b} continues", cont[b], z_w[b])
    check("item 1 restarted", new[1], z_o[0])


def test_refusals():
    e = engine("r84", "f32")
    lib, ctx = e.lib, e._ctx
    wav = wav3().cuda()
    st = e.open_stream(L.MODEL_COND, L.STREAM_ENCODER, 3)
    dec = e.open_stream(L.MODEL_COND, L.STREAM_DECODER, 3)
    main = e.open_stream(L.MODEL_MAIN, L.STREAM_ENCODER, 3)
    z = torch.empty(3, 128, 24, device="cuda")
    codes = torch.empty(6, 3, 24, dtype=torch.int64, device="cuda")
    out = torch.empty(3, 1, 7680, device="cuda")

    def refused(rc, *words):
        assert rc == L.E_INVALID, rc
        msg = lib.ldc_last_error().decode()
        for w in words:
            assert str(w) in msg, (w, msg)

    w, zp, s = wav.data_ptr(), z.data_ptr(), None
    refused(lib.ldc_seanet_encode_stream(ctx, st._st, w, 2240 + 100, zp, s), "T = 2340", 320)       # not a multiple of the hop
    refused(lib.ldc_seanet_encode_stream(ctx, st._st, w, 0, zp, s), "T = 0")
    refused(lib.ldc_seanet_encode_stream(ctx, st._st, w, 6 * 320, zp, s), "fresh", 1920, 2240)      # below the first-chunk minimum
    refused(lib.ldc_seanet_decode_stream(ctx, dec._st, zp, 6, out.data_ptr(), s), "fresh", "L = 6", 7)
    refused(lib.ldc_seanet_decode_stream(ctx, dec._st, zp, 0, out.data_ptr(), s), "L = 0")
    refused(lib.ldc_seanet_encode_stream(ctx, dec._st, w, 2240, zp, s), "side 1")                   # the other side
    refused(lib.ldc_seanet_decode_stream(ctx, st._st, zp, 7, out.data_ptr(), s), "side 0")
    refused(lib.ldc_get_cond_stream(ctx, main._st, w, 2240, 0.0, zp, codes.data_ptr(), s), "codec 0")   # the other codec
    refused(lib.ldc_get_cond_stream(ctx, dec._st, w, 2240, 0.0, zp, codes.data_ptr(), s), "side 1")
    e8 = engine("r8", "f32")
    refused(lib.ldc_seanet_encode_stream(e8._ctx, st._st, w, 2240, zp, s), "another context")
    refused(lib.ldc_seanet_encode_stream(ctx, None, w, 2240, zp, s), "null pointer", "stream object")
    refused(lib.ldc_seanet_encode_stream(ctx, st._st, None, 2240, zp, s), "null pointer", "wav")
    refused(lib.ldc_seanet_encode_stream(ctx, st._st, w, 2240, None, s), "null pointer", "z_out")
    refused(lib.ldc_get_cond_stream(ctx, st._st, w, 2240, 0.0, None, None, s), "null pointer", "cond_out")
    refused(lib.ldc_seanet_decode_stream(ctx, dec._st, None, 7, out.data_ptr(), s), "null pointer", "z")
    refused(lib.ldc_stream_reset(None, None, s), "null pointer")
    handle = C.c_void_p()
    refused(lib.ldc_stream_create(ctx, L.MODEL_COND, L.STREAM_ENCODER, 0, C.byref(handle)), "B = 0")
    refused(lib.ldc_stream_create(ctx, L.MODEL_COND, L.STREAM_ENCODER, 3, None), "null pointer")
    refused(lib.ldc_stream_create(ctx, L.MODEL_COND, 2, 3, C.byref(handle)), "side = 2")
    # nothing above touched the state: the stream is still fresh and the context usable
    z_w = whole("z_cond", lambda: e.encode(L.MODEL_COND, wav)).cuda()
    check("after the refusals", torch.cat(push(st.encode, wav, (12, 12), 320), dim=-1), z_w)
    for o in (st, dec, main):
        o.close()


def test_a_chunk_whose_windows_do_not_fit_is_refused_before_any_gpu_work():
    """One-frame chunks of thousands of items: a conv tile of the last strided layer crosses an item seam at every row and its LDS window
    does not fit.  The call is refused while it is being measured, the state is untouched and the session goes on."""
    e = engine("r84", "f32")
    B = 4096
    wav = wav3()[:1].cuda()
    z_w = whole("z_cond", lambda: e.encode(L.MODEL_COND, wav3().cuda()))[:1].cuda()
    st = e.open_stream(L.MODEL_COND, L.STREAM_ENCODER, B)
    rep = lambda a, b: wav[..., a * 320:b * 320].expand(B, 1, -1)
    z0 = st.encode(rep(0, 7))
    with pytest.raises(L.LdcError) as ei:
        st.encode(rep(7, 8))
    assert ei.value.code == L.E_INVALID and "B = 4096" in str(ei.value) and "chunk of 8 rows" in str(ei.value), str(ei.value)
    z1 = st.encode(rep(7, 24))
    st.close()
    for b in (0, B - 1):
        check(f"item {b} of {B} around the refusal", torch.cat([z0[b], z1[b]], dim=-1), z_w[0])


def test_cli_compress_stream_sec(tmp_path):
    from scipy.io import wavfile
    from ladiffcodec_amd import compress
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind = tmp_path / "in"
    ind.mkdir()
    for k, (name, sec) in enumerate((("a.wav", 3.0), ("b.wav", 5.2))):
        wavfile.write(str(ind / name), 16000, (synth.synthetic_wav(1, int(sec * 16000), seed=310 + k)[0, 0] * 0.5).astype(np.float32))

    def flags(outd, *extra):
        return ["--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff",
                "--scaling_global", "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
                "--diff_dims", "32", "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--dtype", "f32", "--batch_size", "4", *extra]

    plain, streamed = tmp_path / "plain", tmp_path / "streamed"
    assert len(compress.main(flags(plain))) == 2
    assert len(compress.main(flags(streamed, "--stream_sec", "1.0"))) == 2
    for name in ("a.ecdc", "b.ecdc"):
        assert (streamed / name).read_bytes() == (plain / name).read_bytes(), name
