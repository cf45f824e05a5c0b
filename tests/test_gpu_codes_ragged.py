"""Mixed-length batches at both codec ends on the GPU: Engine.get_cond_ragged (sender), Engine.decode_codes_ragged (receiver), the
range coder with a symbol count per stream, and `compress --ragged` / `decompress --ragged`.

Three items per batch, not sorted by length: the shortest legal one (r8: 640 samples = 2 frames, which the sender encodes on its own
-- DESIGN.md section 5a), one of Fmax frames and one in between.  4 DDPM steps, or 4 DDIM steps from t = 40.

The bars of the receiver tests are those tests/test_gpu_ragged.py asserts for the same plan (imported, not copied): f32 against the
engine's own decode_ragged within the f32 floor 1e-5 of max|ref| (GroupNorm's float atomics reorder between runs); bf16 against the
CPU oracle's solo decode of every item, started from the item's (bit-identical) condition.

One case of the CLI test cannot exist as asked: a container whose length is off the receiver's quantum is, by the quantum's
definition (whole condition frames and a latent length that survives the UNet's halvings), one that no decode accepts -- with or
without --ragged.  The test therefore checks that such a container takes the fallback batches and is refused by the engine exactly as
the run without the flag refuses it, and compares waveforms on four decodable files of three lengths."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, sample, synth  # noqa: E402
from ladiffcodec_amd.bitstream import Bitstream, packed_bytes  # noqa: E402
from helpers import CASES, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import check  # noqa: E402
from oracle import bitstream_oracle as BO, ldc_oracle as O  # noqa: E402
from test_gpu_ragged import check_wav, oracle_ddim  # noqa: E402  (the ragged plan's bf16 waveform bar and the oracle's DDIM)

FRAMES = {"r8": (8, 2, 16), "r84": (16, 8, 24)}      # condition frames per item; quanta of 2 (r8) / 8 (r84) frames
N_STEPS, T_START = 4, 40
F32_FLOOR = 1e-5
MODES = {"ddpm": (0, 0.0), "ddim0": (T_START, 0.0), "ddim1": (T_START, 1.0)}
_CACHE = {}


def setup(tag):
    """wav [3, 1, Tmax] (zero behind each item), lengths, the noise tape; the f32 engine's decode_ragged of it per mode (the source of
    the codes, and the f32 reference)."""
    if tag in _CACHE:
        return _CACHE[tag]
    mc, u, _ = CASES[tag]
    frames = list(FRAMES[tag])
    lens = [f * 320 for f in frames]
    Tmax, hop = max(lens), mc.hop_length
    assert min(lens) == sample.chunk_quantum(mc.enc_ratios) and all(n % min(lens) == 0 for n in lens)
    wav = torch.from_numpy(synth.synthetic_wav(3, Tmax, seed=171)) * 0.5
    for b, n in enumerate(lens):
        wav[b, :, n:] = 0
    noise = torch.randn(N_STEPS, 3, 128, Tmax // hop, generator=torch.Generator().manual_seed(27))
    s = dict(tag=tag, mc=mc, u=u, frames=frames, lens=lens, Tmax=Tmax, Fmax=max(frames), hop=hop, wav=wav, noise=noise, noise_dev=noise.cuda(),
             sdm=synth.to_torch(main_sd_np(tag)), by_wav={}, oracle={})
    _CACHE[tag] = s
    return s


def from_wav(s, mode):
    """decode_ragged of the f32 engine (cached, on the host): codes, cond, latents, wav"""
    if mode not in s["by_wav"]:
        t_start, eta = MODES[mode]
        got = engine(s["tag"], "f32").decode_ragged(s["wav"].cuda(), s["lens"], N_STEPS, t_start=t_start, eta=eta, noise=s["noise_dev"],
                                                     want_stages=True)
        s["by_wav"][mode] = {k: v.cpu() for k, v in got.items()}
    return s["by_wav"][mode]


def oracle_items(s, mode):
    """the CPU oracle's solo decode of every item from its condition rows (cached)"""
    if mode not in s["oracle"]:
        t_start, eta = MODES[mode]
        cond = from_wav(s, "ddpm")["cond"]
        out = []
        for b, (n, f) in enumerate(zip(s["lens"], s["frames"])):
            cb = cond[b:b + 1, :, :f].contiguous()
            img0 = O.start_image(s["sdm"], s["u"], cb, True)
            nz = s["noise"][:, b:b + 1, :, :n // s["hop"]]
            lat = (oracle_ddim(s["sdm"], s["u"], img0, cb, t_start, N_STEPS, eta, nz) if t_start
                   else O.halfway_sampling(s["sdm"], s["u"], img0, cb, N_STEPS, nz))
            out.append(dict(latents=lat, wav=O.output_normalise(O.seanet_decode(s["sdm"], s["mc"], lat), True)))
        s["oracle"][mode] = out
    return s["oracle"][mode]


def packed_rows(e, codes, frames, bits, fill=0):
    """[B, stride] uint8: row b = the solo pack of item b's own frames, `fill` in every byte behind it (stride: 3 bytes to spare)"""
    bs = Bitstream(e)
    n_q, B, _ = codes.shape
    rows = torch.full((B, packed_bytes(n_q, max(frames), bits) + 3), fill, dtype=torch.uint8)
    for b, f in enumerate(frames):
        solo = bs.pack_codes(codes[:, b:b + 1, :f].contiguous().cuda(), bits).cpu()[0]
        assert solo.numel() == packed_bytes(n_q, f, bits)
        rows[b, :solo.numel()] = solo
    return rows


def zeros_behind(s, got, keys=("cond", "latents", "wav")):
    for b, (n, f) in enumerate(zip(s["lens"], s["frames"])):
        for k, m in (("cond", f), ("latents", n // s["hop"]), ("wav", n)):
            if k in keys:
                assert not got[k][b, :, m:].any(), (k, b)


# ----------------------------------------------------------------------------------------------------------- 1. dequantiser
@pytest.mark.parametrize("tag,n_q,bits", [("r8", 6, 10), ("r8", 3, 10), ("r8", 6, 11), ("r84", 6, 10)])
def test_condition_rows_are_the_solo_dequantisation(tag, n_q, bits):
    """n_q = 3 and bits = 11 end the 2-frame item's stream mid-byte (60 / 132 bits)"""
    s = setup(tag)
    e = engine(tag, "f32")
    codes = from_wav(s, "ddpm")["codes"][:n_q].contiguous()
    if tag == "r8" and (n_q, bits) != (6, 10):
        assert (n_q * min(s["frames"]) * bits) % 8
    solo = [e.rvq_decode(codes[:, b:b + 1, :f].contiguous().cuda()).cpu() for b, f in enumerate(s["frames"])]
    a = e.decode_codes_ragged(codes=codes.cuda(), frames=s["frames"], bits=bits, n_steps=1, noise=s["noise_dev"][:1], want_stages=True)
    p = e.decode_codes_ragged(packed=packed_rows(e, codes, s["frames"], bits, fill=0xFF).cuda(), n_q=n_q, frames=s["frames"], bits=bits,
                              n_steps=1, noise=s["noise_dev"][:1], want_stages=True)
    for got in (a, p):
        got = {k: v.cpu() for k, v in got.items()}
        for b, f in enumerate(s["frames"]):
            assert float((got["cond"][b:b + 1, :, :f] - solo[b]).abs().max()) == 0.0, b
        zeros_behind(s, got)
        assert bool(torch.isfinite(got["wav"]).all())


# ------------------------------------------------------------------------------------------------------ 2. padding never read
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_codes_behind_an_item_are_never_read(tag):
    s = setup(tag)
    e = engine(tag, "f32")
    codes = from_wav(s, "ddpm")["codes"]
    bins = 1024
    kw = dict(frames=s["frames"], n_steps=N_STEPS, noise=s["noise_dev"], want_stages=True)
    base = {k: v.cpu() for k, v in e.decode_codes_ragged(codes=codes.cuda(), **kw).items()}
    junk = codes.clone()
    for b, f in enumerate(s["frames"]):
        junk[0::2, b, f:] = bins + 5
        junk[1::2, b, f:] = -1
    runs = [e.decode_codes_ragged(codes=junk.cuda(), **kw),
            e.decode_codes_ragged(packed=packed_rows(e, codes, s["frames"], 10, fill=0xFF).cuda(), n_q=codes.shape[0], bits=10, **kw)]
    for got in runs:
        got = {k: v.cpu() for k, v in got.items()}
        assert torch.equal(got["cond"], base["cond"])
        for k in ("latents", "wav"):
            v = rel(got[k].numpy(), base[k].numpy())
            print(f"{tag} {k} junk padding vs zero padding: {v:.3e}")
            assert v < F32_FLOOR, (k, v)
        zeros_behind(s, got)


def test_a_bad_code_inside_an_item_is_still_refused():
    s = setup("r84")
    e = engine("r84", "f32")
    codes = from_wav(s, "ddpm")["codes"]
    bad = codes.clone()
    bad[1, 2, 3] = 1024                                        # item 2 has 24 frames
    with pytest.raises(L.LdcError) as ei:
        e.decode_codes_ragged(codes=bad.cuda(), frames=s["frames"], n_steps=1, noise=s["noise_dev"][:1])
        torch.cuda.synchronize()
        e.rvq_decode(codes.cuda())                             # asynchronous calls: the next call on the context reports
    msg = str(ei.value)
    assert ei.value.code == L.E_INVALID and "[bad_code]" in msg, msg
    assert "codebook 1, item 2, frame 3" in msg, msg
    assert not sample.apply_device_fallback(e, ei.value)
    again = e.decode_codes_ragged(codes=codes.cuda(), frames=s["frames"], n_steps=1, noise=s["noise_dev"][:1], want_stages=True)
    assert torch.equal(again["cond"].cpu(), from_wav(s, "ddpm")["cond"])


# ------------------------------------------------------------------------------------------------------------------ 3. sender
@pytest.mark.parametrize("lens", [(2560, 640, 5120), (2240, 1920, 4800)])     # 2 frames; 7 and 6 frames: either side of the re-encode
def test_get_cond_ragged_is_get_cond_per_item(lens):
    e = engine("r8", "f32")
    Tmax = max(lens)
    wav = torch.from_numpy(synth.synthetic_wav(3, Tmax, seed=172)) * 0.5
    for fill in (0.0, 0.3):                                     # whatever lies behind an item
        w = wav.clone()
        for b, n in enumerate(lens):
            w[b, :, n:] = fill
        for bw in (0.0, 1.5):
            cond, codes = e.get_cond_ragged(w.cuda(), lens, bandwidth=bw, return_codes=True)
            cond, codes = cond.cpu(), codes.cpu()
            for b, n in enumerate(lens):
                c1, k1 = e.get_cond(w[b:b + 1, :, :n].contiguous().cuda(), bandwidth=bw, return_codes=True)
                f = n // 320
                assert torch.equal(codes[:, b:b + 1, :f], k1.cpu()), (b, bw, fill)
                assert float((cond[b:b + 1, :, :f] - c1.cpu()).abs().max()) == 0.0, (b, bw, fill)
                assert not codes[:, b, f:].any() and not cond[b, :, f:].any(), (b, bw, fill)


def test_static_streams_of_unequal_length_are_the_solo_streams():
    e = engine("r84", "f32")
    bs = Bitstream(e)
    g = torch.Generator().manual_seed(8)
    n_q, frames = 6, [16, 1, 9, 24, 0]
    F = max(frames)
    pdf = torch.softmax(torch.randn(n_q, 1024, generator=g) * 2.0, dim=-1)
    cdf = bs.build_cdf(pdf.cuda())
    codes = torch.stack([torch.multinomial(pdf[k], len(frames) * F, replacement=True, generator=g).reshape(len(frames), F) for k in range(n_q)])
    sym = codes.permute(1, 2, 0).reshape(len(frames), F * n_q)
    n_sym = [n_q * f for f in frames]
    streams = bs.ac_encode(sym.cuda(), cdf, static=True, n_sym=n_sym)
    for b, n in enumerate(n_sym):
        solo = bs.ac_encode(sym[b:b + 1, :max(n, 1)].contiguous().cuda(), cdf, static=True)[0] if n else b""
        assert streams[b] == solo, b
    want = BO.ac_encode(sym[2, :n_sym[2]].tolist(), cdf.cpu().numpy().astype(np.int64), np.tile(np.arange(n_q), frames[2]))
    assert streams[2] == want
    back = bs.ac_decode(streams, F * n_q, cdf, static=True, n_sym=n_sym).cpu()
    for b, n in enumerate(n_sym):
        assert torch.equal(back[b, :n], sym[b, :n].to(torch.int32)) and not back[b, n:].any(), b
    # a table per (stream, step): rows b * S + s of the padded layout
    card = 37
    pdf2 = torch.softmax(torch.randn(3, 50, card, generator=g), dim=-1)
    cdf2 = bs.build_cdf(pdf2.cuda())
    sym2 = torch.randint(0, card, (3, 50), generator=g)
    cnt = [50, 7, 31]
    st2 = bs.ac_encode(sym2.cuda(), cdf2, n_sym=cnt)
    for b, n in enumerate(cnt):
        assert st2[b] == bs.ac_encode(sym2[b:b + 1, :n].contiguous().cuda(), cdf2[b:b + 1, :n].contiguous())[0], b
    back2 = bs.ac_decode(st2, 50, cdf2, n_sym=cnt).cpu()
    for b, n in enumerate(cnt):
        assert torch.equal(back2[b, :n], sym2[b, :n].to(torch.int32)) and not back2[b, n:].any(), b
    # containers: a list of lengths in one call = the items' own containers, plain and static; and back
    fr = [16, 1, 9, 24]
    cz = codes[:, :4].clone()
    for b, f in enumerate(fr):
        cz[:, b, f:] = 0
    als = [f * 320 for f in fr]
    for table in (None, cdf):
        blobs = bs.compress_codes(cz.cuda(), als, static_cdf=table)
        for b, f in enumerate(fr):
            assert blobs[b] == bs.compress_codes(cz[:, b:b + 1, :f].contiguous().cuda(), als[b], static_cdf=table)[0], (b, table is None)
        back3, metas = bs.decompress_codes(blobs, static_cdf=table, ragged=True)
        assert torch.equal(back3.cpu(), cz) and [m["al"] for m in metas] == als


# ---------------------------------------------------------------------------------------------------------------- 4. receiver
@pytest.mark.parametrize("mode", ["ddpm", "ddim0", "ddim1"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_decode_codes_ragged(tag, dtype, mode):
    s = setup(tag)
    e = engine(tag, dtype)
    ref = from_wav(s, mode)
    t_start, eta = MODES[mode]
    got = e.decode_codes_ragged(codes=ref["codes"].cuda(), frames=s["frames"], n_steps=N_STEPS, t_start=t_start, eta=eta, noise=s["noise_dev"],
                                want_stages=True)
    got = {k: v.cpu() for k, v in got.items()}
    assert torch.equal(got["cond"], ref["cond"])               # the front end is fp32 on every engine
    zeros_behind(s, got)
    if dtype == "f32":
        for k in ("latents", "wav"):
            v = rel(got[k].numpy(), ref[k].numpy())
            print(f"{tag} {mode} f32 {k} vs decode_ragged: {v:.3e}")
            assert v < F32_FLOOR, (k, v)
        return
    for b, (n, r) in enumerate(zip(s["lens"], oracle_items(s, mode))):
        if mode == "ddpm":                                      # (test_gpu_ragged.py checks the DDIM chain on the waveform alone)
            v = rel(got["latents"][b:b + 1, :, :n // s["hop"]].numpy(), r["latents"].numpy())
            print(f"{tag} {mode} bf16 latents item {b} vs oracle: {v:.3e}")
            check(dtype, "chain_small", v, (tag, mode, "latents", b))
        check_wav(dtype, rel(got["wav"][b:b + 1, :, :n].numpy(), r["wav"].numpy()), (tag, mode, "wav", b))


# --------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_come_before_any_gpu_work():
    s = setup("r84")
    e = engine("r84", "f32")
    codes = from_wav(s, "ddpm")["codes"].cuda()
    lib = L.load()
    out = torch.empty(3, 1, s["Tmax"], device="cuda")
    e8 = engine("r84", "fp8")
    torch.cuda.synchronize()
    before = lib.ldc_debug_sync_count()
    for bad in ([16, 9, 24], [16, 0, 24], [16, 32, 24]):       # off the quantum of 8 frames; empty; longer than Fmax
        with pytest.raises(L.LdcError) as ei:
            e.decode_codes_ragged(codes=codes, frames=bad, n_steps=N_STEPS)
        assert ei.value.code == L.E_INVALID and "condition frames" in str(ei.value), bad
    with pytest.raises(L.LdcError) as ei:                       # a row too short for its longest item
        e.decode_codes_ragged(packed=torch.zeros(3, packed_bytes(6, 24, 10) - 1, dtype=torch.uint8).cuda(), n_q=6, F=24, frames=s["frames"],
                              n_steps=N_STEPS)
    assert ei.value.code == L.E_INVALID and "packed_stride" in str(ei.value)
    fr = (C.c_int32 * 3)(*s["frames"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cp, pp in ((None, None), (codes.data_ptr(), codes.data_ptr())):
        rc = lib.ldc_decode_codes_ragged(e._ctx, cp, pp, 1 << 20, 10, 6, 3, s["Fmax"], fr, 0, N_STEPS, 0.0, None, out.data_ptr(), None, None, stream)
        assert rc == L.E_INVALID and "exactly one of codes / packed" in lib.ldc_last_error().decode()
    with pytest.raises(L.LdcError) as ei:
        e8.decode_codes_ragged(codes=codes, frames=s["frames"], n_steps=N_STEPS)
    assert ei.value.code == L.E_INVALID and "fp8 engine" in str(ei.value)
    with pytest.raises(L.LdcError):                             # the sender: a length off the cond hop, one beyond Tmax
        e.get_cond_ragged(s["wav"].cuda(), [s["lens"][0], 321, s["lens"][2]])
    with pytest.raises(L.LdcError):
        e.get_cond_ragged(s["wav"].cuda(), [s["lens"][0], s["Tmax"] + 320, s["lens"][2]])
    assert lib.ldc_debug_sync_count() == before
    assert bool(torch.isfinite(e.decode_codes_ragged(codes=codes, frames=s["frames"], n_steps=2)).all())


# ------------------------------------------------------------------------------------------------------------ 6. graph reuse
def test_one_graph_serves_every_set_of_lengths_and_both_sources():
    """The step graphs decode_ragged captured for (B, Tmax) are the ones decode_codes_ragged replays at (B, Fmax), for any lengths:
    no call waits for the device (a re-capture or an eviction would) and every call replays as many graphs as the warm decode_ragged
    (a call that captures runs its first step eagerly and replays fewer)."""
    s = setup("r84")
    e = engine("r84", "f32")
    wav, noise = s["wav"].cuda(), s["noise_dev"]
    codes = from_wav(s, "ddpm")["codes"].cuda()
    e.decode_ragged(wav, s["lens"], N_STEPS, noise=noise)       # plans built, graphs captured (the state lives in the engine's scratch)
    torch.cuda.synchronize()
    e.host_stats(reset=True)
    e.decode_ragged(wav, s["lens"], N_STEPS, noise=noise)
    torch.cuda.synchronize()
    warm = e.host_stats(reset=True)[2]
    assert warm > 0
    before = L.load().ldc_debug_sync_count()
    other = [8, 24, 16]
    outs = []
    for frames in (s["frames"], other):
        outs.append(e.decode_codes_ragged(codes=codes, frames=frames, n_steps=N_STEPS, noise=noise).cpu())
        torch.cuda.synchronize()
        assert e.host_stats(reset=True)[2] == warm, frames
    assert L.load().ldc_debug_sync_count() == before
    assert rel(outs[0].numpy(), from_wav(s, "ddpm")["wav"].numpy()) < F32_FLOOR
    for b, f in enumerate(other):                               # (item 1 reads 16 frames of zero codes behind its own 8: valid codes)
        assert not outs[1][b, :, f * 320:].any() and outs[1][b, :, :f * 320].any()


# ---------------------------------------------------------------------------------------------------------------------- 7. CLI
def _flags(tmp_path, ind, outd, *extra):
    return ["--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff",
            "--scaling_global", "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
            "--diff_dims", "32", "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", str(N_STEPS),
            "--dtype", "f32", "--batch_size", "4", *extra]


def test_cli_compress_and_decompress_ragged(tmp_path):
    from scipy.io import wavfile
    from ladiffcodec_amd import compress, decompress
    from ladiffcodec_amd.bitstream import ecdc_container
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"), ddp_prefix=True)
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind = tmp_path / "in"
    ind.mkdir()
    ns = {"a.wav": 5120 + 100, "b.wav": 2560 + 300, "c.wav": 7680 + 639, "d.wav": 5120}     # trimmed to 640: 5120, 2560, 7680, 5120
    for k, (name, n) in enumerate(ns.items()):
        wavfile.write(str(ind / name), 16000, (synth.synthetic_wav(1, n, seed=180 + k)[0, 0] * 0.5).astype(np.float32))
    enc_p, enc_r = tmp_path / "enc_plain", tmp_path / "enc_ragged"
    assert len(compress.main(_flags(tmp_path, ind, enc_p))) == 4
    assert len(compress.main(_flags(tmp_path, ind, enc_r, "--ragged", "--ragged_waste", "0.5"))) == 4     # one batch of four
    for name in ns:
        assert (enc_r / (name[:-4] + ".ecdc")).read_bytes() == (enc_p / (name[:-4] + ".ecdc")).read_bytes(), name

    tapes = {i: torch.randn(N_STEPS, 1, 128, 7680 // 32, generator=torch.Generator().manual_seed(9200 + i)) for i in range(5)}
    provider = lambda idxs, n_steps, Lz: torch.cat([tapes[i][:n_steps, :, :, :Lz] for i in idxs], dim=1)   # noqa: E731

    def run(src, dst, *extra):
        a = decompress.build_parser().parse_args(_flags(tmp_path, src, dst, *extra))
        a.noise_provider = provider
        return decompress.decompress(a)

    got_d, ref_d = tmp_path / "got", tmp_path / "ref"
    assert len(run(enc_r, got_d, "--ragged", "--ragged_waste", "0.5")) == 4
    assert len(run(enc_r, ref_d)) == 4
    for name, n in ns.items():
        y, r = wavfile.read(str(got_d / name))[1], wavfile.read(str(ref_d / name))[1]
        assert y.shape == (n // 640 * 640,) and r.shape == y.shape, name
        v = rel(y, r)
        print(f"{name}: ragged vs per-length decompress {v:.3e}")
        assert v < F32_FLOOR, (name, v)
    # a container off the receiver's quantum (18 frames): the plan keeps it out of the ragged batches, and the engine refuses its
    # length as it does without the flag (see the module docstring)
    (enc_r / "e.ecdc").write_bytes(ecdc_container([bytes(packed_bytes(6, 18, 10))], 5760, 6))
    src = decompress.EcdcSource(sorted(str(p) for p in enc_r.glob("*.ecdc")), 6)
    work = src.plan_ragged(0, 1, 4, 0.5, 2560)
    assert sorted(len(i) for i, _, rag in work if rag) == [4] and [(i, rag) for i, _, rag in work if not rag] == [([4], False)]
    for extra in (("--ragged",), ()):
        with pytest.raises(L.LdcError) as ei:
            run(enc_r, tmp_path / "none", *extra)
        assert ei.value.code == L.E_INVALID, extra
