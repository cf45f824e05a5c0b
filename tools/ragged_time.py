"""Ragged decode timings at the BASELINE configs[1] model (diff_dims 256, enc_ratios 8 4, bf16 UNet, synthetic weights).

    python tools/ragged_time.py --case plan [--rounds 5]
        32 x 2.4 s, 50 DDPM steps, all lengths equal: Engine.decode (the fused plan) against Engine.decode_ragged (the unfused,
        length-aware plan) on one engine, alternated round by round, device-event timed after warm-up; the shader clock of the
        timed region is reported as bench.py reports it.
    python tools/ragged_time.py --case corpus [--files 256] [--waste 0.1 0.25 0.5]
        a seeded synthetic corpus of mono files with lengths uniform over 1.6-16 s on the 2560-sample quantum, decoded through the
        CLI path (sample.decode_files, one engine) without --ragged and with --ragged at every --waste: audio-seconds per
        wall-second, mean batch size and padded fraction per setting.  --codes: the corpus is compressed once (compress --ragged's
        path, untimed) and the settings decode its CONTAINERS (decompress's path: EcdcSource, Engine.decode_codes[_ragged]).

Each case is one process; run each under its own `timeout`, chained, nothing retried.  Prints text lines and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_engine():
    from ladiffcodec_amd import lib as L, synth
    from ladiffcodec_amd.model import Engine
    from ladiffcodec_amd.spec import CodecConfig, UnetConfig
    cc = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0)
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
    e = Engine(mc, u, cc, dtype="bf16", device=0, noise_seed=4321)
    e.load_state_dict(L.MODEL_MAIN, synth.ladiff_state_dict(mc, u, seed=1))
    e.load_state_dict(L.MODEL_COND, synth.codec_state_dict(cc, seed=0))
    e.finalize(strict=True)
    return e


def shader_mhz(e, fn):
    """shader clock over one call of fn: shader cycles / 100 MHz wall ticks between two device clock samples"""
    import ctypes as C
    from ladiffcodec_amd import lib as L
    a, b = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    s = C.c_void_p(e.stream.cuda_stream)
    L.check(e.lib.ldc_clock_sample(e._ctx, a, s))
    fn()
    L.check(e.lib.ldc_clock_sample(e._ctx, b, s))
    return (b[1] - a[1]) / max(1, b[0] - a[0]) * 100.0


def case_plan(rounds):
    import torch
    from ladiffcodec_amd import synth
    B, T = 32, 38400
    e = build_engine()
    wav = torch.from_numpy(synth.synthetic_wav(B, T, seed=3)).cuda() * 0.5
    runs = {"decode_fused": lambda: e.decode(wav, 50, per_item=True),
            "decode_ragged_equal": lambda: e.decode_ragged(wav, [T] * B, 50)}
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            assert bool(torch.isfinite(out).all()), k
            ms[k].append(a.elapsed_time(b))
    res = {k: round(statistics.median(v), 2) for k, v in ms.items()}
    mhz = {k: round(shader_mhz(e, fn)) for k, fn in runs.items()}
    for k, v in ms.items():
        print(f"{k}: median {res[k]:.2f} ms per batch of {B} x {T / 16000:.1f} s (min {min(v):.2f}, max {max(v):.2f}, {rounds} rounds), shader clock {mhz[k]} MHz")
    print(json.dumps({"case": "plan", "ms_per_batch": res, "shader_mhz": mhz, "batch": B, "seconds": T / 16000, "rounds": rounds}))
    e.close()


def case_corpus(n_files, wastes, batch_size, codes=False):
    import numpy as np
    import torch
    from scipy.io import wavfile
    from ladiffcodec_amd import sample, synth
    q = 2560
    rng = np.random.default_rng(2024)
    lens = [int(v) * q for v in rng.integers(16000 * 16 // 10 // q, 16000 * 16 // q + 1, size=n_files)]
    e = build_engine()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ind = os.path.join(tmp, "in")
        os.makedirs(ind)
        base = synth.synthetic_wav(1, max(lens), seed=9)[0, 0] * 0.5
        files = []
        for k, n in enumerate(lens):
            files.append(os.path.join(ind, f"f{k:04d}.wav"))
            wavfile.write(files[-1], 16000, np.roll(base, 37 * k)[:n].astype(np.float32))
        files.sort()
        order = [int(os.path.basename(f)[1:5]) for f in files]
        flen = [lens[k] for k in order]
        source = sampler = None
        if codes:     # the receiver's side: the same files as containers (names keep the order)
            from ladiffcodec_amd import compress, decompress
            enc = os.path.join(tmp, "enc")
            cargs = sample.build_parser().parse_args(["--model_for_cond", "x", "--input_dir", ind + "/", "--output_dir", enc + "/",
                                                      "--batch_size", str(batch_size), "--ragged"])
            files = sorted(compress.compress_files(e, files, cargs))
            source = decompress.EcdcSource(files, e.cond_codec.n_q_layers)
            sampler = sample.CodesSampler(sample.DdpmSampler(50))
        for label, extra in [("equal_length", [])] + [(f"ragged_w{w}", ["--ragged", "--ragged_waste", str(w)]) for w in wastes]:
            args = sample.build_parser().parse_args(["--model_for_cond", "x", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2",
                                                     "--input_dir", ind + "/", "--output_dir", os.path.join(tmp, label) + "/",
                                                     "--midway_t", "50", "--batch_size", str(batch_size)] + extra)
            ragged, waste = sample.ragged_options(args)
            if ragged and codes:
                work = [w[:2] for w in source.plan_ragged(0, 1, batch_size, waste, q)]
            elif ragged:
                work = sample.plan_ragged_batches(flen, [1] * n_files, 0, 1, batch_size, waste, q)
            else:
                work = sample.plan_batches(flen, [1] * n_files, 0, 1, batch_size)
            padded = sum(len(ix) * max(flen[i] for i in ix) for ix, _ in work)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            written = sample.decode_files(e, files, args, 0, 1, 0, sampler=sampler, source=source)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(written) == n_files
            out[label] = {"audio_s_per_wall_s": round(sum(flen) / 16000 / dt, 1), "wall_s": round(dt, 2), "batches": len(work),
                          "mean_batch": round(n_files / len(work), 2), "padded_fraction": round(1.0 - sum(flen) / padded, 4)}
            print(label, out[label])
    print(json.dumps({"case": "corpus_codes" if codes else "corpus", "files": n_files, "audio_s": sum(lens) / 16000, "results": out}))
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["plan", "corpus"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--waste", type=float, nargs="+", default=[0.1, 0.25, 0.5])
    ap.add_argument("--codes", action="store_true", help="--case corpus: decode the corpus' containers instead of its waveforms")
    a = ap.parse_args()
    if a.case == "plan":
        case_plan(a.rounds)
    else:
        case_corpus(a.files, a.waste, a.batch_size, a.codes)


if __name__ == "__main__":
    main()
