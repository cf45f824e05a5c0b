"""Per-call latency of a cond-encoder stream session (ldc_get_cond_stream) next to ldc_get_cond on the joined sequence.

    python tools/stream_time.py [--rounds 20] [--lstm coop|stream|both]
        cond codec (ratios 8 5 4 2, H = 512), synthetic weights, fp32 codec ends.  For B = 1 and 32 and chunks of 1, 8 and 120 frames
        (20 ms, 160 ms, 2.4 s): a stream session is warmed with a first chunk, then `rounds` further chunks are pushed, each call timed
        with device events on the engine's stream; the whole-sequence ldc_get_cond on rounds x chunk frames is timed the same way.  The
        LSTM kernel a chunk takes follows the whole-sequence rule (B <= 2: the XCD-local cooperative kernel, else the chip-wide one);
        --lstm stream repeats every case with option lstm_stream = 1 (one workgroup per item, W_hh streamed from L2), which is how the
        per-chunk kernel choice is measured.

One process; run it under its own `timeout`, nothing retried.  Prints text lines and one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_engine():
    from ladiffcodec_amd import lib as L, synth
    from ladiffcodec_amd.model import Engine
    from ladiffcodec_amd.spec import CodecConfig, UnetConfig
    cc = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0)
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=32, upsampling_ratios=(5, 2), unet_scale_cond=True)
    e = Engine(mc, u, cc, dtype="f32", device=0)
    e.load_state_dict(L.MODEL_MAIN, synth.ladiff_state_dict(mc, u, seed=1))
    e.load_state_dict(L.MODEL_COND, synth.codec_state_dict(cc, seed=0))
    e.finalize(strict=True)
    return e


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--lstm", choices=["coop", "stream", "both"], default="both")
    a = ap.parse_args()
    import torch
    from ladiffcodec_amd import lib as L, synth
    e = build_engine()
    results = []
    for stream_only in ([0], [1], [0, 1])[("coop", "stream", "both").index(a.lstm)]:
        e.set_option("lstm_stream", stream_only)
        for B in (1, 32):
            kernel = "streamed" if stream_only else ("xcd-local cooperative" if B <= 2 else "chip-wide cooperative")
            for frames in (1, 8, 120):
                T = frames * 320
                first = max(T, 2240)
                wav = torch.from_numpy(synth.synthetic_wav(B, first + (a.rounds + 3) * T, seed=3)).cuda() * 0.5
                st = e.open_stream(L.MODEL_COND, L.STREAM_ENCODER, B)
                st.get_cond(wav[..., :first])
                at, ms = first, []
                for k in range(a.rounds + 3):
                    t, out = timed(lambda: st.get_cond(wav[..., at:at + T].contiguous()))
                    at += T
                    if k >= 3:
                        ms.append(t)
                assert bool(torch.isfinite(out).all())
                st.close()
                joined = wav[..., :max(2240, a.rounds * T)].contiguous()
                whole = [timed(lambda: e.get_cond(joined))[0] for _ in range(6)][3:]
                r = {"B": B, "chunk_frames": frames, "lstm_kernel": kernel, "stream_call_ms": round(statistics.median(ms), 3),
                     "stream_call_min_ms": round(min(ms), 3), "stream_call_max_ms": round(max(ms), 3),
                     "whole_frames": joined.shape[-1] // 320, "whole_call_ms": round(statistics.median(whole), 3)}
                results.append(r)
                print(f"B {B:2d} chunk {frames:3d} frames, {kernel} LSTM: stream call median {r['stream_call_ms']:.3f} ms (min {r['stream_call_min_ms']:.3f}, max "
                      f"{r['stream_call_max_ms']:.3f}, {a.rounds} calls); get_cond on {r['whole_frames']} frames {r['whole_call_ms']:.3f} ms")
    e.set_option("lstm_stream", 0)
    print(json.dumps({"case": "stream_time", "rounds": a.rounds, "results": results}))
    e.close()


if __name__ == "__main__":
    main()
