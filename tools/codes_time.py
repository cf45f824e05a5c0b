"""Waveform decode against decode from RVQ codes at the BASELINE configs[1] shape (32 x 2.4 s, diff_dims 256, enc_ratios 8 4, bf16
UNet, 50 DDPM steps, synthetic weights), in one process on one engine: Engine.decode(wav), Engine.decode_codes(codes) (int64) and
Engine.decode_codes(packed) (the 10-bit BitPacker payload), alternated round by round and timed with device events after warm-up.
Prints one line per path (median ms per batch) and a JSON line.  The dequantisation kernel's own time comes from a kernel trace:

    python tools/codes_time.py [rounds]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/codes_time.py 2     (kernel rvq_dequant_kernel in the stats)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from ladiffcodec_amd import lib as L, synth
    from ladiffcodec_amd.bitstream import Bitstream
    from ladiffcodec_amd.model import Engine
    from ladiffcodec_amd.spec import CodecConfig, UnetConfig
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    B, T = 32, int(2.4 * 16000) // 640 * 640
    cc = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0)
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
    e = Engine(mc, u, cc, dtype="bf16", device=0, noise_seed=4321)
    e.load_state_dict(L.MODEL_MAIN, synth.ladiff_state_dict(mc, u, seed=1))
    e.load_state_dict(L.MODEL_COND, synth.codec_state_dict(cc, seed=0))
    e.finalize(strict=True)
    wav = torch.from_numpy(synth.synthetic_wav(B, T, seed=3)).cuda() * 0.5
    _, codes = e.get_cond(wav, return_codes=True)
    packed = Bitstream(e).pack_codes(codes, 10)
    n_q, F = codes.shape[0], codes.shape[2]
    runs = {"decode_wav": lambda: e.decode(wav, 50, per_item=True),
            "decode_codes_int64": lambda: e.decode_codes(codes=codes, n_steps=50, per_item=True),
            "decode_codes_packed": lambda: e.decode_codes(packed=packed, n_q=n_q, F=F, n_steps=50, per_item=True)}
    for fn in runs.values():          # warm-up: plans, graph captures, code objects
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
    for k, v in ms.items():
        print(f"{k}: median {res[k]:.2f} ms per batch of {B} x {T / 16000:.1f} s (min {min(v):.2f}, max {max(v):.2f}, {rounds} rounds)")
    print(json.dumps({"ms_per_batch": res, "batch": B, "seconds": T / 16000, "n_q": n_q, "rounds": rounds}))
    e.close()


if __name__ == "__main__":
    main()
