"""DDPM against DDIM decode time at the BASELINE configs[1] shape (32 x 2.4 s, diff_dims 256, enc_ratios 8 4, bf16 UNet, synthetic
weights), in one process on one engine: DDPM 50 steps, DDIM from t_start 50 with S = 10 and S = 25, alternated round by round
and timed with device events after warm-up.  Prints one line per sampler (median ms per batch) and a JSON line.

    python tools/ddim_time.py [rounds]

`--dpm`: the DPM-Solver++(2M) denoise loop beside the DDIM loop instead (Engine.dpm_sample / Engine.ddim_sample at eta 0 on one start
image and condition, no codec ends), from t_start 50 with S = 10 and S = 20; per sampler the median ms per call, that over S, and the
marginal ms per step (S = 20 minus S = 10, over 10) with the spread of the rounds.

    python tools/ddim_time.py --dpm [rounds]

`--seeded`: the item-seeded denoise loop (Engine.sample_seeded) beside the unseeded Philox loop (Engine.denoise /
Engine.ddim_sample at eta 1 with noise=None) on one start image and condition, no codec ends, at S = 10 and S = 20 steps; per loop the
median ms per call and the marginal ms per step (S = 20 minus S = 10, over 10) with the spread of the rounds.

    python tools/ddim_time.py --seeded [rounds]
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
    from ladiffcodec_amd.model import Engine
    from ladiffcodec_amd.spec import CodecConfig, UnetConfig
    argv = [a for a in sys.argv[1:] if a not in ("--dpm", "--seeded")]
    dpm = "--dpm" in sys.argv[1:]
    seeded = "--seeded" in sys.argv[1:]
    rounds = int(argv[0]) if argv else 5
    B, T = 32, int(2.4 * 16000) // 640 * 640
    cc = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0)
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
    e = Engine(mc, u, cc, dtype="bf16", device=0, noise_seed=4321)
    e.load_state_dict(L.MODEL_MAIN, synth.ladiff_state_dict(mc, u, seed=1))
    e.load_state_dict(L.MODEL_COND, synth.codec_state_dict(cc, seed=0))
    e.finalize(strict=True)
    wav = torch.from_numpy(synth.synthetic_wav(B, T, seed=3)).cuda() * 0.5
    runs = {"ddpm_50": lambda: e.decode(wav, 50, per_item=True),
            "ddim_50_s10": lambda: e.decode_ddim(wav, 50, 10, 0.0, per_item=True),
            "ddim_50_s25": lambda: e.decode_ddim(wav, 50, 25, 0.0, per_item=True)}
    if dpm:
        cond = e.get_cond(wav)
        up = e.cond_upsample(cond, 0)
        img = up / (up.abs().amax(dim=(1, 2), keepdim=True) + 1e-8)
        runs = {"ddim_loop_s10": lambda: e.ddim_sample(cond, 50, 10, 0.0, img=img), "dpm_loop_s10": lambda: e.dpm_sample(cond, 50, 10, img),
                "ddim_loop_s20": lambda: e.ddim_sample(cond, 50, 20, 0.0, img=img), "dpm_loop_s20": lambda: e.dpm_sample(cond, 50, 20, img)}
    if seeded:
        cond = e.get_cond(wav)
        up = e.cond_upsample(cond, 0)
        img = up / (up.abs().amax(dim=(1, 2), keepdim=True) + 1e-8)
        seeds = [1000 + b for b in range(B)]
        runs = {}
        for s in (10, 20):
            runs[f"ddpm_philox_s{s}"] = lambda s=s: e.denoise(img, cond, s)
            runs[f"ddpm_seeded_s{s}"] = lambda s=s: e.sample_seeded(img, cond, seeds, s)
            runs[f"ddim_philox_s{s}"] = lambda s=s: e.ddim_sample(cond, 50, s, 1.0, img=img)
            runs[f"ddim_seeded_s{s}"] = lambda s=s: e.sample_seeded(img, cond, seeds, s, sampler="ddim", t_start=50, eta=1.0)
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
    if dpm:
        for name in ("ddim", "dpm"):
            a, b = ms[f"{name}_loop_s10"], ms[f"{name}_loop_s20"]
            marg = [(y - x) / 10.0 for x, y in zip(a, b)]
            res[f"{name}_ms_per_step"] = round(statistics.median(marg), 4)
            print(f"{name}: {res[name + '_loop_s10'] / 10:.3f} ms per step at S = 10, {res[name + '_loop_s20'] / 20:.3f} at S = 20; marginal "
                  f"{statistics.median(marg):.3f} ms per step (min {min(marg):.3f}, max {max(marg):.3f} over {rounds} rounds)")
    if seeded:
        for name in ("ddpm_philox", "ddpm_seeded", "ddim_philox", "ddim_seeded"):
            a, b = ms[f"{name}_s10"], ms[f"{name}_s20"]
            marg = [(y - x) / 10.0 for x, y in zip(a, b)]
            res[f"{name}_ms_per_step"] = round(statistics.median(marg), 4)
            print(f"{name}: {res[name + '_s10'] / 10:.3f} ms per step at S = 10, {res[name + '_s20'] / 20:.3f} at S = 20; marginal "
                  f"{statistics.median(marg):.3f} ms per step (min {min(marg):.3f}, max {max(marg):.3f} over {rounds} rounds)")
    print(json.dumps({"ms_per_batch": res, "batch": B, "seconds": T / 16000, "rounds": rounds}))
    e.close()


if __name__ == "__main__":
    main()
