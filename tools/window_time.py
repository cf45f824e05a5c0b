"""Coupled windows against independent chunks on one 30 s recording: bf16, diff_dims 256, enc_ratios 8 4,
synthetic weights; windows of 1200 latent frames (2.4 s) overlapping by 200, which gives 15 windows over the 15 000 frames.

Timed with device events after warm-up, alternated round by round, as the marginal ms per step (a 40-step call minus a 20-step call,
over 20):
  windows / windows_at_split1   Engine.denoise_windows of the recording at the default split and at `split` 1 (one batch part of 15
                   windows either way)
  chunks_split1    the independent-chunk denoise of the same recording -- Engine.denoise of its 12 chunks of 1200 frames as one batch
                   plus its 560-frame tail -- as one part
  chunks_default   the same at the engine's default split (two parts on two streams)
  items15_split1 / items15_default   Engine.denoise of the 15 windows as independent items: the UNet work of `windows`, uncoupled
and the launches of one step (step list + the step's first kernel + its update launch) of `windows` and of a one-part batch of 15.

    python tools/window_time.py [rounds]

`--kernels`: only a few windows calls and a few one-part denoise calls at B = 15, for a run under
`rocprofv3 --kernel-trace --stats -- python tools/window_time.py --kernels`, whose kernel statistics then hold windows_group_update_kernel
next to p_sample_update_kernel at B = 15.

`--dpm`: instead of the above, at the default split and alternated round by round in the same way,
  ddim_windows / dpm_windows   Engine.ddim_sample_windows (eta 0) and Engine.dpm_sample_windows from t_start 100, marginal ms per step
  decode_wav / decode_codes    one 20-step Engine.decode_windows of the 30 s waveform and one Engine.decode_codes_windows of its codes, ms
                   per call (the code-driven call skips the cond encoder and the quantiser).

`--group`: instead of the above, at `split` 1 and alternated round by round in the same way, marginal ms per step of
  group_2x15       Engine.sample_windows_group of TWO such recordings: 30 windows in one batch ("Several
                   recordings per call")
  two_single_calls Engine.denoise_windows of the one and then of the other (the figure is per step of BOTH: two steps of 15 windows)
  items30_split1   Engine.denoise of the 30 windows as independent items: the same batch without the blend"""
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
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv[1:]
    dpm_mode = "--dpm" in sys.argv[1:]
    rounds = int(argv[0]) if argv else 5
    Ltot, Lw, O_, up = 15000, 1200, 200, 10
    cc = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0)
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
    e = Engine(mc, u, cc, dtype="bf16", device=0, noise_seed=4321)
    e.load_state_dict(L.MODEL_MAIN, synth.ladiff_state_dict(mc, u, seed=1))
    e.load_state_dict(L.MODEL_COND, synth.codec_state_dict(cc, seed=0))
    e.finalize(strict=True)
    starts, _ = e.window_layout(Ltot, Lw, O_)
    W = len(starts)
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(1, 128, Ltot // up, generator=g).cuda()
    img = e.cond_upsample(cond, 1)
    cut = lambda x, first, n: torch.cat([x[..., a:a + n] for a in first]).contiguous()      # noqa: E731
    chunk0 = [k * Lw for k in range(Ltot // Lw)]
    tail0, tail = len(chunk0) * Lw, (Ltot - len(chunk0) * Lw) // 80 * 80
    cimg, ccond = cut(img, chunk0, Lw), cut(cond, [a // up for a in chunk0], Lw // up)
    timg, tcond = img[..., tail0:tail0 + tail].contiguous(), cond[..., tail0 // up:(tail0 + tail) // up].contiguous()
    wimg, wcond = cut(img, starts, Lw), cut(cond, [a // up for a in starts], Lw // up)

    def chunks(n):
        e.denoise(cimg, ccond, n)
        return e.denoise(timg, tcond, n)

    windows = lambda n: e.denoise_windows(img, cond, n, Lw, O_)      # noqa: E731
    items15 = lambda n: e.denoise(wimg, wcond, n)                    # noqa: E731
    if kernels_only:
        e.set_option("split", 1)
        for _ in range(3):
            assert bool(torch.isfinite(windows(20)).all())
            assert bool(torch.isfinite(items15(20)).all())
        torch.cuda.synchronize()
        e.close()
        return
    if "--group" in sys.argv[1:]:
        # a second recording of the same length; everything at `split` 1 (a windows plan is one part anyway)
        cond2 = torch.randn(1, 128, Ltot // up, generator=g).cuda()
        img2 = e.cond_upsample(cond2, 1)
        wimg2, wcond2 = cut(img2, starts, Lw), cut(cond2, [a // up for a in starts], Lw // up)
        iimg, icond = torch.cat([wimg, wimg2]).contiguous(), torch.cat([wcond, wcond2]).contiguous()
        e.set_option("split", 1)

        def two_singles(n):
            e.denoise_windows(img, cond, n, Lw, O_)
            return e.denoise_windows(img2, cond2, n, Lw, O_)
        timed(e, torch, rounds, {"group_2x15": lambda n: e.sample_windows_group([img, img2], [cond, cond2], n, Lw, O_, seeds=[11, 12])[1],
                                 "two_single_calls": two_singles,
                                 "items30_split1": lambda n: e.denoise(iimg, icond, n)}, 2 * W, 2 * Ltot, Lw, O_)
        e.close()
        return
    if dpm_mode:
        timed(e, torch, rounds, {"ddim_windows": lambda n: e.ddim_sample_windows(img, cond, 100, n, Lw, O_, eta=0.0),
                                 "dpm_windows": lambda n: e.dpm_sample_windows(img, cond, 100, n, Lw, O_)}, W, Ltot, Lw, O_)
        wav = (torch.from_numpy(synth.synthetic_wav(1, Ltot * 32, seed=7)) * 0.5).cuda()
        codes = e.get_cond(wav, return_codes=True)[1]
        calls = {"decode_wav": lambda: e.decode_windows(wav, 20, Lw, O_), "decode_codes": lambda: e.decode_codes_windows(codes=codes, n_steps=20, Lw=Lw, overlap=O_)}
        for fn in calls.values():
            fn(), fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = fn()
                b.record()
                b.synchronize()
                assert bool(torch.isfinite(out).all()), k
                ms[k].append(a.elapsed_time(b))
        for k, v in ms.items():
            print(f"{k}: {statistics.median(v):.2f} ms per 20-step call (min {min(v):.2f}, max {max(v):.2f}, {rounds} rounds)")
        print(json.dumps({"ms_per_call": {k: round(statistics.median(v), 3) for k, v in ms.items()}, "rounds": rounds}))
        e.close()
        return
    # launches of one step: the step list in profile mode (eager, one event pair per op) + the step's first kernel + its update launch
    e.set_option("split", 1)
    launches = {}
    for name, fn in (("windows", windows), ("items15_split1", items15)):
        e.profile(True)
        fn(3)
        launches[name] = sum(r[2] for r in e.profile_read_classes()) // 3 + 2
        e.profile(False)
    # a change of `split` rebuilds every plan, so the arrangements are timed split by split: set once, warmed (plans, captures), then
    # alternated round by round
    groups = {1: {"windows_at_split1": windows, "chunks_split1": chunks, "items15_split1": items15},
              2: {"windows": windows, "chunks_default": chunks, "items15_default": items15}}
    ms = {}
    for split, runs in groups.items():
        e.set_option("split", split)
        for fn in runs.values():
            for n in (20, 40, 20, 40):
                fn(n)
        torch.cuda.synchronize()
        for k in runs:
            ms[k] = []
        for _ in range(rounds):
            for k, fn in runs.items():
                t = []
                for n in (20, 40):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    out = fn(n)
                    b.record()
                    b.synchronize()
                    assert bool(torch.isfinite(out).all()), k
                    t.append(a.elapsed_time(b))
                ms[k].append((t[1] - t[0]) / 20.0)
    res = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k}: {res[k]:.3f} ms per step (min {min(v):.3f}, max {max(v):.3f}, {rounds} rounds)")
    print(f"launches per step: windows {launches['windows']}, one part of {W} items {launches['items15_split1']}")
    print(json.dumps({"ms_per_step": res, "launches_per_step": launches, "windows": W, "Ltot": Ltot, "Lw": Lw, "overlap": O_, "rounds": rounds}))
    e.close()


def timed(e, torch, rounds, runs, W, Ltot, Lw, O_):
    """marginal ms per step of every loop of `runs` (a 40-step call minus a 20-step call, over 20), warmed, alternated round by round"""
    for fn in runs.values():
        for n in (20, 40, 20, 40):
            fn(n)
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t = []
            for n in (20, 40):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = fn(n)
                b.record()
                b.synchronize()
                assert bool(torch.isfinite(out).all()), k
                t.append(a.elapsed_time(b))
            ms[k].append((t[1] - t[0]) / 20.0)
    res = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k}: {res[k]:.3f} ms per step (min {min(v):.3f}, max {max(v):.3f}, {rounds} rounds)")
    print(json.dumps({"ms_per_step": res, "windows": W, "Ltot": Ltot, "Lw": Lw, "overlap": O_, "rounds": rounds}))
    return res


if __name__ == "__main__":
    main()
