"""Window groups on the GPU ("Several recordings per call"): several recordings in one windows call, one batch.
The contract is tests/windows_group_restatement.py: every recording comes out as the single-recording windows call gives it alone.  So each
case compares a group call against the restatement on the CPU oracle AND against the engine's own single-recording calls.

Groups (Lw, overlap; Ltot per recording): `r84` (80, 40; 180, 80, 240) -- 4 + 1 + 5 windows: a triple-covered stretch, a length that is no
multiple of the 32-frame tile, a one-window recording in the middle -- and `r8` (160, 40; 400, 160).  DDPM runs take 40 steps, DDIM and DPM
(40, 8).  References are computed once per process and shared; nothing writes to them.

Bars: tests/drift_tolerances.py; every test prints its figure before it asserts.  f32 keeps the generic bars throughout.  bf16 takes the
constants tests/test_gpu_windows.py and tests/test_gpu_windows_receiver.py hold for the recordings they know (Ltot 180, 400); for
everything else the bar is twice what the PARENT's path shows on the same items and tapes, the worse of two runs on MI355X, held in
PARENT_MEASURED below (`parent_figures` is how they were taken; DESIGN.md section 5g records them).  No bar comes from the group path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from helpers import CASES  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
import dpm_restatement as D  # noqa: E402
import windows_group_restatement as G  # noqa: E402
import windows_restatement as R  # noqa: E402
import test_gpu_windows as TW  # noqa: E402
import test_gpu_windows_receiver as TR  # noqa: E402

TAGS = ["r84", "r8"]
N, T_START, S = 40, 40, 8
SEEDS = [0x5EED0123, 0xFFFFFFFFFFFFFFF1, 77]                              # one per recording (a seed beyond 2^63 among them)
SAMPLERS = ["ddpm", "ddim0", "ddim1", "dpm"]

# bf16 only: the worse of two runs on MI355X of the PARENT's path (see the module docstring and parent_figures below).
#   ("solo", sampler, tag, Ltot)    the single-recording windows call of a recording no other test file has a constant for, against its
#                                   restatement: denoise_windows 40 steps / ddim_sample_windows (40, 8) eta 0, 1 / dpm_sample_windows (40, 8)
#   ("batch", sampler, tag)         Engine.denoise / ddim_sample / dpm_sample of the group's windows as INDEPENDENT items: all of them in one
#                                   batch against one batch per recording -- what a change of the batch a window sits in costs
#   ("batch_lat" | "batch_wav", sampler, tag)   Engine.decode / decode_ddim / decode_dpm of the windows' stretches likewise
PARENT_MEASURED = {
    ("solo", "ddpm", "r84", 80): 1.27e-3, ("solo", "ddpm", "r84", 240): 1.61e-3, ("solo", "ddpm", "r8", 160): 1.57e-3,
    ("solo", "ddim0", "r84", 80): 7.98e-4, ("solo", "ddim0", "r84", 240): 8.77e-4, ("solo", "ddim0", "r8", 160): 1.21e-3,
    ("solo", "ddim1", "r84", 80): 1.36e-3, ("solo", "ddim1", "r84", 240): 1.43e-3, ("solo", "ddim1", "r8", 160): 1.75e-3,
    ("solo", "dpm", "r84", 80): 8.31e-4, ("solo", "dpm", "r84", 240): 8.44e-4, ("solo", "dpm", "r8", 160): 1.05e-3,
    ("batch", "ddpm", "r84"): 5.52e-4, ("batch", "ddim0", "r84"): 7.03e-4, ("batch", "ddim1", "r84"): 1.12e-3, ("batch", "dpm", "r84"): 6.13e-4,
    ("batch", "ddpm", "r8"): 4.77e-4, ("batch", "ddim0", "r8"): 5.58e-4, ("batch", "ddim1", "r8"): 9.33e-4, ("batch", "dpm", "r8"): 7.97e-4,
    ("batch_lat", "ddpm", "r84"): 4.54e-4, ("batch_lat", "ddim0", "r84"): 5.96e-4, ("batch_lat", "ddim1", "r84"): 9.06e-4,
    ("batch_lat", "dpm", "r84"): 4.91e-4, ("batch_lat", "ddpm", "r8"): 4.56e-4, ("batch_lat", "ddim0", "r8"): 6.56e-4,
    ("batch_lat", "ddim1", "r8"): 9.98e-4, ("batch_lat", "dpm", "r8"): 7.18e-4,
    ("batch_wav", "ddpm", "r84"): 9.67e-5, ("batch_wav", "ddim0", "r84"): 1.08e-4, ("batch_wav", "ddim1", "r84"): 1.62e-4,
    ("batch_wav", "dpm", "r84"): 1.08e-4, ("batch_wav", "ddpm", "r8"): 2.39e-4, ("batch_wav", "ddim0", "r8"): 2.98e-4,
    ("batch_wav", "ddim1", "r8"): 4.45e-4, ("batch_wav", "dpm", "r8"): 2.64e-4,
}
KNOWN = {   # the recordings other files hold constants for: (sampler, tag, Ltot) -> (module, key)
    ("ddpm", "r84", 180): (TW, ("chain", "r84", 180)), ("ddpm", "r8", 400): (TW, ("chain", "r8", 400)),
    ("ddim0", "r84", 180): (TW, ("ddim", "r84", 180, 0.0)), ("ddim1", "r84", 180): (TW, ("ddim", "r84", 180, 1.0)),
    ("ddim0", "r8", 400): (TW, ("ddim", "r8", 400, 0.0)), ("ddim1", "r8", 400): (TW, ("ddim", "r8", 400, 1.0)),
    ("dpm", "r84", 180): (TR, ("dpm", "r84", 180, 40, 8)), ("dpm", "r8", 400): (TR, ("dpm", "r8", 400, 40, 8)),
}
_REF = {}


def measured(sampler, tag, Ltot):
    """the parent's figure of one recording's chain against its restatement (bf16), or None"""
    if (sampler, tag, Ltot) in KNOWN:
        mod, key = KNOWN[(sampler, tag, Ltot)]
        return mod.PARENT_MEASURED[key]
    return PARENT_MEASURED.get(("solo", sampler, tag, Ltot))


def bar(dtype, key, m=None):
    return max(TOL[dtype][key], 2.0 * m) if (m and dtype == "bf16") else TOL[dtype][key]


def close(dtype, key, value, what, m=None):
    b = bar(dtype, key, m)
    print(f"window group {dtype} {what}: {value:.3e} ({key} bar {b:.3e})")
    assert value < b, (dtype, key, what, value, b)


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def npy(xs):
    return [x.detach().cpu().numpy() for x in xs]


def gpu(s, k):
    return [i[k].cuda() for i in s]


def run_group(e, s, sampler, Lw, O_, noise=True, seeds=None):
    """the group call of one of SAMPLERS on the inputs s"""
    imgs, conds = gpu(s, "img"), gpu(s, "cond")
    if sampler == "ddpm":
        return e.sample_windows_group(imgs, conds, N, Lw, O_, noise=gpu(s, "noise") if noise else None, seeds=seeds)
    if sampler == "dpm":
        return e.sample_windows_group(imgs, conds, S, Lw, O_, sampler="dpm", t_start=T_START)
    return e.sample_windows_group(imgs, conds, S, Lw, O_, sampler="ddim", t_start=T_START, eta=float(sampler[-1]),
                                  noise=[i["noise"][:S].cuda() for i in s] if noise else None, seeds=seeds)


def run_alone(e, i, sampler, Lw, O_, noise=True):
    """the single-recording call of the same sampler on one recording's inputs"""
    img, cond = i["img"].cuda(), i["cond"].cuda()
    if sampler == "ddpm":
        return e.denoise_windows(img, cond, N, Lw, O_, noise=i["noise"].cuda() if noise else None)
    if sampler == "dpm":
        return e.dpm_sample_windows(img, cond, T_START, S, Lw, O_)
    return e.ddim_sample_windows(img, cond, T_START, S, Lw, O_, eta=float(sampler[-1]), noise=i["noise"][:S].cuda() if noise else None)


def restated(tag, sampler):
    Lw, O_, _ = G.GROUPS[tag]
    s = G.inputs(tag, N)
    a = (s[0]["sd"], s[0]["u"], [i["img"] for i in s], [i["cond"] for i in s])
    if sampler == "ddpm":
        return G.reference(tag, N)
    if sampler == "dpm":
        return cached(("dpm", tag), lambda: G.dpm_windows_group(*a, T_START, S, Lw, O_, s[0]["up"]))
    return cached((sampler, tag), lambda: G.ddim_windows_group(*a, L.ddim_times(T_START, S), float(sampler[-1]), [i["noise"] for i in s], Lw, O_, s[0]["up"]))


def windows_as_items(s, Lw, O_):
    """per recording: the windows' stretches of (img, cond, tape) as independent batch items"""
    out = []
    for i in s:
        starts, lw = R.layout(i["img"].shape[2], Lw, O_)
        up = i["up"]
        out.append((torch.cat([i["img"][..., a:a + lw] for a in starts]).contiguous(),
                    torch.cat([i["cond"][..., a // up:(a + lw) // up] for a in starts]).contiguous(),
                    torch.cat([i["noise"][..., a:a + lw] for a in starts], dim=1).contiguous()))
    return out


def wavs_of(tag):
    mc = CASES[tag][0]
    return [torch.from_numpy(synth.synthetic_wav(1, Ltot * mc.hop_length, seed=83 + r)) * 0.5 for r, Ltot in enumerate(G.GROUPS[tag][2])]


def parent_figures(tag, dtype="bf16"):
    """How PARENT_MEASURED was taken: only calls the parent commit has (run it from a script, twice, and keep the worse value per key)."""
    e = engine(tag, dtype)
    Lw, O_, lens = G.GROUPS[tag]
    s = G.inputs(tag, N)
    out = {}
    for sampler in SAMPLERS:
        ref = restated(tag, sampler)
        for r, Ltot in enumerate(lens):
            if (sampler, tag, Ltot) not in KNOWN:
                out[("solo", sampler, tag, Ltot)] = rel(run_alone(e, s[r], sampler, Lw, O_).cpu().numpy(), ref[r].numpy())

        def items(img, cond, noise):
            img, cond, noise = img.cuda(), cond.cuda(), noise.cuda()
            if sampler == "ddpm":
                return e.denoise(img, cond, N, noise)
            if sampler == "dpm":
                return e.dpm_sample(cond, T_START, S, img)
            return e.ddim_sample(cond, T_START, S, eta=float(sampler[-1]), img=img, noise=noise[:S].contiguous())
        per = windows_as_items(s, Lw, O_)
        one = items(*(torch.cat([p[k] for p in per], dim=1 if k == 2 else 0).contiguous() for k in range(3))).cpu().numpy()
        sep = np.concatenate([items(*p).cpu().numpy() for p in per])
        out[("batch", sampler, tag)] = rel(one, sep)
        mc = CASES[tag][0]
        wv = [torch.cat([w[..., a * mc.hop_length:(a + Lw) * mc.hop_length] for a in R.layout(L_, Lw, O_)[0]]).contiguous()
              for w, L_ in zip(wavs_of(tag), lens)]

        def dec(wav, noise):
            wav, noise = wav.cuda(), noise.cuda()
            if sampler == "ddpm":
                g = e.decode(wav, N, noise, per_item=True, want_stages=True)
            elif sampler == "dpm":
                g = e.decode_dpm(wav, T_START, S, per_item=True, want_stages=True)
            else:
                g = e.decode_ddim(wav, T_START, S, eta=float(sampler[-1]), noise=noise[:S].contiguous(), per_item=True, want_stages=True)
            return g["latents"].cpu().numpy(), g["wav"].cpu().numpy()
        one = dec(torch.cat(wv), torch.cat([p[2] for p in per], dim=1).contiguous())
        sep = [dec(w, p[2]) for w, p in zip(wv, per)]
        out[("batch_lat", sampler, tag)] = rel(one[0], np.concatenate([a for a, _ in sep]))
        out[("batch_wav", sampler, tag)] = rel(one[1], np.concatenate([b for _, b in sep]))
    return out


# ------------------------------------------------------------------------------------------------------------ 1. one UNet pass
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_unet_forward_windows_group(tag, dtype):
    Lw, O_, lens = G.GROUPS[tag]
    s = G.inputs(tag, N)
    xs = [i["noise"][3] * 0.5 + i["img"] for i in s]
    ref = cached(("eps", tag), lambda: G.unet_forward_windows_group(s[0]["sd"], s[0]["u"], xs, 37, [i["cond"] for i in s], Lw, O_, s[0]["up"]))
    got = npy(engine(tag, dtype).unet_forward_windows_group([x.cuda() for x in xs], 37, gpu(s, "cond"), Lw, O_))
    for r, Ltot in enumerate(lens):
        close(dtype, "eps_small", rel(got[r], ref[r].numpy()), f"{tag} recording {r} ({Ltot}) eps at t = 37")


# -------------------------------------------------------------------------------------------- 2., 3. the loops, on tapes
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_sample_windows_group(tag, dtype, sampler):
    Lw, O_, lens = G.GROUPS[tag]
    s = G.inputs(tag, N)
    e = engine(tag, dtype)
    ref = restated(tag, sampler)
    got = npy(run_group(e, s, sampler, Lw, O_))
    for r, Ltot in enumerate(lens):
        assert np.isfinite(got[r]).all()
        close(dtype, "chain_small", rel(got[r], ref[r].numpy()), f"{tag} {sampler} recording {r} ({Ltot}) against the restatement",
              measured(sampler, tag, Ltot))
        alone = run_alone(e, s[r], sampler, Lw, O_).cpu().numpy()
        close(dtype, "repeat", rel(got[r], alone), f"{tag} {sampler} recording {r} ({Ltot}) against the single-recording call",
              PARENT_MEASURED.get(("batch", sampler, tag)))
    if sampler == "ddpm" and tag == "r84":
        # what the bars must see (tests/test_windows_group_cpu.py asserts the oracle's side, 10 x the f32 bar): (a) a cover read without
        # w0_r moves the recordings behind the first, (b) a tape indexed on the packed axis moves every recording
        for mode, who in (("cover", (1, 2)), ("noise", (0, 1, 2))):
            other = G.reference(tag, N, mode=mode)
            for r in who:
                d = rel(got[r], other[r].numpy())
                print(f"window group {dtype} recording {r} against the mutant '{mode}': {d:.3e}")
                assert d > bar(dtype, "chain_small", measured(sampler, tag, lens[r])), (mode, r, d)


# ------------------------------------------------------------------------------------------------------------------ 4. Philox
@pytest.mark.parametrize("sampler", ["ddpm", "ddim1"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_philox_seeds_draw_what_the_single_call_draws_after_reseed(dtype, sampler):
    tag = "r84"
    Lw, O_, lens = G.GROUPS[tag]
    s = G.inputs(tag, N)
    e = engine(tag, dtype)
    m = PARENT_MEASURED.get(("batch", sampler, tag))
    wav = wavs_of(tag)[1].cuda()
    e.reseed(4242)
    undisturbed = e.decode(wav, 6, None).clone()                          # epoch 0 of seed 4242
    e.reseed(4242)
    got = npy(run_group(e, s, sampler, Lw, O_, noise=False, seeds=SEEDS))
    after = e.decode(wav, 6, None)                                        # the group call neither read nor advanced the epoch
    close(dtype, "repeat", rel(after.cpu().numpy(), undisturbed.cpu().numpy()), f"{sampler}: a decode behind the group call against one without it")
    for r, Ltot in enumerate(lens):
        e.reseed(SEEDS[r])
        alone = run_alone(e, s[r], sampler, Lw, O_, noise=False).cpu().numpy()
        close(dtype, "repeat", rel(got[r], alone), f"{sampler} recording {r} ({Ltot}) against reseed({SEEDS[r]:#x}) and the single call", m)
    swapped = npy(run_group(e, s, sampler, Lw, O_, noise=False, seeds=[SEEDS[0], SEEDS[2], SEEDS[1]]))
    close(dtype, "repeat", rel(swapped[0], got[0]), f"{sampler}: recording 0 with the other two seeds swapped", m)
    for r in (1, 2):
        assert rel(swapped[r], got[r]) > 10 * bar(dtype, "repeat", m), r
    with pytest.raises(L.LdcError) as ei:
        run_group(e, s, sampler, Lw, O_, noise=False, seeds=None)
    assert ei.value.code == L.E_INVALID and "seeds NULL" in str(ei.value)


# ------------------------------------------------------------------------------------------------------------ 5., 6. identities
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_a_group_of_one_is_the_single_call(tag, dtype, sampler):
    Lw, O_, _ = G.GROUPS[tag]
    s = G.inputs(tag, N)[:1]
    e = engine(tag, dtype)
    got = npy(run_group(e, s, sampler, Lw, O_))[0]
    # A single-recording call IS the group of one (one plan, one kernel): this compares a code path with itself and guards against the
    # two ever splitting again.  What pins the arithmetic are the tests against the restatements (test_sample_windows_group, tests/test_gpu_windows.py).
    # the same batch, the same sampler, another call: the run-to-run constant of THIS sampler on a batch of this recording's W windows
    # (tests/test_gpu_windows_receiver.py; a DDIM eta 1 chain scatters twice as far run to run as a DDPM one, 8.1e-4 against 4.4e-4 on r8)
    m = TR.PARENT_MEASURED[("rerun_lat", tag, TR.W_OF[tag], sampler)]
    close(dtype, "repeat", rel(got, run_alone(e, s[0], sampler, Lw, O_).cpu().numpy()), f"{tag} {sampler} R = 1 against the single call", m)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_single_call_and_a_group_of_one_alternate_on_their_shared_plan(dtype):
    """The two calls of one (Ltot, Lw, O) share a plan, its recording table and its step graphs.  The single call runs on a tape, the group
    call draws under its seed: a key or a tape left behind by the other call would move the second result of either off its first."""
    tag, sampler = "r84", "ddpm"
    Lw, O_, _ = G.GROUPS[tag]
    s = G.inputs(tag, N)[:1]
    e = engine(tag, dtype)
    m = TR.PARENT_MEASURED[("rerun_lat", tag, TR.W_OF[tag], sampler)]
    single = lambda: run_alone(e, s[0], sampler, Lw, O_).cpu().numpy()                                       # noqa: E731
    group = lambda: npy(run_group(e, s, sampler, Lw, O_, noise=False, seeds=SEEDS[:1]))[0]                    # noqa: E731
    single0, group0, single1, group1 = single(), group(), single(), group()
    close(dtype, "repeat", rel(single1, single0), "the single call on its tape, behind the group call, against its first result", m)
    close(dtype, "repeat", rel(group1, group0), "the group call under its seed, behind the single call, against its first result", m)
    assert rel(group0, single0) > 10 * bar(dtype, "repeat", m)                                                # (the seed's noise is not the tape's)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_one_window_recordings_are_an_ordinary_batch(tag, dtype):
    Lw, O_, _ = G.GROUPS[tag]
    s = G.inputs(tag, N, lens=(Lw, Lw, Lw))
    e = engine(tag, dtype)
    got = np.concatenate(npy(e.sample_windows_group(gpu(s, "img"), gpu(s, "cond"), N, Lw, O_, noise=gpu(s, "noise"))))
    ref = e.denoise(torch.cat(gpu(s, "img")), torch.cat(gpu(s, "cond")), N, torch.cat(gpu(s, "noise"), dim=1).contiguous()).cpu().numpy()
    close(dtype, "repeat", rel(got, ref), f"{tag} three one-window recordings against denoise at B = 3", TW.PARENT_MEASURED[("repeat", tag, 3)])


# ------------------------------------------------------------------------------------------------------------------ 7. graphs
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replays_equal_eager_steps_and_stay_with_their_group(dtype):
    tag, Lw, O_ = "r84", 80, 20                                           # (groups no other test uses: their first use is here)
    A, B = (200, 80, 140), (140, 80, 200)                                 # 3 + 1 + 2 windows either way, the same frames in all
    assert L.window_group_layout(A, Lw, O_, 10)[0][-1] == L.window_group_layout(B, Lw, O_, 10)[0][-1] == 6
    sa, sb = G.inputs(tag, N, lens=A), G.inputs(tag, N, lens=B)
    e = engine(tag, dtype)
    m = TW.PARENT_MEASURED[("repeat", "r84", 4)]
    seeds1, seeds2 = SEEDS, [s + 1 for s in SEEDS]
    grp = lambda s, seeds: [x.clone() for x in run_group(e, s, "ddpm", Lw, O_, noise=False, seeds=seeds)]      # noqa: E731

    def member():                                                         # the single-recording call of one member
        e.reseed(seeds1[0])
        return run_alone(e, sa[0], "ddpm", Lw, O_, noise=False).clone()
    member0 = member()
    e.set_option("serial_parts", 1)
    try:
        eager_a1, eager_a2, eager_b = grp(sa, seeds1), grp(sa, seeds2), grp(sb, seeds1)
    finally:
        e.set_option("serial_parts", 0)
    first, other = grp(sa, seeds1), grp(sb, seeds1)                       # the eager first step, the capture, replays
    torch.cuda.synchronize()
    syncs = L.load().ldc_debug_sync_count()
    replay, reseeded, other2, member1, again = grp(sa, seeds1), grp(sa, seeds2), grp(sb, seeds1), member(), grp(sa, seeds1)
    torch.cuda.synchronize()
    assert L.load().ldc_debug_sync_count() == syncs                       # warm calls: no device-wide synchronisation
    for what, a, b in (("first use", first, eager_a1), ("replay", replay, eager_a1), ("replay with other seeds", reseeded, eager_a2),
                       ("the other group", other, eager_b), ("the other group, replayed", other2, eager_b), ("replay again", again, eager_a1),
                       ("the single call of a member before and after", [member1], [member0]),
                       ("the member in the group against its single call", first[:1], [member0])):
        close(dtype, "repeat", G.rel_group(npy(a), npy(b)), f"graphs: {what}", m)
    assert rel(npy(eager_a1)[0], npy(eager_a2)[0]) > 10 * bar(dtype, "repeat", m)                       # (other seeds, other noise)
    # the middle recording, its inputs and its seed are the same in both groups: it does not care which group it is decoded in
    close(dtype, "repeat", rel(npy(other2)[1], npy(replay)[1]), "graphs: the recording both groups share", m)


# ---------------------------------------------------------------------------------------------------------- 8. the cap, once
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_thirty_two_windows(dtype):
    tag, Lw, O_ = "r84", 80, 40
    lens = (180,) * 8
    s = G.inputs(tag, N, lens=lens)
    e = engine(tag, dtype)
    assert e.window_group_layout(lens, Lw, O_)[0][-1] == 32
    got = npy(e.sample_windows_group(gpu(s, "img"), gpu(s, "cond"), 6, Lw, O_, noise=[i["noise"][:6].cuda() for i in s]))
    for r in range(8):
        alone = e.denoise_windows(s[r]["img"].cuda(), s[r]["cond"].cuda(), 6, Lw, O_, noise=s[r]["noise"][:6].cuda()).cpu().numpy()
        close(dtype, "repeat", rel(got[r], alone), f"32 windows: recording {r} against the single call", PARENT_MEASURED.get(("batch", "ddpm", tag)))
    with pytest.raises(L.LdcError) as ei:
        s9 = s + s[:1]
        e.sample_windows_group(gpu(s9, "img"), gpu(s9, "cond"), 6, Lw, O_, noise=[i["noise"][:6].cuda() for i in s9])
    assert ei.value.code == L.E_INVALID and "36 windows" in str(ei.value)


# ------------------------------------------------------------------------------------------------------------------ 9. decode
@pytest.mark.parametrize("sampler", ["ddpm", "ddim1", "dpm"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", TAGS)
def test_decode_windows_group(tag, dtype, sampler):
    Lw, O_, lens = G.GROUPS[tag]
    s = G.inputs(tag, N)
    e = engine(tag, dtype)
    wavs = [w.cuda() for w in wavs_of(tag)]
    if sampler == "ddpm":
        got = e.decode_windows_group(wavs, N, Lw, O_, noise=gpu(s, "noise"), want_stages=True)
    elif sampler == "dpm":
        got = e.decode_windows_group(wavs, S, Lw, O_, sampler="dpm", t_start=T_START, want_stages=True)
    else:
        got = e.decode_windows_group(wavs, S, Lw, O_, sampler="ddim", t_start=T_START, eta=1.0, noise=[i["noise"][:S].cuda() for i in s], want_stages=True)
    for r, Ltot in enumerate(lens):
        if sampler == "ddpm":
            one = e.decode_windows(wavs[r], N, Lw, O_, noise=s[r]["noise"].cuda(), want_stages=True)
        elif sampler == "dpm":
            one = e.decode_dpm_windows(wavs[r], T_START, S, Lw, O_, want_stages=True)
        else:
            one = e.decode_ddim_windows(wavs[r], T_START, S, Lw, O_, eta=1.0, noise=s[r]["noise"][:S].cuda(), want_stages=True)
        assert torch.equal(got[r]["codes"], one["codes"]), r
        assert torch.equal(got[r]["cond"], one["cond"]), r                                # bit-identical: the same code at B = 1
        close(dtype, "repeat", rel(got[r]["latents"].cpu().numpy(), one["latents"].cpu().numpy()),
              f"{tag} {sampler} decode: latents of recording {r} ({Ltot})", PARENT_MEASURED.get(("batch_lat", sampler, tag)))
        close(dtype, "wav_small", rel(got[r]["wav"].cpu().numpy(), one["wav"].cpu().numpy()),
              f"{tag} {sampler} decode: waveform of recording {r} ({Ltot})", PARENT_MEASURED.get(("batch_wav", sampler, tag)))


# --------------------------------------------------------------------------------------------------------------------- 10. CLI
def test_cli_window_group_writes_what_the_run_without_the_flag_writes(tmp_path, monkeypatch):
    from scipy.io import wavfile
    from ladiffcodec_amd import sample
    from ladiffcodec_amd.model import Engine
    from helpers import cond_sd_np, main_sd_np
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"))
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind = tmp_path / "in"
    ind.mkdir()
    steps, lens = 10, (180, 80, 240)                                      # trimmed to 5760, 2560 and 7680 samples
    for k, Ltot in enumerate(lens):
        x = (synth.synthetic_wav(1, Ltot * 32 + 100, seed=84 + k)[0, 0] * 0.5).astype(np.float32)
        wavfile.write(str(ind / f"long{k}.wav"), 16000, x)
    tapes = [torch.randn(steps, 1, 128, Ltot, generator=torch.Generator().manual_seed(9200 + k)) for k, Ltot in enumerate(lens)]
    calls = {"group": 0, "single": 0}
    for name, key in (("decode_windows_group", "group"), ("decode_windows", "single")):
        def counted(self, *a, _f=getattr(Engine, name), _k=key, **kw):
            calls[_k] += 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(Engine, name, counted)

    def run(out, extra):
        args = sample.build_parser().parse_args([
            "--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff", "--scaling_global",
            "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2", "--diff_dims", "32",
            "--input_dir", str(ind) + "/", "--output_dir", str(tmp_path / out) + "/", "--midway_t", str(steps), "--dtype", "f32",
            "--chunk_sec", "0.16", "--chunk_overlap_sec", "0.08"] + extra)
        asked = []
        args.noise_provider = lambda keys, n_steps, Lz: (asked.append((keys, n_steps, Lz)), tapes[keys[0][0]][:n_steps, :, :, :Lz])[1]
        assert len(sample.synthesis(args)) == 3
        assert sorted(asked) == [([(k, 0)], steps, Ltot) for k, Ltot in enumerate(lens)]                # per recording, as without the flag
        return [wavfile.read(str(tmp_path / out / f"long{k}.wav"))[1] for k in range(3)]
    plain = run("plain", [])
    assert calls == {"group": 0, "single": 3}
    grouped = run("grouped", ["--window_group"])
    assert calls == {"group": 1, "single": 3}                             # 4 + 1 + 5 windows: ONE engine call for the three files
    for k, Ltot in enumerate(lens):
        assert grouped[k].shape == (Ltot * 32,)
        close("f32", "wav_small", rel(grouped[k], plain[k]), f"the CLI's file {k} with --window_group against the run without it")


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_usable():
    tag = "r84"
    Lw, O_, lens = G.GROUPS[tag]
    s = G.inputs(tag, N)
    e = engine(tag, "f32")
    imgs, conds, tapes = gpu(s, "img"), gpu(s, "cond"), gpu(s, "noise")
    good = npy(e.sample_windows_group(imgs, conds, 3, Lw, O_, noise=tapes))
    short = [imgs[0], imgs[1][..., :70].contiguous(), imgs[2]], [conds[0], conds[1][..., :7].contiguous(), conds[2]]
    calls = [
        (lambda: e.sample_windows_group(imgs, conds, 3, Lw, 45, noise=tapes), "overlap 45"),
        (lambda: e.sample_windows_group(imgs, conds, 3, 90, 40, noise=tapes), "Lw 90"),                 # a multiple of up, not of the quantum
        (lambda: e.sample_windows_group(imgs, [conds[0], conds[1][..., :7].contiguous(), conds[2]], 3, Lw, O_, noise=tapes), "recording 1: Ltot (80) must equal Ftot (7)"),
        (lambda: e.sample_windows_group(short[0], short[1], 3, Lw, O_, seeds=SEEDS), "recording 1: Ltot 70"),
        (lambda: e.sample_windows_group(imgs, conds, 0, Lw, O_, noise=tapes), "n_steps 0"),
        (lambda: e.sample_windows_group(imgs, conds, 41, Lw, O_, sampler="ddim", t_start=40, seeds=SEEDS), "n_steps"),
        (lambda: e.sample_windows_group(imgs, conds, 8, Lw, O_, sampler="ddim", t_start=40, eta=1.5, noise=tapes), "eta"),
        (lambda: e.sample_windows_group(imgs, conds, 41, Lw, O_, sampler="dpm", t_start=40), "n_steps 41"),
        (lambda: e.sample_windows_group(imgs, conds, 3, Lw, O_), "seeds NULL"),
        (lambda: e.unet_forward_windows_group(imgs, 1000, conds, Lw, O_), "t 1000"),
        (lambda: e.decode_windows_group([torch.zeros(1, 1, 180 * 32).cuda(), torch.zeros(1, 1, 80 * 32 + 32).cuda()], 3, Lw, O_, seeds=SEEDS[:2]), "recording 1: T 2592"),
    ]
    for call, word in calls:
        with pytest.raises(L.LdcError) as ei:
            call()
        assert ei.value.code == L.E_INVALID and word in str(ei.value), (word, str(ei.value))
        again = npy(e.sample_windows_group(imgs, conds, 3, Lw, O_, noise=tapes))
        assert G.rel_group(again, good) < TOL["f32"]["repeat"], word
    e.sample_windows_group(imgs, conds, 8, Lw, O_, sampler="ddim", t_start=40, eta=0.0)                 # eta 0 draws nothing: neither tape nor seeds
    with pytest.raises(L.LdcError) as ei:
        engine(tag, "fp8").sample_windows_group(imgs, conds, 3, Lw, O_, noise=tapes)
    assert ei.value.code == L.E_INVALID and "fp8 engine" in str(ei.value)
