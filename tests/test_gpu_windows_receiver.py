"""Coupled windows for the receiver on the GPU ("DPM-Solver++ windows and the receiver"): DPM-Solver++(2M) on the
shared latent against the Python restatement on the CPU oracle (tests/windows_dpm_restatement.py) and against the engine's own B = 1 and
independent-chunk calls; the decodes from RVQ codes against the waveform-driven windows decodes; the CLIs.

Shapes (Ltot, Lw, overlap) in latent frames, those of test_gpu_windows.py: `r84` (180, 80, 40) -- four windows, a triple-covered stretch,
Ltot no multiple of the 32-frame tile -- and `r8` (400, 160, 40); (t_start, S) = (40, 8) and (100, 12).  The references are computed
once per process and shared; nothing writes to them.

Bars: tests/drift_tolerances.py; every test prints its figure before it asserts.  f32 keeps the generic bars throughout, and its
`chain_small` bar (1e-5) sees all three mutants of tests/test_windows_receiver_cpu.py (3.0e-4 at the least).  The generic bf16 bars were
recorded on shorter chains; where a bf16 figure exceeds one, the bar is twice what the PARENT's path shows on the same items, two runs
on MI355X, held in PARENT_MEASURED below (DESIGN.md section 5g records both sides).  The bf16 bars cannot see mutants (a)-(c)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from ladiffcodec_amd.bitstream import Bitstream  # noqa: E402
from helpers import cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
import windows_dpm_restatement as WD  # noqa: E402
import windows_restatement as R  # noqa: E402
from test_gpu_windows import decode_setup  # noqa: E402

MAIN = [("r84", 180, 80, 40), ("r8", 400, 160, 40)]
SCHEDULES = [(40, 8), (100, 12)]
N = 40                                                                   # DDPM steps of the decodes (test_gpu_windows.decode_setup)
W_OF = {"r84": 4, "r8": 3}                                               # windows of the two layouts

# bf16 only, worst of two runs on MI355X of the PARENT's path on the same items (see the module docstring); a figure without an entry
# keeps the generic bar.
#   ("dpm", tag, Ltot, t_start, S)   Engine.dpm_sample of the W windows as independent items against dpm_restatement.dpm_sample solo
#   ("dpm_repeat", tag, B)           Engine.dpm_sample (100, 12) run to run: B = 1 and the three chunks of the identity tests; B = W:
#                                    graphs against eager steps on the windows as independent items
#   ("codes_lat" | "codes_wav", tag, Ltot, "ddpm" | "dpm")   Engine.decode_codes (40 steps, the tape) / decode_codes_dpm (40, 8) of the
#                                    windows' stretches of the oracle's codes against the oracle's solo decodes
#   ("rerun_lat" | "rerun_wav", tag, W, "ddpm" | "ddim0" | "ddim1" | "dpm")   the same decodes (DDIM: decode_codes_ddim (40, 8) at eta 0 / 1
#                                    on the tape) run to run, three reruns against the first
PARENT_MEASURED = {
    ("dpm", "r84", 180, 40, 8): 9.65e-4, ("dpm", "r84", 180, 100, 12): 1.90e-3, ("dpm", "r8", 400, 40, 8): 1.27e-3, ("dpm", "r8", 400, 100, 12): 2.37e-3,
    ("dpm_repeat", "r84", 1): 7.87e-4, ("dpm_repeat", "r84", 3): 9.08e-4, ("dpm_repeat", "r84", 4): 1.10e-3,
    ("dpm_repeat", "r8", 1): 1.25e-3, ("dpm_repeat", "r8", 3): 1.11e-3,
    ("codes_lat", "r84", 180, "ddpm"): 1.61e-3, ("codes_lat", "r84", 180, "dpm"): 9.79e-4,
    ("codes_lat", "r8", 400, "ddpm"): 2.12e-3, ("codes_lat", "r8", 400, "dpm"): 1.10e-3,
    ("codes_wav", "r84", 180, "ddpm"): 2.61e-4, ("codes_wav", "r84", 180, "dpm"): 2.02e-4,
    ("codes_wav", "r8", 400, "ddpm"): 1.15e-3, ("codes_wav", "r8", 400, "dpm"): 7.53e-4,
    ("rerun_lat", "r84", 4, "ddpm"): 5.24e-4, ("rerun_lat", "r84", 4, "ddim0"): 5.04e-4, ("rerun_lat", "r84", 4, "ddim1"): 6.96e-4,
    ("rerun_lat", "r84", 4, "dpm"): 4.54e-4, ("rerun_lat", "r8", 3, "ddpm"): 4.42e-4, ("rerun_lat", "r8", 3, "ddim0"): 6.01e-4,
    ("rerun_lat", "r8", 3, "ddim1"): 8.08e-4, ("rerun_lat", "r8", 3, "dpm"): 6.73e-4,
    ("rerun_wav", "r84", 4, "ddpm"): 8.95e-5, ("rerun_wav", "r84", 4, "ddim0"): 9.07e-5, ("rerun_wav", "r84", 4, "ddim1"): 1.08e-4,
    ("rerun_wav", "r84", 4, "dpm"): 1.02e-4, ("rerun_wav", "r8", 3, "ddpm"): 2.02e-4, ("rerun_wav", "r8", 3, "ddim0"): 3.56e-4,
    ("rerun_wav", "r8", 3, "ddim1"): 4.08e-4, ("rerun_wav", "r8", 3, "dpm"): 3.08e-4,
}
_REF = {}


def bar(dtype, key, measured=None):
    m = PARENT_MEASURED.get(measured) if dtype == "bf16" else None
    return max(TOL[dtype][key], 2.0 * m) if m else TOL[dtype][key]


def close(dtype, key, value, what, measured=None):
    b = bar(dtype, key, measured)
    print(f"receiver windows {dtype} {what}: {value:.3e} ({key} bar {b:.3e})")
    assert value < b, (dtype, key, what, value, b)


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def npy(x):
    return x.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the loop against the restatement
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("t_start,S", SCHEDULES)
@pytest.mark.parametrize("tag,Ltot,Lw,O_", MAIN)
def test_dpm_sample_windows_against_the_restatement(tag, Ltot, Lw, O_, t_start, S, dtype):
    s = R.inputs(tag, Ltot)
    ref = WD.reference(tag, Ltot, Lw, O_, t_start, S).numpy()
    got = npy(engine(tag, dtype).dpm_sample_windows(s["img"].cuda(), s["cond"].cuda(), t_start, S, Lw, O_))
    assert np.isfinite(got).all()
    err = rel(got, ref)
    key = ("dpm", tag, Ltot, t_start, S)
    close(dtype, "chain_small", err, f"{tag} {(Ltot, Lw, O_)} DPM ({t_start}, {S})", key)
    # the mutants: by the triangle inequality the GPU result is as far from each as the oracle's coupled result is, give or take `err`;
    # the f32 bar sees every one of them (the CPU test asserts >= 10 x the bar on the oracle alone), the bf16 bar need not
    m = np.abs(ref).max()
    mutants = (("(a) blended once at the end", WD.reference(tag, Ltot, Lw, O_, t_start, S, mode="end")[0]),
               ("(b) first order", WD.reference(tag, Ltot, Lw, O_, t_start, S, mode="first")),
               ("(c) DDIM windows at eta 0", WD.reference(tag, Ltot, Lw, O_, t_start, S, mode="ddim")))
    for what, other in mutants:
        d_gpu, d_cpu = np.abs(got - other.numpy()).max() / m, np.abs(ref - other.numpy()).max() / m
        print(f"receiver windows {dtype} {tag} ({t_start}, {S}) against the mutant {what}: {d_gpu:.3e} (the oracle's: {d_cpu:.3e})")
        assert abs(d_gpu - d_cpu) < bar(dtype, "chain_small", key), (what, d_gpu, d_cpu)
        if dtype == "f32":
            assert d_gpu > bar(dtype, "chain_small"), (what, d_gpu)


# ------------------------------------------------------------------------------------------------------------ 2. history hygiene
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_history_never_leaks_between_calls(dtype):
    tag, Ltot, Lw, O_ = MAIN[0]
    e = engine(tag, dtype)
    a, b, c = R.inputs(tag, Ltot), R.inputs(tag, Ltot, seed=35), R.inputs(tag, 200)
    ia, ca, ib, cb, ic, cc = (x.cuda() for x in (a["img"], a["cond"], b["img"], b["cond"], c["img"], c["cond"]))
    e.dpm_sample_windows(ia, ca, 100, 12, Lw, O_)                          # leaves its x0 in the plan's history
    one = e.dpm_sample_windows(ib, cb, 60, 1, Lw, O_).clone()              # the only iteration is the last: the clipped x0
    ref = e.ddim_sample_windows(ib, cb, 60, 1, Lw, O_, eta=0.0)
    assert float(one.abs().max()) <= 1.0
    close(dtype, "repeat", rel(npy(one), npy(ref)), "DPM S = 1 after a 12-step call on other inputs against DDIM S = 1, eta 0",
          ("dpm_repeat", tag, W_OF[tag]))
    first = e.dpm_sample_windows(ia, ca, 40, 8, Lw, O_).clone()
    e.dpm_sample_windows(ic, cc, 100, 12, 80, 20)                          # another layout's call in between
    e.dpm_sample_windows(ib, cb, 100, 12, Lw, O_)                          # and another recording's on this layout
    second = e.dpm_sample_windows(ia, ca, 40, 8, Lw, O_)
    close(dtype, "repeat", rel(npy(second), npy(first)), "8 steps, twice with other calls in between", ("dpm_repeat", tag, W_OF[tag]))


# ------------------------------------------------------------------------------------------------------------------ 3. graphs
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replays_equal_eager_steps_and_stay_with_their_kind(dtype):
    tag, Ltot, Lw, O_ = "r84", 260, 80, 20                                # (a layout no other test uses: its first use is here)
    t_start, S = 100, 12                                                  # the eager first step, two 5-step graphs, one single step
    s, s2 = R.inputs(tag, Ltot), R.inputs(tag, 180)
    e = engine(tag, dtype)
    img, cond, img2, cond2 = s["img"].cuda(), s["cond"].cuda(), s2["img"].cuda(), s2["cond"].cuda()
    W = len(R.layout(Ltot, Lw, O_)[0])
    assert W == W_OF[tag]
    # an ordinary dpm_sample of the windows' shape (W, Lw), before and after
    starts = R.layout(Ltot, Lw, O_)[0]
    ximg = torch.cat([img[..., a:a + Lw] for a in starts]).contiguous()
    xcond = torch.cat([cond[..., a // s["up"]:(a + Lw) // s["up"]] for a in starts]).contiguous()
    plain0 = e.dpm_sample(xcond, t_start, S, ximg).clone()
    e.set_option("serial_parts", 1)
    try:
        eager = e.dpm_sample_windows(img, cond, t_start, S, Lw, O_).clone()
        eager_ddim = e.ddim_sample_windows(img, cond, t_start, S, Lw, O_, eta=0.0).clone()
    finally:
        e.set_option("serial_parts", 0)
    first = e.dpm_sample_windows(img, cond, t_start, S, Lw, O_).clone()   # the eager first step, the capture, replays
    ddim = e.ddim_sample_windows(img, cond, t_start, S, Lw, O_, eta=0.0).clone()   # the same layout and step count, DDIM's own graphs
    e.ddim_sample_windows(img2, cond2, 40, 8, 80, 40, eta=0.0)
    torch.cuda.synchronize()
    syncs = L.load().ldc_debug_sync_count()
    replay = e.dpm_sample_windows(img, cond, t_start, S, Lw, O_).clone()
    ddim2 = e.ddim_sample_windows(img, cond, t_start, S, Lw, O_, eta=0.0).clone()
    e.ddim_sample_windows(img2, cond2, 40, 8, 80, 40, eta=0.0)
    plain1 = e.dpm_sample(xcond, t_start, S, ximg).clone()
    again = e.dpm_sample_windows(img, cond, t_start, S, Lw, O_).clone()
    torch.cuda.synchronize()
    assert L.load().ldc_debug_sync_count() == syncs                       # warm calls: no device-wide synchronisation
    for what, a, b in (("first use", first, eager), ("replay", replay, eager), ("replay again", again, eager),
                       ("DDIM windows in between", ddim, eager_ddim), ("DDIM windows in between, replayed", ddim2, eager_ddim),
                       ("an ordinary dpm_sample of (W, Lw) before and after", plain1, plain0)):
        close(dtype, "repeat", rel(npy(a), npy(b)), f"graphs: {what}", ("dpm_repeat", tag, W))
    # two samplers, two results: further apart than "equal" is (the oracle has them 2.8e-3 ... 4.7e-3 apart at (100, 12))
    assert rel(npy(eager), npy(eager_ddim)) > bar(dtype, "repeat", ("dpm_repeat", tag, W))


# ------------------------------------------------------------------------------------------------------- 4. identities and epoch
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Lw", [("r84", 80), ("r8", 160)])
def test_one_window_is_dpm_sample_at_batch_one(tag, Lw, dtype):
    s = R.inputs(tag, Lw)
    e = engine(tag, dtype)
    img, cond = s["img"].cuda(), s["cond"].cuda()
    ref = npy(e.dpm_sample(cond, 100, 12, img))
    for lw in (Lw, 2 * Lw):                                               # Ltot == Lw and Ltot < Lw: one window of Ltot frames
        got = npy(e.dpm_sample_windows(img, cond, 100, 12, lw, 40))
        close(dtype, "repeat", rel(got, ref), f"{tag} W = 1 (Lw {lw}) against dpm_sample at B = 1", ("dpm_repeat", tag, 1))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Lw", [("r84", 80), ("r8", 160)])
def test_overlap_zero_is_the_batch_of_independent_chunks(tag, Lw, dtype):
    s = R.inputs(tag, 3 * Lw)
    e = engine(tag, dtype)
    cut = lambda x, n: torch.cat([x[..., k * n:(k + 1) * n] for k in range(3)], dim=-3).contiguous()      # noqa: E731
    ref = e.dpm_sample(cut(s["cond"], Lw // s["up"]).cuda(), 100, 12, cut(s["img"], Lw).cuda()).cpu()
    ref = torch.cat(list(ref[:, None]), dim=-1).numpy()
    got = npy(e.dpm_sample_windows(s["img"].cuda(), s["cond"].cuda(), 100, 12, Lw, 0))
    close(dtype, "repeat", rel(got, ref), f"{tag} overlap 0 against dpm_sample of the three chunks at B = 3", ("dpm_repeat", tag, 3))


def test_dpm_windows_leave_the_noise_epoch_alone():
    """reseed; decode == reseed; DPM windows calls; decode, with device-drawn (Philox) noise: they draw nothing and move no epoch."""
    tag, Ltot, Lw, O_ = MAIN[0]
    d = decode_setup(tag, Ltot, Lw, O_)
    s = R.inputs(tag, Ltot)
    e = engine(tag, "f32")
    wav = (torch.from_numpy(synth.synthetic_wav(1, 5120, seed=36)) * 0.5).cuda()
    e.reseed(5)
    plain = e.decode(wav, 8, per_item=True, want_stages=True)["latents"].clone()
    e.reseed(5)
    e.decode_dpm_windows(d["wav"].cuda(), 40, 8, Lw, O_)
    e.dpm_sample_windows(s["img"].cuda(), s["cond"].cuda(), 40, 8, Lw, O_)
    e.decode_codes_dpm_windows(codes=d["codes"].cuda(), t_start=40, n_steps=8, Lw=Lw, overlap=O_)
    after = e.decode(wav, 8, per_item=True, want_stages=True)["latents"].clone()
    close("f32", "repeat", rel(npy(after), npy(plain)), "decode after DPM windows calls against decode alone")


# ------------------------------------------------------------------------------------------------------- 5. decode from codes
def _codes_calls(e, codes, packed, **kw):
    n_q, _, F = codes.shape
    a = e.decode_codes_windows(codes=codes, want_stages=True, **kw)
    a = {k: v.clone() for k, v in a.items()}
    b = e.decode_codes_windows(packed=packed, n_q=n_q, F=F, want_stages=True, **kw)
    return a, {k: v.clone() for k, v in b.items()}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", MAIN)
def test_decode_codes_windows_is_decode_windows(tag, Ltot, Lw, O_, dtype):
    d = decode_setup(tag, Ltot, Lw, O_)
    e = engine(tag, dtype)
    wav, noise = d["wav"].cuda(), d["noise"].cuda()
    refs = {"ddpm": e.decode_windows(wav, N, Lw, O_, noise=noise, want_stages=True)}
    refs["ddpm"] = {k: v.clone() for k, v in refs["ddpm"].items()}
    codes = refs["ddpm"]["codes"]
    packed = Bitstream(e).pack_codes(codes, 10)
    assert codes.shape[1:] == (1, Ltot // R.inputs(tag, Ltot)["up"]) and packed.shape[0] == 1
    runs = [("ddpm", "ddpm", dict(n_steps=N, Lw=Lw, overlap=O_, noise=noise))]
    for eta in (0.0, 1.0):
        r = e.decode_ddim_windows(wav, 40, 8, Lw, O_, eta=eta, noise=noise[:8], want_stages=True)
        refs[f"ddim eta {eta}"] = {k: v.clone() for k, v in r.items()}
        runs.append((f"ddim eta {eta}", f"ddim{int(eta)}", dict(n_steps=8, Lw=Lw, overlap=O_, t_start=40, eta=eta, noise=noise[:8])))
    for what, kind, kw in runs:
        ref = refs[what]
        assert torch.equal(ref["codes"], codes)
        a, b = _codes_calls(e, codes, packed, **kw)
        assert torch.equal(a["cond"], ref["cond"]), what                  # bit-identical: the dequantised rows are get_cond's
        assert torch.equal(b["cond"], a["cond"]), what                    # packed and int64 sources
        for src, got in (("int64", a), ("packed", b)):
            close(dtype, "repeat", rel(npy(got["latents"]), npy(ref["latents"])), f"{tag} {what} from {src} codes: latents",
                  ("rerun_lat", tag, W_OF[tag], kind))
            close(dtype, "repeat", rel(npy(got["wav"]), npy(ref["wav"])), f"{tag} {what} from {src} codes: waveform",
                  ("rerun_wav", tag, W_OF[tag], kind))
    # against the restatement's decode: the oracle's codes (the engine's agree with them wherever the quantiser's margin is safe)
    safe = np.logical_and.accumulate(d["margins"].numpy() > 1e-3, axis=0)
    assert np.array_equal(npy(codes)[safe], d["codes"].numpy()[safe])
    got = e.decode_codes_windows(codes=d["codes"].cuda(), n_steps=N, Lw=Lw, overlap=O_, noise=noise, want_stages=True)
    close(dtype, "chain_small", rel(npy(got["latents"]), d["latents"].numpy()), f"{tag} from the oracle's codes: latents against the restatement",
          ("codes_lat", tag, Ltot, "ddpm"))
    close(dtype, "wav_small", rel(npy(got["wav"]), d["out"].numpy()), f"{tag} from the oracle's codes: waveform against the restatement",
          ("codes_wav", tag, Ltot, "ddpm"))


def dpm_decode_setup(tag, Ltot, Lw, O_, t_start, S):
    def make():
        d = decode_setup(tag, Ltot, Lw, O_)
        s = R.inputs(tag, Ltot)
        sdc = synth.to_torch(cond_sd_np())
        from helpers import COND_CFG
        return WD.decode_dpm_windows(sdc, COND_CFG, s["sd"], d["mc"], s["u"], d["wav"], t_start, S, Lw, O_)
    return cached(("dpm decode", tag, Ltot, Lw, O_, t_start, S), make)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag,Ltot,Lw,O_", MAIN)
def test_decode_dpm_windows_its_staged_calls_and_its_codes(tag, Ltot, Lw, O_, dtype):
    t_start, S = 40, 8
    d = decode_setup(tag, Ltot, Lw, O_)
    o = dpm_decode_setup(tag, Ltot, Lw, O_, t_start, S)
    e = engine(tag, dtype)
    wav = d["wav"].cuda()
    rep, rep_wav = ("rerun_lat", tag, W_OF[tag], "dpm"), ("rerun_wav", tag, W_OF[tag], "dpm")
    got = e.decode_dpm_windows(wav, t_start, S, Lw, O_, want_stages=True)
    got = {k: v.clone() for k, v in got.items()}
    # the staged calls: get_cond and the normalised start image over the whole recording, the coupled loop, decoder, normalisation
    cond, codes = e.get_cond(wav, return_codes=True)
    lat = e.dpm_sample_windows(e.cond_upsample(cond, 1), cond, t_start, S, Lw, O_)
    staged = e.output_normalise(e.decode_latents(L.MODEL_MAIN, lat))
    assert torch.equal(got["codes"], codes)
    close(dtype, "repeat", rel(npy(got["cond"]), npy(cond)), f"{tag} decode_dpm: cond against get_cond")
    close(dtype, "repeat", rel(npy(got["latents"]), npy(lat)), f"{tag} decode_dpm: latents against the staged calls", rep)
    close(dtype, "repeat", rel(npy(got["wav"]), npy(staged)), f"{tag} decode_dpm: waveform against the staged calls", rep_wav)
    # from codes: int64 and packed
    n_q, _, F = codes.shape
    for src, kw in (("int64", dict(codes=codes)), ("packed", dict(packed=Bitstream(e).pack_codes(codes, 10), n_q=n_q, F=F))):
        c = e.decode_codes_dpm_windows(t_start=t_start, n_steps=S, Lw=Lw, overlap=O_, want_stages=True, **kw)
        assert torch.equal(c["cond"], got["cond"]), src
        close(dtype, "repeat", rel(npy(c["latents"]), npy(got["latents"])), f"{tag} decode_codes_dpm from {src} codes: latents", rep)
        close(dtype, "repeat", rel(npy(c["wav"]), npy(got["wav"])), f"{tag} decode_codes_dpm from {src} codes: waveform", rep_wav)
    # against the restatement's decode, from the oracle's codes
    c = e.decode_codes_dpm_windows(codes=o["codes"].cuda(), t_start=t_start, n_steps=S, Lw=Lw, overlap=O_, want_stages=True)
    close(dtype, "chain_small", rel(npy(c["latents"]), o["latents"].numpy()), f"{tag} DPM from the oracle's codes: latents against the restatement",
          ("codes_lat", tag, Ltot, "dpm"))
    close(dtype, "wav_small", rel(npy(c["wav"]), o["out"].numpy()), f"{tag} DPM from the oracle's codes: waveform against the restatement",
          ("codes_wav", tag, Ltot, "dpm"))


# --------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_engine_usable():
    tag, Ltot, Lw, O_ = MAIN[0]
    s = R.inputs(tag, Ltot)
    d = decode_setup(tag, Ltot, Lw, O_)
    e = engine(tag, "f32")
    lib = L.load()
    img, cond, noise = s["img"].cuda(), s["cond"].cuda(), d["noise"].cuda()
    codes = d["codes"].cuda()
    n_q, _, F = codes.shape
    packed = Bitstream(e).pack_codes(codes, 10)
    bad = codes.clone()
    bad[1, 0, 7] = 1024                                                    # a code >= bins
    many = torch.zeros(n_q, 1, (80 + 32 * 40) // 10, dtype=torch.int64).cuda()
    out = torch.empty(1, 1, F * 320).cuda()
    good = e.dpm_sample_windows(img, cond, 40, 3, Lw, O_).clone()
    good_codes = e.decode_codes_windows(codes=codes, n_steps=3, Lw=Lw, overlap=O_, noise=noise[:3], want_stages=True)
    good_codes = {k: v.clone() for k, v in good_codes.items()}

    def raw(c, p):   # both / neither source straight at the library (the Engine refuses them itself, with a ValueError)
        def call():
            L.check(lib.ldc_decode_codes_windows(e._ctx, c, p, packed.stride(0), 10, n_q, F, 0, 3, 0.0, None, Lw, O_, out.data_ptr(), None, None, None))
        return call

    def flagged(fn):   # a bad code VALUE is found on the device: the call, or the next call on the context, reports it
        def call():
            fn()
            torch.cuda.synchronize()
            e.rvq_decode(codes)
        return call

    calls = [
        (lambda: e.dpm_sample_windows(img, cond, 40, 3, Lw, 45), "overlap 45"),
        (lambda: e.dpm_sample_windows(img, cond, 40, 3, 90, 40), "Lw 90"),                          # a multiple of up, not of the quantum
        (lambda: e.dpm_sample_windows(img, cond, 40, 41, Lw, O_), "n_steps 41"),
        (lambda: e.dpm_sample_windows(img, cond, 0, 1, Lw, O_), "t_start 0"),
        (lambda: e.dpm_sample_windows(img, cond, 100000, 8, Lw, O_), "t_start 100000"),
        (lambda: e.decode_dpm_windows(d["wav"].cuda(), 40, 41, Lw, O_), "n_steps 41"),
        (lambda: e.decode_dpm_windows(d["wav"].cuda(), 40, 8, Lw, 45), "overlap 45"),
        (lambda: e.decode_codes_windows(codes=codes, n_steps=3, Lw=Lw, overlap=45), "overlap 45"),
        (lambda: e.decode_codes_windows(codes=codes, n_steps=3, Lw=90, overlap=40), "Lw 90"),
        (lambda: e.decode_codes_windows(codes=codes, n_steps=41, Lw=Lw, overlap=O_, t_start=40), "n_steps 41"),
        (lambda: e.decode_codes_windows(codes=codes, n_steps=8, Lw=Lw, overlap=O_, t_start=40, eta=1.5), "eta 1.5"),
        (lambda: e.decode_codes_dpm_windows(codes=codes, t_start=40, n_steps=41, Lw=Lw, overlap=O_), "n_steps 41"),
        (lambda: e.decode_codes_dpm_windows(codes=codes, t_start=40, n_steps=8, Lw=Lw, overlap=45), "overlap 45"),
        (lambda: e.decode_codes_windows(codes=many, n_steps=3, Lw=80, overlap=40), "33 windows"),
        (lambda: e.decode_codes_dpm_windows(codes=many, t_start=40, n_steps=8, Lw=80, overlap=40), "33 windows"),
        (raw(codes.data_ptr(), packed.data_ptr()), "exactly one of codes / packed"),
        (raw(None, None), "exactly one of codes / packed"),
        (flagged(lambda: e.decode_codes_windows(codes=bad, n_steps=3, Lw=Lw, overlap=O_, noise=noise[:3])), "[bad_code]"),
        (flagged(lambda: e.decode_codes_dpm_windows(codes=bad, t_start=40, n_steps=3, Lw=Lw, overlap=O_)), "[bad_code]"),
    ]
    for call, word in calls:
        with pytest.raises(L.LdcError) as ei:
            call()
        assert ei.value.code == L.E_INVALID and word in str(ei.value), (word, str(ei.value))
        again = e.dpm_sample_windows(img, cond, 40, 3, Lw, O_)
        assert rel(npy(again), npy(good)) < TOL["f32"]["repeat"], word
        again = e.decode_codes_windows(codes=codes, n_steps=3, Lw=Lw, overlap=O_, noise=noise[:3], want_stages=True)
        assert torch.equal(again["cond"], good_codes["cond"]), word
        assert rel(npy(again["latents"]), npy(good_codes["latents"])) < TOL["f32"]["repeat"], word
        assert rel(npy(again["wav"]), npy(good_codes["wav"])) < TOL["f32"]["wav_small"], word
    for kw in (dict(codes=codes, packed=packed), dict()):
        with pytest.raises(ValueError, match="exactly one of codes / packed"):
            e.decode_codes_windows(n_steps=3, Lw=Lw, overlap=O_, **kw)
        with pytest.raises(ValueError, match="exactly one of codes / packed"):
            e.decode_codes_dpm_windows(t_start=40, n_steps=3, Lw=Lw, overlap=O_, **kw)
    with pytest.raises(ValueError):
        e.dpm_sample_windows(torch.cat([img, img]), torch.cat([cond, cond]), 40, 3, Lw, O_)        # one recording per call
    with pytest.raises(ValueError):
        e.decode_codes_windows(codes=torch.cat([codes, codes], dim=1), n_steps=3, Lw=Lw, overlap=O_)
    f8 = engine(tag, "fp8")
    for call in (lambda: f8.dpm_sample_windows(img, cond, 40, 3, Lw, O_), lambda: f8.decode_dpm_windows(d["wav"].cuda(), 40, 3, Lw, O_),
                 lambda: f8.decode_codes_windows(codes=codes, n_steps=3, Lw=Lw, overlap=O_),
                 lambda: f8.decode_codes_dpm_windows(codes=codes, t_start=40, n_steps=3, Lw=Lw, overlap=O_)):
        with pytest.raises(L.LdcError) as ei:
            call()
        assert ei.value.code == L.E_INVALID and "fp8 engine" in str(ei.value)


# --------------------------------------------------------------------------------------------------------------------- 7. CLIs
def _flags(tmp_path, ind, outd, *extra):
    return ["--model_for_cond", str(tmp_path / "codec.amlt"), "--model_path", str(tmp_path / "ladiff.amlt"), "--run_diff", "--scaling_global",
            "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2", "--diff_dims", "32",
            "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", str(N), "--dtype", "f32",
            "--chunk_sec", "0.16", "--chunk_overlap_sec", "0.08", *extra]


def test_clis_write_what_the_engine_gives(tmp_path, capfd):
    from scipy.io import wavfile
    from ladiffcodec_amd import compress, decompress, sample_dpm
    synth.save_amlt(main_sd_np("r84"), str(tmp_path / "ladiff.amlt"))
    synth.save_amlt(cond_sd_np(), str(tmp_path / "codec.amlt"))
    ind, enc = tmp_path / "in", tmp_path / "enc"
    ind.mkdir()
    n = 180 * 32 + 100                                                    # 5860 samples, trimmed to 5760: 180 latent frames
    x = (synth.synthetic_wav(1, n, seed=84)[0, 0] * 0.5).astype(np.float32)
    wavfile.write(str(ind / "long.wav"), 16000, x)
    assert len(compress.main(_flags(tmp_path, ind, enc)[:-4])) == 1
    e = engine("r84", "f32")
    codes, _ = Bitstream(e).decompress_codes([(enc / "long.ecdc").read_bytes()])
    assert codes.shape[1:] == (1, 18)
    tape = torch.randn(N, 1, 128, 180, generator=torch.Generator().manual_seed(9200))
    read = lambda p: wavfile.read(str(p))[1]                              # noqa: E731

    # decompress, the default sampler: DDPM halfway sampling of --midway_t steps, on the provider's tape
    asked = []
    a = decompress.build_parser().parse_args(_flags(tmp_path, enc, tmp_path / "out_ddpm"))
    a.noise_provider = lambda keys, n_steps, Lz: (asked.append((keys, n_steps, Lz)), tape[:n_steps, :, :, :Lz])[1]
    assert len(decompress.decompress(a)) == 1
    assert asked == [([(0, 0)], N, 180)]                                  # one call, the whole recording: no independent chunks
    y = read(tmp_path / "out_ddpm" / "long.wav")
    ref = e.decode_codes_windows(codes=codes.cuda(), n_steps=N, Lw=80, overlap=40, noise=tape.cuda())
    assert y.shape == (5760,)
    close("f32", "wav_small", rel(y, npy(ref)[0, 0]), "decompress against Engine.decode_codes_windows")
    # decompress --dpm_steps 8 (a provider must not be asked: nothing is drawn)
    a = decompress.build_parser().parse_args(_flags(tmp_path, enc, tmp_path / "out_dpm", "--dpm_steps", "8"))
    a.noise_provider = lambda *k: pytest.fail("a DPM decode asked for noise")
    assert len(decompress.decompress(a)) == 1
    y = read(tmp_path / "out_dpm" / "long.wav")
    ref = e.decode_codes_dpm_windows(codes=codes.cuda(), t_start=N, n_steps=8, Lw=80, overlap=40)
    close("f32", "wav_small", rel(y, npy(ref)[0, 0]), "decompress --dpm_steps against Engine.decode_codes_dpm_windows")
    # sample_dpm with the same flags, from the waveform
    assert len(sample_dpm.main(_flags(tmp_path, ind, tmp_path / "out_wav", "--dpm_steps", "8"))) == 1
    y = read(tmp_path / "out_wav" / "long.wav")
    ref = e.decode_dpm_windows(torch.from_numpy(x[None, None, :5760]).cuda(), N, 8, 80, 40)
    close("f32", "wav_small", rel(y, npy(ref)[0, 0]), "sample_dpm against Engine.decode_dpm_windows")
    assert "hard-joined" not in capfd.readouterr().err                    # four windows: one segment
