"""Item seeds on the GPU ("Item seeds"): `Engine.sample_seeded`, `decode_seeded`, `decode_codes_seeded` and the CLIs'
`--item_seeds`.  Item b of a seeded call draws under key seeds[b] at the block index of the item alone, g = c_first * len_b + l.

Shapes are those of tests/test_gpu_noise.py: engine `r84` (dim 32), B = 3 (parts of 1 and 2 items), C = 128, L in (160, 80), ragged Lmax 320
with quanta (2, 4, 1) and Lmax 240 = 7.5 tiles with (1, 3, 2), N = 6 steps, DDIM (t_start 40, eta 1).  One of the three seeds has a
non-zero high word.

The reference of a seeded call is never the new draws: it is the SAME entry's existing explicit-tape path (`denoise`, `ddim_sample`,
`decode`, `decode_ddim`, `decode_ragged`, `decode_codes*`) fed the tape `assembled_tape` (tests/test_item_seeds_cpu.py) builds from the exact
oracle: `philox_oracle.tape_item(s_b, N, C, len_b)` per item, zero behind its length.  Bars: `chain_small` for latents, test_gpu_noise's
WAV_BAR for waveforms; "equal" is `repeat` (bf16 on the ragged plan: twice test_gpu_dpm.py's RAGGED_DDIM_BF16_REPEAT, and for the latents
of test 3, which runs DDIM at eta 1, twice the same derivation on this file's items: RAGGED_DDIM_ETA1_BF16_REPEAT).
bf16 runs the DDPM cases only where the bar is `chain_small`, as tests/test_gpu_noise.py does: two runs of ONE bf16 ragged DDIM decode
already differ by up to 6.84e-4 (tests/test_gpu_dpm.py), more than the 6.4e-4 bar.

"As if alone" in bf16 (test 2) has a bar of its own.  The batch plans and the B = 1 plan of an item round differently in bf16 (a ragged
batch takes the unfused launch forms), whatever the noise: measured on the PARENT commit with explicit tapes -- the batch of three on the
assembled tape against every item solo on its own tape, the cases of ALONE_CASES, two runs on MI355X -- see ALONE_BF16_MEASURED; the
test asserts against twice the worst, the rule of POOL_DDIM_MEASURED and RAGGED_B1_DDIM_LATENTS.  `measure_alone` is that measurement.

Every comparison prints its figure before it asserts.

RECORDED on MI355X (two runs).  (1) seeded against the assembled tape, f32: latents 1.2e-7 ... 3.0e-7, waveforms 5.4e-7 ... 1.0e-6 (bars
1e-5); bf16 (DDPM): latents up to 2.7e-4 (bar 6.4e-4), waveforms up to 5.8e-5 (bar 1.62e-3).  (2) as if alone, f32: latents 1.2e-7 ...
3.0e-7, waveforms 6.6e-7 ... 1.0e-6; bf16: latents up to 1.11e-3 (ragged 320, DDIM eta 1; bar 1.99e-3), waveforms up to 2.2e-4.  (3) f32
1.2e-7 ... 3.0e-7 / 5.4e-7 ... 9.5e-7; bf16 ragged DDIM eta 1 latents 5.0e-4 ... 1.06e-3 (bar 2.03e-3; the parent's tape path: 1.014e-3),
waveforms 9.9e-5 ... 1.8e-4 (bar 1.37e-3).  (4), (5), (7): 1.2e-7 ... 3.0e-7 / 5.4e-7 ... 1.07e-6 under `repeat` 1e-5.  (6) the two layouts are
7.8e-2 ... 3.9e-1 apart (100 bars: 1e-3), the seeded run 1.8e-7 ... 2.4e-7 from the own-tape run.  (9) every file 6e-7 ... 9e-7 from its
--batch_size 1 run (bar 1e-5).  Wall time: 11 s for the 56 tests, the slowest 0.9 s (the CLI fixture: compress and two reference runs)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, sample, synth  # noqa: E402
from helpers import CASES, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
from oracle import philox_oracle as P  # noqa: E402
from test_gpu_noise import B, C, RAGGED, WAV_BAR, cu, inputs, start_image  # noqa: E402
from test_gpu_dpm import RAGGED_DDIM_BF16_REPEAT  # noqa: E402
from test_item_seeds_cpu import assembled_tape  # noqa: E402

N = 6
T_START, ETA = 40, 1.0
SEEDS = [0x2F6E2B1, 0xC0FFEE12_9E3779B1, 5]                     # the second has a non-zero high word
OTHER = [0x9E3779B9_00000001, 17, 0x1234_5678_9ABC_DEF0]
HOP, CHOP = 32, 320                                             # samples per latent / condition frame (`r84`, the cond codec)
# (kind, size, ddim): the comparisons of test 2 and of measure_alone
ALONE_CASES = [("sample", 160, False), ("sample", 80, True), ("decode", 80, False), ("ragged", 240, False), ("ragged", 320, True),
               ("codes_ragged", 240, False)]
# bf16, item b of the batch of three against the item solo, explicit tapes, parent commit, MI355X: worst of two runs over ALONE_CASES
ALONE_BF16_MEASURED = {"latents": 9.93e-4, "wav": 1.88e-4}     # runs: 9.80e-4 / 9.93e-4 (ragged 320 ddim eta 1) and 1.69e-4 / 1.88e-4
# bf16, ragged 240, DDIM eta 1: an item of the batch of three against the same item in another arrangement (permuted, at B = 2, split 1)
# on the explicit-tape path of the parent commit, MI355X, three runs: latents 8.96e-4 / 9.52e-4 / 1.014e-3, waveforms 1.91e-4 / 2.42e-4 /
# 2.02e-4 (f32: 3.0e-7 / 8.9e-7).  test_gpu_dpm.py's RAGGED_DDIM_BF16_REPEAT (6.84e-4) is the same derivation on eta 0 and on that file's
# items; the noise of eta 1 carries the drift further, so the latents here are held to twice THEIR parent figure.
RAGGED_DDIM_ETA1_BF16_REPEAT = 1.014e-3
_CACHE = {}


# ------------------------------------------------------------------------------------------------------------------------ bars
def bar_of(dtype, key, ragged=False):
    if key == "repeat_lat":                                         # latents of the arrangements of test 3
        if dtype == "bf16" and ragged:
            return max(TOL["bf16"]["repeat"], 2.0 * RAGGED_DDIM_BF16_REPEAT, 2.0 * RAGGED_DDIM_ETA1_BF16_REPEAT)
        key = "repeat"
    if key == "repeat" and dtype == "bf16" and ragged:
        return max(TOL["bf16"]["repeat"], 2.0 * RAGGED_DDIM_BF16_REPEAT)
    if key == "wav":
        return WAV_BAR[dtype]
    if key == "alone":
        return TOL["f32"]["chain_small"] if dtype == "f32" else 2.0 * ALONE_BF16_MEASURED["latents"]
    if key == "alone_wav":
        return WAV_BAR["f32"] if dtype == "f32" else max(WAV_BAR["bf16"], 2.0 * ALONE_BF16_MEASURED["wav"])
    return TOL[dtype][key]


def close(dtype, key, value, what, ragged=False):
    bar = bar_of(dtype, key, ragged)
    print(f"item seeds {dtype} {what}: {value:.3e} ({key} bar {bar:.3e})")
    assert value < bar, (dtype, key, what, value, bar)


def npy(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------- inputs
def is_ragged(kind):
    return kind in ("ragged", "codes_ragged")


def lat_lens(kind, size):
    """latent frames of the three items: `size` is L of a rectangular case, Lmax of a ragged one"""
    return [k * 80 for k in RAGGED[size]] if is_ragged(kind) else [size] * B


def source(e, kind, size):
    """the inputs of a case for all three items (made once: the codec ends are fp32 on every engine)"""
    key = (kind, size)
    if key in _CACHE:
        return _CACHE[key]
    lens = lat_lens(kind, size)
    if kind == "sample":
        src = dict(cond=inputs(size)["cond"], img=start_image(e, size).clone())
    elif kind in ("decode", "codes"):
        src = dict(wav=inputs(size)["wav"])
        if kind == "codes":
            src["codes"] = e.get_cond(src["wav"], return_codes=True)[1].clone()
    else:
        wav = synth.synthetic_wav(B, size * HOP, seed=92) * 0.5
        for b, n in enumerate(lens):
            wav[b, :, n * HOP:] = 0
        src = dict(wav=cu(wav))
        if kind == "codes_ragged":
            src["codes"] = e.get_cond_ragged(src["wav"], [n * HOP for n in lens], return_codes=True)[1].clone()
    _CACHE[key] = src
    return src


def run(e, kind, size, ddim, seeds=None, tape=None, items=(0, 1, 2), eta=ETA, solo=False):
    """One call of the case's entry on `items` of its inputs -> {"latents" [, "wav"]} (clones).
    seeds given: the seeded entry.  Else the existing entry, with `tape` as its noise (None: it draws under the context's epoch).
    solo (one item): the item alone on its OWN length through the rectangular entry."""
    src, lens = source(e, kind, size), lat_lens(kind, size)
    items = list(items)
    lens = [lens[b] for b in items]
    Lm = max(lens)
    ragged = is_ragged(kind) and not solo
    kw = dict(t_start=T_START, eta=eta) if ddim else {}
    skw = dict(sampler="ddim", **kw) if ddim else {}
    if kind == "sample":
        cond, img = src["cond"][items].contiguous(), src["img"][items].contiguous()
        if seeds is not None:
            out = dict(latents=e.sample_seeded(img, cond, seeds, N, **skw))
        elif ddim:
            out = dict(latents=e.ddim_sample(cond, T_START, N, eta, img=img, noise=tape))
        else:
            out = dict(latents=e.denoise(img, cond, N, tape))
    elif kind in ("decode", "ragged"):
        wav = src["wav"][items][:, :, :Lm * HOP].contiguous()
        slens = [n * HOP for n in lens]
        if seeds is not None:
            out = e.decode_seeded(wav, seeds, N, lengths=slens if ragged else None, want_stages=True, **skw)
        elif ragged:
            out = e.decode_ragged(wav, slens, N, noise=tape, want_stages=True, **kw)
        elif ddim:
            out = e.decode_ddim(wav, T_START, N, eta, noise=tape, per_item=True, want_stages=True)
        else:
            out = e.decode(wav, N, tape, per_item=True, want_stages=True)
    else:
        up = CHOP // HOP
        codes = src["codes"][:, items][:, :, :Lm // up].contiguous()
        fr = [n // up for n in lens]
        if seeds is not None:
            out = e.decode_codes_seeded(seeds, codes=codes, lengths=fr if ragged else None, n_steps=N, want_stages=True, **skw)
        elif ragged:
            out = e.decode_codes_ragged(codes=codes, frames=fr, n_steps=N, noise=tape, want_stages=True, **kw)
        elif ddim:
            out = e.decode_codes_ddim(codes=codes, t_start=T_START, n_steps=N, eta=eta, noise=tape, per_item=True, want_stages=True)
        else:
            out = e.decode_codes(codes=codes, n_steps=N, noise=tape, per_item=True, want_stages=True)
    return {k: out[k].clone() for k in ("latents", "wav") if k in out}


def own_tape(kind, size, seeds, items=(0, 1, 2)):
    lens = [lat_lens(kind, size)[b] for b in items]
    return cu(assembled_tape(seeds, N, C, lens))


def compare_items(dtype, got, ref, lens, what, lat_key="chain_small", wav_key="wav", ragged=False, ref_items=None):
    """item by item on its own length; exact zeros behind every length of `got`"""
    for b, n in enumerate(lens):
        rb = b if ref_items is None else ref_items[b]
        close(dtype, lat_key, rel(npy(got["latents"][b, :, :n]), npy(ref["latents"][rb, :, :n])), f"{what} item {b} latents", ragged)
        assert not got["latents"][b, :, n:].any(), (what, b)
        if "wav" in got:
            close(dtype, wav_key, rel(npy(got["wav"][b, :, :n * HOP]), npy(ref["wav"][rb, :, :n * HOP])), f"{what} item {b} wav", ragged)
            assert not got["wav"][b, :, n * HOP:].any(), (what, b)


def name_of(kind, size, ddim):
    return f"{kind} {size} {'ddim eta 1' if ddim else 'ddpm'}"


# ------------------------------------------------------------------------------------ 1. seeded against the assembled tape
TAPE_CASES = [(k, s, d) for k, sizes in (("sample", (160, 80)), ("decode", (160, 80)), ("ragged", (320, 240)), ("codes", (80,)),
                                         ("codes_ragged", (320, 240))) for s in sizes for d in (False, True)]


@pytest.mark.parametrize("kind,size,ddim", TAPE_CASES)
def test_seeded_equals_the_assembled_tape(kind, size, ddim):
    e = engine("r84", "f32")
    got = run(e, kind, size, ddim, seeds=SEEDS)
    ref = run(e, kind, size, ddim, tape=own_tape(kind, size, SEEDS))
    compare_items("f32", got, ref, lat_lens(kind, size), name_of(kind, size, ddim))


@pytest.mark.parametrize("kind,size", [("sample", 80), ("decode", 160), ("ragged", 240), ("codes_ragged", 320)])
def test_seeded_equals_the_assembled_tape_bf16(kind, size):
    e = engine("r84", "bf16")
    got = run(e, kind, size, False, seeds=SEEDS)
    ref = run(e, kind, size, False, tape=own_tape(kind, size, SEEDS))
    compare_items("bf16", got, ref, lat_lens(kind, size), name_of(kind, size, False) + " bf16")


# -------------------------------------------------------------------------------------------------------------- 2. as if alone
def alone_figures(e, kind, size, ddim, seeded):
    """[(what, "latents" | "wav", value)]: item b of the batch of three against the item solo on its own length.
    seeded: the seeded call against reseed(s_b) + the unseeded entry at B = 1.  Else (the measurement behind ALONE_BF16_MEASURED, code
    that exists on the parent): the explicit-tape call on the assembled tape against the B = 1 call on the item's own tape."""
    lens = lat_lens(kind, size)
    batch = run(e, kind, size, ddim, seeds=SEEDS) if seeded else run(e, kind, size, ddim, tape=own_tape(kind, size, SEEDS))
    out = []
    for b, n in enumerate(lens):
        if seeded:
            e.reseed(SEEDS[b])
            one = run(e, kind, size, ddim, items=[b], solo=True)
        else:
            one = run(e, kind, size, ddim, tape=own_tape(kind, size, [SEEDS[b]], [b]), items=[b], solo=True)
        out.append((f"{name_of(kind, size, ddim)} item {b}", "latents", rel(npy(batch["latents"][b, :, :n]), npy(one["latents"][0]))))
        if "wav" in batch:
            out.append((f"{name_of(kind, size, ddim)} item {b}", "wav", rel(npy(batch["wav"][b, :, :n * HOP]), npy(one["wav"][0]))))
    return out


def measure_alone(dtype="bf16"):
    """the figures behind ALONE_BF16_MEASURED: worst latents / waveform figure over ALONE_CASES on the explicit-tape paths"""
    e = engine("r84", dtype)
    worst = {"latents": 0.0, "wav": 0.0}
    for kind, size, ddim in ALONE_CASES:
        for what, key, v in alone_figures(e, kind, size, ddim, seeded=False):
            print(f"alone (explicit tapes) {dtype} {what} {key}: {v:.3e}")
            worst[key] = max(worst[key], v)
    return worst


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind,size,ddim", ALONE_CASES)
def test_an_item_of_a_seeded_batch_is_the_item_alone(kind, size, ddim, dtype):
    e = engine("r84", dtype)
    for what, key, v in alone_figures(e, kind, size, ddim, seeded=True):
        close(dtype, "alone" if key == "latents" else "alone_wav", v, f"{what} against reseed + the unseeded B = 1 call: {key}")


# ---------------------------------------------------------------------------------------------- 3. order and company do not matter
def arrangements(e, kind, size, ddim, seeded):
    """[(what, result, the B = 3 result, the items' lengths, their places in the B = 3 batch)]: the items permuted (seeds with them), two of
    them at B = 2, and all three under split 1.  seeded False: the same arrangements through the explicit-tape entries (every item's own
    tape travels with it): code the parent has, the measurement behind RAGGED_DDIM_ETA1_BF16_REPEAT."""
    lens = lat_lens(kind, size)

    def go(items):
        seeds = [SEEDS[b] for b in items]
        return run(e, kind, size, ddim, seeds=seeds, items=items) if seeded else run(e, kind, size, ddim, tape=own_tape(kind, size, seeds, items), items=items)

    base = go([0, 1, 2])
    out = [(f"{what}", go(items), base, [lens[b] for b in items], items)
           for what, items in (("permuted", [2, 0, 1]), ("B = 2 [0, 2]", [0, 2]), ("B = 2 [1, 2]", [1, 2]))]   # (ragged 240: the pair [0, 2] is padded to 160)
    try:
        e.set_option("split", 1)
        out.append(("split 1 against the default split", go([0, 1, 2]), base, lens, [0, 1, 2]))
    finally:
        e.set_option("split", 2)
    return out


def measure_order(dtype="bf16", kind="ragged", size=240, ddim=True):
    """worst latents / waveform figure of `arrangements` on the explicit-tape path"""
    e = engine("r84", dtype)
    worst = {"latents": 0.0, "wav": 0.0}
    for what, got, base, lens, items in arrangements(e, kind, size, ddim, seeded=False):
        for b, n in enumerate(lens):
            for key, m in (("latents", n), ("wav", n * HOP)):
                v = rel(npy(got[key][b, :, :m]), npy(base[key][items[b], :, :m]))
                print(f"order (explicit tapes) {dtype} {name_of(kind, size, ddim)} {what} item {b} {key}: {v:.3e}")
                worst[key] = max(worst[key], v)
    return worst


@pytest.mark.parametrize("kind,size,ddim,dtype", [("sample", 80, False, "f32"), ("ragged", 240, True, "f32"), ("ragged", 240, True, "bf16"),
                                                  ("codes_ragged", 320, False, "f32")])
def test_order_company_and_split_do_not_matter(kind, size, ddim, dtype):
    e = engine("r84", dtype)
    rag, lens = is_ragged(kind), lat_lens(kind, size)
    for what, got, base, ln, items in arrangements(e, kind, size, ddim, seeded=True):
        compare_items(dtype, got, base, ln, f"{name_of(kind, size, ddim)} {what}", "repeat_lat", "repeat", rag, ref_items=items)
    other = run(e, kind, size, ddim, seeds=OTHER)                   # (other seeds, other noise: the comparisons above are not vacuous)
    assert rel(npy(base["latents"][0, :, :lens[0]]), npy(other["latents"][0, :, :lens[0]])) > 100 * bar_of(dtype, "repeat", rag)


# --------------------------------------------------------------------------------------------------------- 4. seeds are data
def fresh_inputs(e, L, seed):
    """a shape no other test of the suite uses, so the order of first use below is this test's"""
    wav = cu(synth.synthetic_wav(B, L * HOP, seed=seed) * 0.5)
    cond = e.get_cond(wav).clone()
    return cond, e.cond_upsample(cond, 2).clone()


@pytest.mark.parametrize("ddim", [False, True])
@pytest.mark.parametrize("first,L", [("seeded", 400), ("unseeded", 480)])
def test_seeds_are_data_and_the_two_kinds_of_graph_never_mix(first, L, ddim):
    e = engine("r84", "f32")
    cond, img = fresh_inputs(e, L, 95)
    skw = dict(sampler="ddim", t_start=T_START, eta=ETA) if ddim else {}

    def seeded(seeds):
        return e.sample_seeded(img, cond, seeds, N, **skw).clone()

    def unseeded(tape=None):
        e.reseed(SEEDS[0])
        return (e.ddim_sample(cond, T_START, N, ETA, img=img, noise=tape) if ddim else e.denoise(img, cond, N, tape)).clone()

    if first == "seeded":
        s0, u0 = seeded(SEEDS), unseeded()
    else:
        u0, s0 = unseeded(), seeded(SEEDS)
    s1, u1, s2, u2 = seeded(OTHER), unseeded(), seeded(SEEDS), unseeded()
    what = f"L {L} {'ddim' if ddim else 'ddpm'}, {first} first"
    close("f32", "repeat", rel(npy(s2), npy(s0)), f"{what}: the first seeds again, behind other seeds and unseeded calls")
    close("f32", "repeat", rel(npy(u1), npy(u0)), f"{what}: the unseeded call again (reseeded), behind seeded calls")
    close("f32", "repeat", rel(npy(u2), npy(u0)), f"{what}: and once more")
    for got, seeds, name in ((s0, SEEDS, "first seeds"), (s1, OTHER, "other seeds (graphs replayed)")):
        ref = unseeded(cu(assembled_tape(seeds, N, C, [L] * B)))
        close("f32", "chain_small", rel(npy(got), npy(ref)), f"{what}: {name} against their assembled tape")
    ref = unseeded(cu(P.tape_steps(P.call_key(SEEDS[0], 0), N, B, C, L, split=2)))
    close("f32", "chain_small", rel(npy(u1), npy(ref)), f"{what}: the unseeded call against the batch-position tape of its epoch")
    assert rel(npy(s1), npy(s0)) > 100 * TOL["f32"]["chain_small"] and rel(npy(u0), npy(s0)) > 100 * TOL["f32"]["chain_small"]


# ------------------------------------------------------------------------------------------------------ 5. the epoch is untouched
@pytest.mark.parametrize("ddim", [False, True])
def test_seeded_calls_neither_read_nor_advance_the_epoch(ddim):
    e = engine("r84", "f32")
    e.reseed(5)
    plain = run(e, "decode", 80, ddim)
    e.reseed(5)
    run(e, "decode", 80, ddim, seeds=SEEDS)
    run(e, "sample", 80, ddim, seeds=OTHER)
    run(e, "ragged", 240, ddim, seeds=SEEDS)
    after = run(e, "decode", 80, ddim)
    compare_items("f32", after, plain, [80] * B, "a decode behind seeded calls against one without them", "repeat", "repeat")
    again = run(e, "decode", 80, ddim)                              # (and that decode moved the epoch on: the check above is not vacuous)
    assert rel(npy(again["latents"]), npy(plain["latents"])) > 100 * TOL["f32"]["repeat"]


# ----------------------------------------------------------------------------------------------- 6. the test can see the old layout
@pytest.mark.parametrize("kind,size,ddim,items", [("ragged", 240, False, (0, 1, 2)), ("ragged", 320, True, (0, 2)), ("sample", 80, False, (1, 2)),
                                                  ("decode", 160, True, (1, 2))])
def test_the_bar_tells_the_item_alone_layout_from_the_batch_position_layout(kind, size, ddim, items):
    """The explicit-tape entry on the items' own tapes against the same entry on the batch-position tapes of the SAME keys
    (philox_oracle.tape_steps: g = elem_base + (b C + c_first) Lmax + l).  Chosen items: in a ragged batch those shorter than Lmax, in a
    rectangular one those behind item 0 (item 0 of the first part is the one whose two layouts coincide)."""
    e = engine("r84", "f32")
    lens, what = lat_lens(kind, size), name_of(kind, size, ddim)
    own = own_tape(kind, size, SEEDS)
    old = own.clone()
    for b in items:
        old[:, b] = cu(P.tape_steps(SEEDS[b], N, B, C, max(lens), split=2, lens=lens if is_ragged(kind) else None)[:, b])
    right, wrong, got = run(e, kind, size, ddim, tape=own), run(e, kind, size, ddim, tape=old), run(e, kind, size, ddim, seeds=SEEDS)
    bar = TOL["f32"]["chain_small"]
    for b in items:
        n = lens[b]
        apart = rel(npy(wrong["latents"][b, :, :n]), npy(right["latents"][b, :, :n]))
        side = rel(npy(got["latents"][b, :, :n]), npy(right["latents"][b, :, :n]))
        print(f"item seeds f32 {what} item {b}: the two layouts are {apart:.3e} apart (100 bars: {100 * bar:.3e}); seeded against the own-tape run {side:.3e}")
        assert apart > 100 * bar, (what, b, apart)
        assert side < bar, (what, b, side)


# ------------------------------------------------------------------------------------------------------------- 7. DDIM at eta 0
@pytest.mark.parametrize("kind,size", [("sample", 80), ("ragged", 240)])
def test_ddim_at_eta_0_takes_seeds_and_draws_nothing(kind, size):
    e = engine("r84", "f32")
    a = run(e, kind, size, True, seeds=SEEDS, eta=0.0)
    b = run(e, kind, size, True, seeds=OTHER, eta=0.0)
    compare_items("f32", b, a, lat_lens(kind, size), f"{kind} {size} ddim eta 0 under other seeds", "repeat", "repeat")
    ref = run(e, kind, size, True, eta=0.0)                          # (the unseeded entry, which draws nothing either)
    compare_items("f32", a, ref, lat_lens(kind, size), f"{kind} {size} ddim eta 0 against the unseeded entry", "repeat", "repeat")


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_name_the_value_and_leave_no_gpu_work_behind():
    e = engine("r84", "f32")
    s, r, c = source(e, "sample", 80), source(e, "ragged", 240), source(e, "codes_ragged", 240)
    rl = [n * HOP for n in lat_lens("ragged", 240)]
    fr = [n * HOP // CHOP for n in lat_lens("ragged", 240)]
    good = run(e, "ragged", 240, True, seeds=SEEDS)
    e.reseed(11)
    plain = run(e, "decode", 80, False)
    engine("r84", "fp8")                                              # (built in front of the count below)
    syncs = L.load().ldc_debug_sync_count()
    ddim = dict(sampler="ddim", t_start=T_START, eta=ETA)
    cases = [
        ("seeds NULL", lambda: e.sample_seeded(s["img"], s["cond"], None, N)),
        ("seeds NULL", lambda: e.decode_seeded(r["wav"], None, N, lengths=rl)),
        ("seeds NULL", lambda: e.decode_codes_seeded(None, codes=c["codes"], lengths=fr, n_steps=N)),
        ("sampler 2", lambda: e.sample_seeded(s["img"], s["cond"], SEEDS, N, sampler=2, t_start=T_START)),
        ("sampler 2", lambda: e.decode_seeded(r["wav"], SEEDS, N, lengths=rl, sampler=2, t_start=T_START)),
        ("sampler 2", lambda: e.decode_codes_seeded(SEEDS, codes=c["codes"], lengths=fr, n_steps=N, sampler=2, t_start=T_START)),
        ("sampler -1", lambda: e.decode_seeded(r["wav"], SEEDS, N, sampler=-1)),
        # what the unseeded entries refuse
        ("n_steps", lambda: e.sample_seeded(s["img"], s["cond"], SEEDS, 0)),
        ("n_steps", lambda: e.sample_seeded(s["img"], s["cond"], SEEDS, T_START + 1, **ddim)),
        ("t_start", lambda: e.sample_seeded(s["img"], s["cond"], SEEDS, N, sampler="ddim", t_start=1001)),
        ("t_start", lambda: e.decode_seeded(r["wav"], SEEDS, N, lengths=rl, sampler="ddim", t_start=0)),
        ("eta", lambda: e.decode_seeded(r["wav"], SEEDS, N, lengths=rl, sampler="ddim", t_start=T_START, eta=1.5)),
        ("eta", lambda: e.decode_codes_seeded(SEEDS, codes=c["codes"], n_steps=N, sampler="ddim", t_start=T_START, eta=float("nan"))),
        ("n_steps", lambda: e.decode_seeded(r["wav"], SEEDS, 1001)),
        ("length", lambda: e.decode_seeded(r["wav"], SEEDS, N, lengths=[rl[0] + 320] + rl[1:])),
        ("length", lambda: e.decode_codes_seeded(SEEDS, codes=c["codes"], lengths=[fr[0] + 1] + fr[1:], n_steps=N)),
        ("must equal", lambda: e.sample_seeded(s["img"][:, :, :70].contiguous(), s["cond"], SEEDS, N)),
        ("fp8", lambda: engine("r84", "fp8").decode_seeded(r["wav"], SEEDS, N, lengths=rl)),
        ("fp8", lambda: engine("r84", "fp8").decode_codes_seeded(SEEDS, codes=c["codes"], lengths=fr, n_steps=N)),
    ]
    for word, call in cases:
        with pytest.raises(L.LdcError) as ei:
            call()
        assert ei.value.code == L.E_INVALID, (word, str(ei.value))
        assert word in str(ei.value), (word, str(ei.value))
    with pytest.raises(ValueError):
        e.decode_seeded(r["wav"], SEEDS[:2], N, lengths=rl)           # two seeds for three items: refused in front of the library
    assert L.load().ldc_debug_sync_count() == syncs                   # no refusal waited for the device
    again = run(e, "ragged", 240, True, seeds=SEEDS)
    compare_items("f32", again, good, lat_lens("ragged", 240), "the good call again behind the refusals", "repeat", "repeat")
    e.reseed(11)                                                      # nor did one move the epoch or leave a half-written table behind
    compare_items("f32", run(e, "decode", 80, False), plain, [80] * B, "an unseeded decode behind the refusals", "repeat", "repeat")


# ----------------------------------------------------------------------------------------------------------------------- 9. CLI
CLI_STEPS = 6
CLI_LENGTHS = [5120, 7680, 5120, 7680, 5120]                      # two lengths, whole quanta: --ragged and the 640-sample trim keep every sample


def _flags(root, ind, outd, *extra):
    return ["--model_for_cond", str(root / "codec.amlt"), "--model_path", str(root / "ladiff.amlt"), "--run_diff", "--scaling_global",
            "--cond_bandwidth", "3", "--unet_scale_cond", "--enc_ratios", "8", "4", "--upsampling_ratios", "5", "2", "--diff_dims", "32",
            "--input_dir", str(ind) + "/", "--output_dir", str(outd) + "/", "--midway_t", str(CLI_STEPS), "--dtype", "f32",
            "--seed", str((1 << 64) - 3), *extra]                   # (file 3 and 4 wrap around 2^64)


@pytest.fixture(scope="module")
def cli_tree(tmp_path_factory):
    """five short files of two lengths, their containers, and the --batch_size 1 runs every other run is held to"""
    from scipy.io import wavfile
    from ladiffcodec_amd import compress, decompress
    root = tmp_path_factory.mktemp("item_seeds_cli")
    synth.save_amlt(main_sd_np("r84"), str(root / "ladiff.amlt"))
    synth.save_amlt(cond_sd_np(), str(root / "codec.amlt"))
    ind = root / "in"
    ind.mkdir()
    names = [f"u{k}.wav" for k in range(len(CLI_LENGTHS))]
    for k, (name, n) in enumerate(zip(names, CLI_LENGTHS)):
        wavfile.write(str(ind / name), 16000, (synth.synthetic_wav(1, n, seed=120 + k)[0, 0] * 0.5).astype(np.float32))
    assert len(compress.main(_flags(root, ind, root / "enc"))) == len(names)
    sample.main(_flags(root, ind, root / "ref_sample", "--item_seeds", "--batch_size", "1"))
    decompress.main(_flags(root, root / "enc", root / "ref_decompress", "--item_seeds", "--batch_size", "1"))
    return root, names


def _read(path):
    from scipy.io import wavfile
    return wavfile.read(str(path))[1]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("cli", ["sample", "decompress"])
def test_cli_item_seeds_do_not_depend_on_the_batching(cli_tree, cli, ragged):
    from ladiffcodec_amd import decompress
    root, names = cli_tree
    main, src = (sample.main, root / "in") if cli == "sample" else (decompress.main, root / "enc")
    for bs in ([1, 2, 4] if ragged else [2, 4]):                    # (without --ragged the --batch_size 1 run is the reference itself)
        out = root / f"{cli}_{'ragged' if ragged else 'equal'}_{bs}"
        main(_flags(root, src, out, "--item_seeds", "--batch_size", str(bs), *(["--ragged"] if ragged else [])))
        for name, n in zip(names, CLI_LENGTHS):
            y, r = _read(out / name), _read(root / f"ref_{cli}" / name)
            assert y.shape == (n,) and r.shape == (n,), name
            close("f32", "wav", rel(y, r), f"{cli} --item_seeds{' --ragged' if ragged else ''} --batch_size {bs} {name} against --batch_size 1")
    # the seeds matter (file 0 is not file 2 under file 2's seed), and without the flag the run draws by batch position as it always did
    if cli == "sample" and not ragged:
        a, b = _read(root / "ref_sample" / names[0]), _read(root / "ref_sample" / names[2])
        assert rel(a, b) > 100 * WAV_BAR["f32"]


def test_cli_refuses_item_seeds_with_chunks_and_on_multichannel_files(cli_tree, tmp_path):
    from scipy.io import wavfile
    root, _ = cli_tree
    with pytest.raises(SystemExit) as ei:
        sample.main(_flags(root, root / "in", tmp_path / "o1", "--item_seeds", "--chunk_sec", "0.2"))
    assert "--chunk_sec" in str(ei.value)
    st = tmp_path / "stereo"
    st.mkdir()
    wavfile.write(str(st / "st.wav"), 16000, np.ascontiguousarray((synth.synthetic_wav(2, 5120, seed=130)[:, 0] * 0.5).astype(np.float32).T))
    with pytest.raises(SystemExit) as ei:
        sample.main(_flags(root, st, tmp_path / "o2", "--item_seeds"))
    assert "more than one channel" in str(ei.value)
    assert not os.path.exists(tmp_path / "o2" / "st.wav")
