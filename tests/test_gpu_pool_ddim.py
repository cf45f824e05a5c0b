"""DDIM items in decode pools on the GPU: a sampler and a schedule per slot (ldc_pool_admit_ddim, `DecodePool.submit(t_start=...)`).

References are the CPU oracle's SOLO results -- `oracle_ddim` of tests/test_gpu_ragged.py on the item alone with its own tape and
schedule, the oracle's halfway sampling for DDPM items -- or the engine's unchanged B = 1 entry points (`Engine.ddim_sample` for the
Philox check).  Never the pool.  Items are those of tests/test_gpu_pool.py (latent lengths 240, 80, 400, 160 and 160 frames on `r84`:
80 is no multiple of the 32-wide tile of the update kernel), each DDIM item with a tape of its own.

Bars.  Latents, f32: TOL["f32"]["chain_small"].  Latents, bf16: no bar existed for DDIM (test_decode_ragged_ddim checks waveforms
only), so the path this one shares its launch forms with was measured: `Engine.decode_ragged(t_start, eta)` at B = 1 on the same
items and tapes against the same oracle latents on MI355X (`ragged_b1_latents` below prints the figures under LDC_RECORD_DRIFT).  Two
runs per tag gave 1.51e-3 and 1.81e-3 on `r84` (item C, eta 1) and 1.69e-3 and 1.66e-3 on `r8`; RAGGED_B1_DDIM_LATENTS holds the worst,
the pool is held to 2 x it, the margin of tests/drift_tolerances.py (pool values recorded: up to 1.91e-3).
Waveforms: the ragged bar quoted in tests/test_gpu_pool.py, f32 1e-5 and bf16 2 x 8.1e-4, with that file's rule: a recorded pool value
above 8.1e-4 gets a measured constant of its own and a bar of twice it.  DDIM items at eta 1 on `r8` do exceed it: 8.95e-4 (C) and
8.25e-4 (E) in the pool, and the B = 1 ragged decode of the same items gives 9.00e-4 and 8.34e-4, so this is the ragged DDIM path's own
drift on these items, not the pool's.  POOL_DDIM_MEASURED holds 9.0e-4; the bf16 bar here is 1.8e-3.  DDPM items
keep tests/test_gpu_pool.py's bar through its `check_item`.  Every check prints its figure before it asserts."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
from oracle import ldc_oracle as O, philox_oracle as PX  # noqa: E402
from test_gpu_pool import WAV_BAR, check_item, setup, submit  # noqa: E402
from test_gpu_ragged import oracle_ddim  # noqa: E402

# bf16 latents of B = 1 ragged DDIM decodes (Engine.decode_ragged, the code before pools had DDIM items) against the oracle, worst
# over the items of DDIM below, both tags and two runs each, MI355X; DESIGN.md section 5d quotes it
RAGGED_B1_DDIM_LATENTS = {"bf16": 1.82e-3}
POOL_DDIM_MEASURED = {"bf16": {"wav_small": 9.0e-4}}   # r8, item C (40, 8, eta 1): 8.95e-4 in the pool, 9.00e-4 through decode_ragged at B = 1
DDIM_WAV_BAR = {"f32": WAV_BAR["f32"], "bf16": max(2.0 * POOL_DDIM_MEASURED["bf16"]["wav_small"], WAV_BAR["bf16"])}
# name: (item of tests/test_gpu_pool.py whose waveform it is, t_start, n_steps, eta)
DDIM = {"B": ("B", 40, 8, 0.0), "C": ("C", 40, 8, 1.0), "D": ("D", 25, 4, 0.5), "E": ("E", 40, 7, 1.0),
        "one": ("B", 40, 1, 1.0),                   # the only iteration is the last: x <- x0
        "dense": ("D", 6, 6, 1.0)}                  # stride 1
_CACHE = {}


def lat_bar(dtype):
    return TOL["f32"]["chain_small"] if dtype == "f32" else 2.0 * RAGGED_B1_DDIM_LATENTS[dtype]


def solo_ddim(s, src, t_start, S, eta, tape):
    """the oracle's DDIM decode of one item alone, from the oracle's own start image and condition"""
    r = s["items"][src]["ref"]
    lat = oracle_ddim(s["sdm"], s["u"], r["img0"], r["cond"], t_start, S, eta, tape)
    return dict(latents=lat, wav=O.output_normalise(O.seanet_decode(s["sdm"], s["mc"], lat), True))


def ddim_setup(tag):
    """tests/test_gpu_pool.py's items plus, for every entry of DDIM, a tape of its own and the oracle's solo DDIM decode"""
    if tag in _CACHE:
        return _CACHE[tag]
    s = setup(tag)
    g = torch.Generator().manual_seed(41)
    items = {}
    for name, (src, t_start, S, eta) in DDIM.items():
        it = s["items"][src]
        tape = torch.randn(S, 1, 128, it["n"] // s["hop"], generator=g)
        items[name] = dict(wav=it["wav"], n=it["n"], tape=tape, t_start=t_start, steps=S, eta=eta, ref=solo_ddim(s, src, t_start, S, eta, tape))
    _CACHE[tag] = dict(s, ddim=items)
    return _CACHE[tag]


def submit_ddim(pool, it, **kw):
    kw.setdefault("noise", it["tape"].cuda())
    return pool.submit(wav=it["wav"].cuda(), n_steps=it["steps"], t_start=it["t_start"], eta=it["eta"], **kw)


def check_ddim(dtype, it, out, what):
    lat = rel(out["latents"].cpu().numpy(), it["ref"]["latents"].numpy())
    wav = rel(out["wav"].cpu().numpy(), it["ref"]["wav"].numpy())
    print(f"pool ddim {dtype} {what}: latents {lat:.3e} (bar {lat_bar(dtype):.3e}), wav {wav:.3e} (bar {DDIM_WAV_BAR[dtype]:.3e})")
    assert tuple(out["wav"].shape) == (1, 1, it["n"])
    assert torch.isfinite(out["latents"]).all()
    assert lat < lat_bar(dtype), (dtype, what, "latents", lat, lat_bar(dtype))
    assert wav < DDIM_WAV_BAR[dtype], (dtype, what, "wav", wav, DDIM_WAV_BAR[dtype])


def ragged_b1_latents(e, s, dtype, tag):
    """the figure behind RAGGED_B1_DDIM_LATENTS: every DDIM item through Engine.decode_ragged at B = 1 against the oracle's latents"""
    worst = 0.0
    for name, it in s["ddim"].items():
        got = e.decode_ragged(it["wav"].cuda(), [it["n"]], it["steps"], t_start=it["t_start"], eta=it["eta"], noise=it["tape"].cuda(),
                              want_stages=True)
        v = rel(got["latents"].cpu().numpy(), it["ref"]["latents"].numpy())
        w = rel(got["wav"].cpu().numpy(), it["ref"]["wav"].numpy())
        print(f"ragged B=1 ddim {tag} {dtype} {name}: latents {v:.3e}, wav {w:.3e}")
        worst = max(worst, v)
    return worst


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_mixed_staggered_pool(tag, dtype):
    s = ddim_setup(tag)
    e = engine(tag, dtype)
    if os.environ.get("LDC_RECORD_DRIFT"):
        print(f"ragged B=1 ddim {tag} {dtype} worst latents: {ragged_b1_latents(e, s, dtype, tag):.3e}")
    d = s["ddim"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        t, out = {}, {}
        t["A"] = submit(pool, s["items"]["A"])                  # DDPM, 10 steps
        pool.step(3)                                             # one eager step, then both graphs are captured (the single-step one replayed twice):
        assert pool.remaining() == [7, -1, -1, -1]               # no DDIM item has existed so far
        t["B"] = submit_ddim(pool, d["B"]); pool.step(5)         # the 5-step graph
        t["C"] = submit_ddim(pool, d["C"]); t["D"] = submit_ddim(pool, d["D"])
        assert pool.free_slots() == [] and pool.remaining() == [2, 3, 8, 4]
        pool.step(3)
        assert pool.finished() == [t["A"], t["B"]] and pool.remaining() == [0, 0, 5, 1]
        slot_b = pool._slot_of[t["B"]]
        out["B"] = pool.pop(t["B"])
        t["E"] = submit_ddim(pool, d["E"])                       # into B's slot while C (5 to go) and D (1 to go) are mid-flight
        assert pool._slot_of[t["E"]] == slot_b
        out["A"] = pool.pop(t["A"])
        t["one"] = submit_ddim(pool, d["one"])
        pool.step(1)
        assert pool.finished() == [t["D"], t["one"]] and pool.remaining() == [0, 6, 4, 0]
        out["D"], out["one"] = pool.pop(t["D"]), pool.pop(t["one"])
        t["dense"] = submit_ddim(pool, d["dense"])
        pool.run_until_done()
        for k in ("C", "E", "dense"):
            out[k] = pool.pop(t[k])
        assert pool.free_slots() == [0, 1, 2, 3]
        check_item(dtype, s["items"]["A"], out["A"], (tag, "A (DDPM) before and among DDIM items"))
        for k in DDIM:
            check_ddim(dtype, d[k], out[k], (tag, k))
    finally:
        pool.close()


def test_the_schedule_is_per_item():
    s = ddim_setup("r84")
    e = engine("r84", "f32")
    d = s["ddim"]
    bar = TOL["f32"]["chain_small"]
    # B (40, 8, eta 0) and D (25, 4, eta 0.5): each under the other's schedule on the oracle alone, with its own tape where it reaches
    own = {k: d[k]["ref"]["latents"] for k in "BD"}
    other = {}
    for k, o in (("B", "D"), ("D", "B")):
        S = d[o]["steps"]
        tape = d[k]["tape"]
        tape = tape[:S] if tape.shape[0] >= S else torch.cat([tape, tape[:S - tape.shape[0]]])
        other[k] = solo_ddim(s, DDIM[k][0], d[o]["t_start"], S, d[o]["eta"], tape)["latents"]
    # and B as a DDPM item of as many steps
    as_ddpm = O.halfway_sampling(s["sdm"], s["u"], s["items"]["B"]["ref"]["img0"], s["items"]["B"]["ref"]["cond"], 8, d["B"]["tape"])
    for k in "BD":
        apart = rel(own[k].numpy(), other[k].numpy())
        print(f"oracle: {k} under its own schedule against {k} under the other's: {apart:.3e} (10 x bar {10 * bar:.3e})")
        assert apart > 10 * bar
    apart = rel(own["B"].numpy(), as_ddpm.numpy())
    print(f"oracle: B as DDIM (40, 8, 0) against B as DDPM (8 steps): {apart:.3e} (10 x bar {10 * bar:.3e})")
    assert apart > 10 * bar
    pool = e.open_pool(4, s["Tmax"])
    try:
        tb = submit_ddim(pool, d["B"]); pool.step(2)
        td = submit_ddim(pool, d["D"])
        tp = pool.submit(wav=d["B"]["wav"].cuda(), n_steps=8, noise=d["B"]["tape"].cuda())       # the same item as DDPM beside it
        pool.run_until_done()
        got = {"B": pool.pop(tb)["latents"].cpu(), "D": pool.pop(td)["latents"].cpu(), "P": pool.pop(tp)["latents"].cpu()}
        for k in "BD":
            err = rel(got[k].numpy(), own[k].numpy())
            print(f"pool f32 {k} against the oracle under {k}'s schedule: {err:.3e} (bar {bar:.3e})")
            assert err < bar
        err_i, err_p = rel(got["B"].numpy(), own["B"].numpy()), rel(got["P"].numpy(), as_ddpm.numpy())
        print(f"pool f32 B as DDIM {err_i:.3e}, B as DDPM {err_p:.3e} (bar {bar:.3e})")
        assert err_i < bar and err_p < bar
    finally:
        pool.close()


def test_philox_items_draw_what_ddim_sample_draws_alone():
    s = ddim_setup("r84")
    e = engine("r84", "f32")
    it = s["ddim"]["D"]                                          # (25, 4, eta 0.5) on 160 frames
    bar = TOL["f32"]["chain_small"]
    Lz = it["n"] // s["hop"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        other = submit(pool, s["items"]["A"])                    # company in another slot, already three steps in
        pool.step(3)
        t1 = submit_ddim(pool, it, noise=None, seed=1234)
        taped = torch.from_numpy(PX.tape_item(1234, it["steps"], 128, Lz)).float()
        t2 = submit_ddim(pool, it, noise=taped.cuda())
        pool.run_until_done()
        a, b = pool.pop(t1)["latents"].cpu(), pool.pop(t2)["latents"].cpu()
        img, cond = e.pool_front(wav=it["wav"].cuda())
        e.reseed(1234)
        solo = e.ddim_sample(cond, it["t_start"], it["steps"], it["eta"], img=img).cpu()
        err_t, err_s = rel(a.numpy(), b.numpy()), rel(a.numpy(), solo.numpy())
        print(f"pool ddim Philox against the oracle's tape of the seed: {err_t:.3e}, against the solo path: {err_s:.3e} (bar {bar:.3e})")
        assert err_t < bar and err_s < bar
        # eta 1: two seeds differ; eta 0: the seed does not matter
        hot, cold = dict(it, eta=1.0), dict(it, eta=0.0)
        th = [submit_ddim(pool, hot, noise=None, seed=k) for k in (1234, 99)]
        pool.run_until_done()
        h = [pool.pop(t)["latents"].cpu() for t in th]
        tc = [submit_ddim(pool, cold, noise=None, seed=k) for k in (1234, 99)]
        pool.run_until_done()
        c = [pool.pop(t)["latents"].cpu() for t in tc]
        apart, same = rel(h[0].numpy(), h[1].numpy()), rel(c[0].numpy(), c[1].numpy())
        print(f"pool ddim two seeds at eta 1: {apart:.3e} apart (10 x bar {10 * bar:.3e}); at eta 0: {same:.3e} (bar {bar:.3e})")
        assert apart > 10 * bar and same < bar
        pool.evict(other)
    finally:
        pool.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_what_is_never_read(dtype):
    s = ddim_setup("r84")
    e = engine("r84", dtype)
    d = s["ddim"]
    bar = lat_bar(dtype)
    pool = e.open_pool(4, s["Tmax"])
    try:
        # the last entry of a tape is never read; at eta 0 none is
        it = d["C"]                                              # (40, 8, eta 1)
        bad = it["tape"].clone()
        bad[-1] = float("nan")
        cold = dict(d["B"])                                      # (40, 8, eta 0)
        t_clean, t_bad = submit_ddim(pool, it), submit_ddim(pool, it, noise=bad.cuda())
        t_nan = submit_ddim(pool, cold, noise=torch.full_like(cold["tape"], float("nan")).cuda())
        t_none = submit_ddim(pool, cold, noise=None)
        pool.run_until_done()
        clean, last_nan = pool.pop(t_clean)["latents"].cpu(), pool.pop(t_bad)["latents"].cpu()
        all_nan, none = pool.pop(t_nan)["latents"].cpu(), pool.pop(t_none)["latents"].cpu()
        assert torch.isfinite(last_nan).all() and torch.isfinite(all_nan).all()
        e1, e2 = rel(last_nan.numpy(), clean.numpy()), rel(all_nan.numpy(), none.numpy())
        print(f"pool ddim {dtype} NaN in the last tape entry: {e1:.3e}; an all-NaN tape at eta 0 against no tape: {e2:.3e} (bar {bar:.3e})")
        assert e1 < bar and e2 < bar
        # a finished DDIM item keeps its latents bit for bit while the others step on; its tape is freed and the block reused
        tape = d["D"]["tape"].cuda()
        td = submit_ddim(pool, d["D"], noise=tape)               # 4 iterations
        tc = submit_ddim(pool, d["C"])
        ta = submit(pool, s["items"]["A"])
        tb = submit_ddim(pool, d["B"], noise=None, seed=7)
        pool.step(4)
        assert pool.finished() == [td] and pool.running() == [tc, ta, tb]
        first = pool.peek(td).clone()
        torch.cuda.synchronize()
        n = tape.numel()
        del tape
        pool._info[td] = (pool._info[td][0], None)               # the pool's own reference to the tape
        junk = torch.full((n,), float("nan"), device="cuda")     # the allocator hands the tape's block out again
        pool.step(3)
        again = pool.peek(td)
        assert torch.equal(first, again), "a finished DDIM item's latents moved while it waited"
        del junk
        pool.run_until_done()
        check_ddim(dtype, d["D"], pool.pop(td), "D after waiting")
        check_ddim(dtype, d["C"], pool.pop(tc), "C in the full pool")
        check_item(dtype, s["items"]["A"], pool.pop(ta), "A (DDPM) in the full pool")
        assert torch.isfinite(pool.pop(tb)["latents"]).all()
    finally:
        pool.close()


def test_ddpm_items_are_unmoved():
    s = ddim_setup("r84")
    e = engine("r84", "f32")
    d = s["ddim"]
    it = s["items"]["C"]                                         # DDPM, 10 steps, 400 frames
    pool = e.open_pool(4, s["Tmax"])
    try:
        tb = submit_ddim(pool, d["B"]); pool.step(1)
        tc = submit(pool, it)
        te, td = submit_ddim(pool, d["E"]), submit_ddim(pool, d["D"])
        assert pool.free_slots() == []
        pool.run_until_done()
        among = pool.pop(tc)
        for t in (tb, te, td):
            pool.pop(t)
        t = submit(pool, it)
        assert len(pool.free_slots()) == 3
        pool.run_until_done()
        alone = pool.pop(t)
        err = rel(among["latents"].cpu().numpy(), alone["latents"].cpu().numpy())
        print(f"pool f32 C (DDPM) among three DDIM items against C alone in the pool: {err:.3e} (bar 1e-5)")
        assert err < 1e-5
        check_item("f32", it, among, "C (DDPM) among three DDIM items")
        check_item("f32", it, alone, "C (DDPM) alone")
    finally:
        pool.close()


def test_refusals_leave_the_pool_usable():
    s = ddim_setup("r84")
    e = engine("r84", "f32")
    d = s["ddim"]
    T = 1000                                                     # timesteps of the schedule
    pool = e.open_pool(4, s["Tmax"])

    def refused(fn, *names):
        before = pool.remaining()
        with pytest.raises(L.LdcError) as ei:
            fn()
        assert ei.value.code == L.E_INVALID, (names, str(ei.value))
        for n in names:
            assert str(n) in str(ei.value), (n, str(ei.value))
        assert pool.remaining() == before
    try:
        tb = submit_ddim(pool, d["B"]); pool.step(2)
        tc = submit_ddim(pool, d["C"])
        img, cond = e.pool_front(wav=d["D"]["wav"].cuda())
        Ld = img.shape[-1]
        h = pool._h
        refused(lambda: e.pool_admit_ddim(h, 2, img, cond, 0, 1, 0.0), "t_start = 0")
        refused(lambda: e.pool_admit_ddim(h, 2, img, cond, T + 1, 4, 0.0), f"t_start = {T + 1}")
        refused(lambda: e.pool_admit_ddim(h, 2, img, cond, 25, 26, 0.0), "n_steps = 26", "t_start = 25")
        refused(lambda: e.pool_admit_ddim(h, 2, img, cond, 25, 0, 0.0), "n_steps = 0")
        refused(lambda: e.pool_admit_ddim(h, 2, img, cond, 25, 4, 1.5), "eta = 1.5")
        refused(lambda: e.pool_admit_ddim(h, 2, img, cond, 25, 4, float("nan")), "eta = nan")
        refused(lambda: e.pool_admit_ddim(h, 0, img, cond, 25, 4, 0.5), "slot 0 is not free")
        refused(lambda: e.pool_admit_ddim(h, 2, img[..., :Ld - 1].contiguous(), cond, 25, 4, 0.5), Ld - 1)      # off the quantum
        refused(lambda: e.pool_admit_ddim(h, 4, img, cond, 25, 4, 0.5), "slot 4")
        refused(lambda: L.check(L.load().ldc_pool_admit_ddim(e._ctx, h, 2, None, cond.data_ptr(), Ld, 25, 4, 0.5, None, 0, None)), "null pointer")
        assert pool.remaining() == [6, 8, -1, -1]
        td = submit_ddim(pool, d["D"])
        pool.run_until_done()
        for k, t in (("B", tb), ("C", tc), ("D", td)):
            check_ddim("f32", d[k], pool.pop(t), (k, "after the refusals"))
    finally:
        pool.close()


def test_warm_mixed_calls_never_wait_for_the_device():
    s = ddim_setup("r84")
    e = engine("r84", "f32")
    d = s["ddim"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        def visit():
            ta = submit(pool, s["items"]["A"]); pool.step(2)
            tb = submit_ddim(pool, d["B"]); td = submit_ddim(pool, d["D"]); pool.step(7); pool.step(1)
            return {"D": (d["D"], pool.pop(td)), "B": (d["B"], pool.pop(tb)), "A": (None, pool.pop(ta))}
        visit()                                                  # plans built, graphs captured, codec ends warm
        torch.cuda.synchronize()
        before = L.load().ldc_debug_sync_count()
        outs = visit()
        torch.cuda.synchronize()
        assert L.load().ldc_debug_sync_count() == before
        for k, (it, o) in outs.items():
            if it is None:
                check_item("f32", s["items"]["A"], o, ("warm", k))
            else:
                check_ddim("f32", it, o, ("warm", k))
    finally:
        pool.close()
