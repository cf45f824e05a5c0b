"""DPM-Solver++(2M) items in decode pools on the GPU: an x0 history per slot (ldc_pool_admit_dpm, `DecodePool.submit(sampler="dpm")`).

References are never the pool.  Primary: `dpm_restatement.dpm_sample` on the item ALONE (CPU oracle's UNet), run on the oracle's own
start image and condition of the item; secondary: the engine's unchanged `Engine.dpm_sample` at B = 1.  Items are those of
tests/test_gpu_pool.py (240, 80, 400, 160 and 160 latent frames on `r84`; 80 is no multiple of the 32-wide tile of the update kernel)
under the schedules of tests/pool_dpm_items.py; tests/test_pool_dpm_cpu.py shows on the restatement that `three`, `C` and `D` are 0.12
to 0.53 away from a run without the `b1` term and from a run fed another item's history (bar x 10: 1e-4).

Bars.  Latents, f32: TOL["f32"]["chain_small"]; waveforms, f32: WAV_BAR["f32"] of tests/test_gpu_pool.py.  bf16 had no bar for DPM on
the unfused launch forms at B = 1, so the parent path was measured as tests/test_gpu_pool_ddim.py did for DDIM:
`Engine.decode_ragged_dpm` at B = 1 on the same items against the same restatement on MI355X (`ragged_b1` below prints the figures
under LDC_RECORD_DRIFT), two runs per tag: worst latents 1.33e-3 and 1.28e-3 on `r84` (items "three" and "one"), 1.59e-3 and 1.66e-3
on `r8` ("one"); worst waveforms 2.6e-4 twice on `r84`, 7.14e-4 and 6.3e-4 on `r8`.  RAGGED_B1_DPM holds the worst of each; the pool's
latents are held to 2 x the former, 3.34e-3 (the margin of tests/drift_tolerances.py), its waveforms to WAV_BAR["bf16"] = 1.62e-3,
which is higher than 2 x the latter (1.43e-3) -- the rule of tests/test_gpu_pool.py.  "Equal" across pools and slots is TOL["f32"]["repeat"]: the step kernels sum GroupNorm statistics with float
atomics.  Every check prints its figure before it asserts."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402
import dpm_restatement as R  # noqa: E402
from pool_dpm_items import DPM  # noqa: E402
from test_gpu_pool import WAV_BAR, check_item, setup, submit  # noqa: E402
from test_gpu_pool_ddim import check_ddim, ddim_setup, submit_ddim  # noqa: E402

# bf16, B = 1 ragged DPM decodes (Engine.decode_ragged_dpm, the code before pools had DPM items) against the restatement: worst over
# the items of DPM, both tags and two runs each, MI355X; DESIGN.md section 5d quotes the runs
RAGGED_B1_DPM = {"bf16": {"latents": 1.67e-3, "wav": 7.15e-4}}   # `r8`, item "one" (40, 1), both
DPM_WAV_BAR = {"f32": WAV_BAR["f32"], "bf16": max(2.0 * RAGGED_B1_DPM["bf16"]["wav"], WAV_BAR["bf16"])}
SAME = TOL["f32"]["repeat"]
_CACHE = {}


def lat_bar(dtype):
    return TOL["f32"]["chain_small"] if dtype == "f32" else 2.0 * RAGGED_B1_DPM[dtype]["latents"]


def dpm_setup(tag):
    """tests/test_gpu_pool.py's items (and the DDIM items of tests/test_gpu_pool_ddim.py) plus, for every entry of DPM, the solo
    restatement from the oracle's own start image and condition of its item, computed once"""
    if tag in _CACHE:
        return _CACHE[tag]
    s = ddim_setup(tag)
    items = {}
    for name, (src, t_start, S) in DPM.items():
        it = s["items"][src]
        lat = R.dpm_sample(s["sdm"], s["u"], it["ref"]["img0"], it["ref"]["cond"], t_start, S)
        ref = dict(latents=lat, wav=O.output_normalise(O.seanet_decode(s["sdm"], s["mc"], lat), True))
        items[name] = dict(wav=it["wav"], n=it["n"], t_start=t_start, steps=S, ref=ref)
    _CACHE[tag] = dict(s, dpm=items)
    return _CACHE[tag]


def submit_dpm(pool, it):
    return pool.submit(wav=it["wav"].cuda(), n_steps=it["steps"], t_start=it["t_start"], sampler="dpm")


def check_dpm(dtype, it, out, what):
    lat = rel(out["latents"].cpu().numpy(), it["ref"]["latents"].numpy())
    wav = rel(out["wav"].cpu().numpy(), it["ref"]["wav"].numpy())
    print(f"pool dpm {dtype} {what}: latents {lat:.3e} (bar {lat_bar(dtype):.3e}), wav {wav:.3e} (bar {DPM_WAV_BAR[dtype]:.3e})")
    assert tuple(out["wav"].shape) == (1, 1, it["n"])
    assert torch.isfinite(out["latents"]).all()
    assert lat < lat_bar(dtype), (dtype, what, "latents", lat, lat_bar(dtype))
    assert wav < DPM_WAV_BAR[dtype], (dtype, what, "wav", wav, DPM_WAV_BAR[dtype])


def ragged_b1(e, s, dtype, tag):
    """the figures behind RAGGED_B1_DPM: every DPM item through Engine.decode_ragged_dpm at B = 1 against the restatement"""
    worst = [0.0, 0.0]
    for name, it in s["dpm"].items():
        got = e.decode_ragged_dpm(it["wav"].cuda(), [it["n"]], it["t_start"], it["steps"], want_stages=True)
        v = rel(got["latents"].cpu().numpy(), it["ref"]["latents"].numpy())
        w = rel(got["wav"].cpu().numpy(), it["ref"]["wav"].numpy())
        print(f"ragged B=1 dpm {tag} {dtype} {name}: latents {v:.3e}, wav {w:.3e}")
        worst = [max(worst[0], v), max(worst[1], w)]
    return worst


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_mixed_staggered_pool(tag, dtype):
    s = dpm_setup(tag)
    e = engine(tag, dtype)
    if os.environ.get("LDC_RECORD_DRIFT"):
        v, w = ragged_b1(e, s, dtype, tag)
        print(f"ragged B=1 dpm {tag} {dtype} worst: latents {v:.3e}, wav {w:.3e}")
    it, dd, d = s["items"], s["ddim"], s["dpm"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        t, out = {}, {}
        t["A"] = submit(pool, it["A"])                           # DDPM, 10 steps, a tape
        pool.step(7)                                             # one eager step, the 5-step graph and the single-step graph: both are
        assert pool.remaining() == [3, -1, -1, -1]               # captured before any DPM item has existed
        t["C"] = submit_dpm(pool, d["C"])
        t["I"] = submit_ddim(pool, dd["C"])                      # DDIM (40, 8) at eta 1 with a tape
        t["three"] = submit_dpm(pool, d["three"])
        assert pool.free_slots() == [] and pool.remaining() == [3, 8, 8, 3]
        pool.step(3)
        assert pool.finished() == [t["A"], t["three"]] and pool.remaining() == [0, 5, 5, 0]
        out["three"], out["A"] = pool.pop(t["three"]), pool.pop(t["A"])
        t["P"] = submit(pool, it["D"])                           # DDPM, 4 steps, a tape: into A's slot while C and I are mid-flight
        t["one"] = submit_dpm(pool, d["one"])                    # into the slot `three` left
        assert pool._slot_of[t["P"]] == 0 and pool._slot_of[t["one"]] == 3
        pool.step(1)
        assert pool.finished() == [t["one"]] and pool.remaining() == [3, 4, 4, 0]
        out["one"] = pool.pop(t["one"])
        t["two"] = submit_dpm(pool, d["two"]); pool.step(2)      # writes the slot's history once and never reads it
        assert pool.finished() == [t["two"]] and pool.remaining() == [1, 2, 2, 0]
        out["two"] = pool.pop(t["two"])
        t["D"] = submit_dpm(pool, d["D"]); pool.step(1)          # behind `two` in the same slot
        assert pool.finished() == [t["P"]] and pool.remaining() == [0, 1, 1, 3]
        out["P"] = pool.pop(t["P"])
        t["dense"] = submit_dpm(pool, d["dense"])
        pool.run_until_done()
        for k in ("C", "I", "D", "dense"):
            out[k] = pool.pop(t[k])
        assert pool.free_slots() == [0, 1, 2, 3]
        for k in DPM:
            check_dpm(dtype, d[k], out[k], (tag, k))
        check_item(dtype, it["A"], out["A"], (tag, "A (DDPM) before and among DPM items"))
        check_item(dtype, it["D"], out["P"], (tag, "D (DDPM) among DPM items"))
        check_ddim(dtype, dd["C"], out["I"], (tag, "C (DDIM, eta 1) among DPM items"))
    finally:
        pool.close()


def test_against_the_engine_alone():
    s = dpm_setup("r84")
    e = engine("r84", "f32")
    d = s["dpm"]
    bar = TOL["f32"]["chain_small"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        ta = submit(pool, s["items"]["A"]); pool.step(2)         # company, two steps in
        tc, t3 = submit_dpm(pool, d["C"]), submit_dpm(pool, d["three"])
        pool.run_until_done()
        got = {"C": pool.pop(tc)["latents"].cpu(), "three": pool.pop(t3)["latents"].cpu()}
        pool.pop(ta)
        for k in ("C", "three"):
            img, cond = e.pool_front(wav=d[k]["wav"].cuda())
            solo = e.dpm_sample(cond, d[k]["t_start"], d[k]["steps"], img).cpu()
            err = rel(got[k].numpy(), solo.numpy())
            print(f"pool dpm f32 {k} against Engine.dpm_sample at B = 1: {err:.3e} (bar {bar:.3e})")
            assert err < bar, (k, err)
    finally:
        pool.close()


def test_stale_history_and_slot_reuse():
    """item D (25, 4) in a fresh pool -- a history block nothing has written -- and then in (b) a slot a DPM item was evicted from
    mid-run, (a) a slot a finished DPM item was popped from, (c) a slot a DDIM item left"""
    s = dpm_setup("r84")
    e = engine("r84", "f32")
    d, dd = s["dpm"], s["ddim"]
    it = d["D"]
    fresh_pool = e.open_pool(4, s["Tmax"])
    try:
        t = submit_dpm(fresh_pool, it)
        fresh_pool.run_until_done()
        fresh = fresh_pool.pop(t)
    finally:
        fresh_pool.close()
    check_dpm("f32", it, fresh, "D in a fresh pool")
    pool = e.open_pool(4, s["Tmax"])
    try:
        tc = submit_dpm(pool, d["C"])                            # slot 0: evicted after three of its eight iterations
        tn = submit_dpm(pool, d["dense"])                        # slot 1: runs its six iterations and is popped
        ti = submit_ddim(pool, dd["D"])                          # slot 2: DDIM (25, 4), eta 0.5
        pool.step(3)
        pool.evict(tc)
        tb = submit_dpm(pool, it)
        assert pool._slot_of[tb] == 0
        pool.run_until_done()
        got = {"b: behind an evicted DPM item": pool.pop(tb)}
        pool.pop(tn); pool.pop(ti)
        hold = submit(pool, s["items"]["B"])                     # keeps slot 0 busy
        ta, tc2 = submit_dpm(pool, it), submit_dpm(pool, it)
        assert (pool._slot_of[ta], pool._slot_of[tc2]) == (1, 2)
        pool.run_until_done()
        got["a: behind a finished DPM item"], got["c: behind a DDIM item"] = pool.pop(ta), pool.pop(tc2)
        pool.pop(hold)
        for k, o in got.items():
            err = rel(o["latents"].cpu().numpy(), fresh["latents"].cpu().numpy())
            print(f"pool dpm f32 D, {k}, against D in a fresh pool: {err:.3e} (bar {SAME:.3e})")
            assert err < SAME, (k, err)
            check_dpm("f32", it, o, k)
    finally:
        pool.close()


def test_a_finished_dpm_item_keeps_its_latents_bit_for_bit():
    s = dpm_setup("r84")
    e = engine("r84", "f32")
    d = s["dpm"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        t3, tc = submit_dpm(pool, d["three"]), submit_dpm(pool, d["C"])
        ta, tn = submit(pool, s["items"]["A"]), submit_dpm(pool, d["dense"])
        pool.step(3)
        assert pool.finished() == [t3] and pool.running() == [tc, ta, tn]
        first = pool.peek(t3).clone()
        pool.step(4)
        again = pool.peek(t3)
        assert torch.equal(first, again), "a finished DPM item's latents moved while it waited"
        pool.run_until_done()
        check_dpm("f32", d["three"], pool.pop(t3), "three after waiting")
        check_dpm("f32", d["C"], pool.pop(tc), "C in the full pool")
        check_dpm("f32", d["dense"], pool.pop(tn), "dense in the full pool")
        check_item("f32", s["items"]["A"], pool.pop(ta), "A (DDPM) in the full pool")
    finally:
        pool.close()


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_ddpm_and_ddim_items_are_unmoved(kind):
    s = dpm_setup("r84")
    e = engine("r84", "f32")
    d = s["dpm"]
    it = s["items"]["C"] if kind == "ddpm" else s["ddim"]["C"]   # 400 frames: DDPM 10 steps / DDIM (40, 8) at eta 1, each with a tape
    sub, chk = (submit, check_item) if kind == "ddpm" else (submit_ddim, check_ddim)
    pool = e.open_pool(4, s["Tmax"])
    try:
        t3 = submit_dpm(pool, d["C"]); pool.step(1)
        tc = sub(pool, it)
        td, tn = submit_dpm(pool, d["D"]), submit_dpm(pool, d["dense"])
        assert pool.free_slots() == []
        pool.run_until_done()
        among = pool.pop(tc)
        for t in (t3, td, tn):
            pool.pop(t)
        t = sub(pool, it)
        assert len(pool.free_slots()) == 3
        pool.run_until_done()
        alone = pool.pop(t)
        err = rel(among["latents"].cpu().numpy(), alone["latents"].cpu().numpy())
        print(f"pool f32 C ({kind}) among three DPM items against C alone in the pool: {err:.3e} (bar 1e-5)")
        assert err < 1e-5
        chk("f32", it, among, f"C ({kind}) among three DPM items")
        chk("f32", it, alone, f"C ({kind}) alone")
    finally:
        pool.close()


def test_refusals_leave_the_pool_usable():
    s = dpm_setup("r84")
    e = engine("r84", "f32")
    d = s["dpm"]
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
        t3 = submit_dpm(pool, d["three"]); pool.step(1)
        tc = submit_dpm(pool, d["C"])
        img, cond = e.pool_front(wav=d["D"]["wav"].cuda())
        Ld = img.shape[-1]
        h = pool._h
        refused(lambda: e.pool_admit_dpm(h, 2, img, cond, 0, 1), "t_start = 0")
        refused(lambda: e.pool_admit_dpm(h, 2, img, cond, T + 1, 4), f"t_start = {T + 1}")
        refused(lambda: e.pool_admit_dpm(h, 2, img, cond, 25, 26), "n_steps = 26", "t_start = 25")
        refused(lambda: e.pool_admit_dpm(h, 2, img, cond, 25, 0), "n_steps = 0")
        refused(lambda: e.pool_admit_dpm(h, 0, img, cond, 25, 4), "slot 0 is not free")
        refused(lambda: e.pool_admit_dpm(h, 2, img[..., :Ld - 1].contiguous(), cond, 25, 4), Ld - 1)      # off the quantum
        refused(lambda: e.pool_admit_dpm(h, 4, img, cond, 25, 4), "slot 4")
        refused(lambda: L.check(L.load().ldc_pool_admit_dpm(e._ctx, h, 2, None, cond.data_ptr(), Ld, 25, 4, None)), "null pointer")
        assert pool.remaining() == [2, 8, -1, -1]
        td = submit_dpm(pool, d["D"])
        pool.run_until_done()
        for k, t in (("three", t3), ("C", tc), ("D", td)):
            check_dpm("f32", d[k], pool.pop(t), (k, "after the refusals"))
    finally:
        pool.close()


def test_warm_dpm_calls_never_wait_for_the_device():
    s = dpm_setup("r84")
    e = engine("r84", "f32")
    d = s["dpm"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        def visit():
            ta = submit(pool, s["items"]["A"]); pool.step(2)
            tc = submit_dpm(pool, d["C"]); td = submit_dpm(pool, d["D"]); pool.step(7); pool.step(1)
            return {"D": (d["D"], pool.pop(td)), "C": (d["C"], pool.pop(tc)), "A": (None, pool.pop(ta))}
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
                check_dpm("f32", it, o, ("warm", k))
    finally:
        pool.close()
