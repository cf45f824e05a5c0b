"""A timestep per item and the decode pool on the GPU.  References are the CPU oracle's SOLO results (every item alone, at its own
timestep / with its own tape and step count), never the engine under test -- except the Philox checks here, which compare with the
engine's own unchanged B = 1 path; tests/test_gpu_noise.py ties both, the pool item and the B = 1 path, to the oracle's exact Philox
(oracle/philox_oracle.py).

Items: the four lengths of tests/test_gpu_ragged.py (3, 1, 5, 2 quanta for `r84`, the same sample counts for `r8`) cut from the same
waveforms, plus a fifth item E (5120 samples) that enters the slot B leaves.  n_steps 10, 6, 10, 4, 7.

Waveform bar: the pool's plan is the ragged plan (the same unfused launch forms rounding the same way), so the bar is the ragged
waveform bar of tests/test_gpu_ragged.py, quoted here: max(2 x 8.1e-4, TOL) = 1.62e-3 for bf16, and the f32 `wav_small` bar 1e-5.
Every check prints its figure before it asserts; if a pool waveform recorded on MI355X exceeds the ragged figure (8.1e-4), this file
gets a POOL_MEASURED of its own and asserts 2x that."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, sample, synth  # noqa: E402
from ladiffcodec_amd.model import _DiffModel  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from drift_tolerances import TOL, check  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402

QUANTA = {"r84": (3, 1, 5, 2), "r8": (12, 4, 20, 8)}
STEPS = {"A": 10, "B": 6, "C": 10, "D": 4, "E": 7}
T_ITEMS = (37, 499, 0, 999)
WAV_BAR = {"bf16": 1.62e-3, "f32": 1e-5}          # the ragged waveform bar (see above)
_CACHE = {}


def setup(tag):
    """the five items (waveform, tape, the oracle's solo decode) and the UNet inputs of check 1 with the oracle's solo eps"""
    if tag in _CACHE:
        return _CACHE[tag]
    mc, u, _ = CASES[tag]
    q = sample.chunk_quantum(mc.enc_ratios)
    lens = [k * q for k in QUANTA[tag]] + [5120]
    Tmax, hop = max(lens), mc.hop_length
    src = torch.from_numpy(synth.synthetic_wav(4, Tmax, seed=71)) * 0.5
    sdc, sdm = synth.to_torch(cond_sd_np()), synth.to_torch(main_sd_np(tag))
    items = {}
    g = torch.Generator().manual_seed(23)
    for k, (name, n) in enumerate(zip("ABCDE", lens)):
        wav = src[k % 4:k % 4 + 1, :, :n].contiguous()          # (E: a prefix of A's waveform)
        tape = torch.randn(STEPS[name], 1, 128, n // hop, generator=g)
        ref = O.decode_utterances(sdc, COND_CFG, sdm, mc, u, wav, STEPS[name], tape, per_item=True)
        items[name] = dict(wav=wav, tape=tape, n=n, steps=STEPS[name], ref=ref)
    up = int(np.prod(u.upsampling_ratios))
    Lmax = max(lens[:4]) // hop
    llens = [n // hop for n in lens[:4]]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 128, Lmax, generator=g)
    cond = torch.randn(4, 128, Lmax // up, generator=g)

    def solo(b, t):
        n = llens[b]
        return O.unet_forward(sdm, u, x[b:b + 1, :, :n].contiguous(), torch.full((1,), t, dtype=torch.long),
                              cond[b:b + 1, :, :n // up].contiguous())
    eps = [solo(b, t) for b, t in enumerate(T_ITEMS)]
    swapped = [solo(0, T_ITEMS[1]), solo(1, T_ITEMS[0])]        # item 0 at item 1's t and the reverse: the sensitivity references
    _CACHE[tag] = dict(mc=mc, u=u, q=q, Tmax=Tmax, hop=hop, up=up, items=items, x=x, cond=cond, llens=llens, Lmax=Lmax, eps=eps,
                       swapped=swapped, sdm=sdm)
    return _CACHE[tag]


def check_item(dtype, it, out, what):
    lat = rel(out["latents"].cpu().numpy(), it["ref"]["latents"].numpy())
    wav = rel(out["wav"].cpu().numpy(), it["ref"]["wav"].numpy())
    print(f"pool {dtype} {what}: latents {lat:.3e} (bar {TOL[dtype]['chain_small']:.3e}), wav {wav:.3e} (bar {WAV_BAR[dtype]:.3e})")
    assert tuple(out["wav"].shape) == (1, 1, it["n"])
    check(dtype, "chain_small", lat, (what, "latents"))
    assert wav < WAV_BAR[dtype], (dtype, what, "wav", wav, WAV_BAR[dtype])


def submit(pool, it, **kw):
    return pool.submit(wav=it["wav"].cuda(), n_steps=it["steps"], noise=it["tape"].cuda(), **kw)


def run_schedule(pool, s, dtype, what=""):
    """the staggered schedule of check 2 on a 4-slot pool; every item against the oracle's solo halfway sampling of it"""
    it = s["items"]
    t = {}
    t["A"] = submit(pool, it["A"]); pool.step(3)
    t["B"] = submit(pool, it["B"]); t["C"] = submit(pool, it["C"]); pool.step(1); pool.step(4)
    t["D"] = submit(pool, it["D"])                               # the last free slot
    assert pool.free_slots() == []
    pool.step(2)
    assert t["B"] in pool.finished() and t["C"] in pool.running() and t["D"] in pool.running()
    slot_b = pool._slot_of[t["B"]]
    out = {"B": pool.pop(t["B"])}
    t["E"] = submit(pool, it["E"])                               # into B's slot while C and D are mid-flight (A waits, finished)
    assert pool._slot_of[t["E"]] == slot_b
    pool.step(1); pool.step(7)
    assert pool.running() == [] and sorted(pool.finished()) == sorted(t[k] for k in "ACDE")
    for k in "ACDE":
        out[k] = pool.pop(t[k])
    assert pool.free_slots() == [0, 1, 2, 3]
    for k in "ABCDE":
        check_item(dtype, it[k], out[k], (what, k))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_unet_forward_items(tag, dtype):
    s = setup(tag)
    e = engine(tag, dtype)
    bar = TOL[dtype]["eps_small"]
    x, cond, llens = s["x"].cuda(), s["cond"].cuda(), s["llens"]
    got = e.unet_forward_items(x, T_ITEMS, cond, llens).cpu()
    for b, n in enumerate(llens):
        err = rel(got[b:b + 1, :, :n].numpy(), s["eps"][b].numpy())
        print(f"items {tag} {dtype} item {b} t {T_ITEMS[b]}: {err:.3e} (bar {bar:.3e})")
        check(dtype, "eps_small", err, (tag, b, "oracle solo at its own t"))
        assert not got[b, :, n:].any(), ("eps beyond the length", b)
    # a shared timestep cannot pass: each of items 0 and 1 misses the oracle at the OTHER's timestep by more than twice the bar
    for b in (0, 1):
        miss = rel(got[b:b + 1, :, :llens[b]].numpy(), s["swapped"][b].numpy())
        print(f"items {tag} {dtype} item {b} against t {T_ITEMS[1 - b]}: {miss:.3e}")
        assert miss > 2 * bar, (tag, dtype, b, miss)
    same = e.unet_forward_items(x, [37] * 4, cond, llens).cpu()
    rag = e.unet_forward_ragged(x, 37, cond, llens).cpu()
    for b, n in enumerate(llens):
        check(dtype, "eps_small", rel(same[b:b + 1, :, :n].numpy(), rag[b:b + 1, :, :n].numpy()), (tag, b, "equal t against the ragged plan"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["r84", "r8"])
def test_staggered_pool(tag, dtype):
    s = setup(tag)
    pool = engine(tag, dtype).open_pool(4, s["Tmax"])
    try:
        run_schedule(pool, s, dtype, tag)
    finally:
        pool.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_idle_slots_keep_their_latents(dtype):
    s = setup("r84")
    e = engine("r84", dtype)
    it = s["items"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        # C among three others in a full pool: A (its tape) and B (Philox) run all ten of C's steps, D its four and then waits finished
        tape = it["D"]["tape"].cuda()
        td = pool.submit(wav=it["D"]["wav"].cuda(), n_steps=4, noise=tape)
        ta = submit(pool, it["A"])
        tb = pool.submit(wav=it["B"]["wav"].cuda(), n_steps=10, seed=7)
        tc = submit(pool, it["C"])
        assert pool.free_slots() == []
        pool.step(4)
        assert pool.finished() == [td] and pool.running() == [ta, tb, tc]
        first = pool.peek(td).clone()
        torch.cuda.synchronize()
        nbytes = tape.numel()
        del tape
        pool._info[td] = (pool._info[td][0], None)               # the pool's own reference to the tape
        junk = torch.full((nbytes,), float("nan"), device="cuda")  # the allocator hands the tape's block out again
        pool.step(5)
        again = pool.peek(td)
        assert torch.equal(first, again), "a finished item's latents moved while it waited"
        del junk
        pool.run_until_done()
        check_item(dtype, it["D"], pool.pop(td), "D after waiting")
        check_item(dtype, it["A"], pool.pop(ta), "A in the full pool")
        assert torch.isfinite(pool.pop(tb)["latents"]).all()
        among = pool.pop(tc)["latents"].cpu()
        check(dtype, "chain_small", rel(among.numpy(), it["C"]["ref"]["latents"].numpy()), "C among three others")
        if dtype == "f32":                                       # the same item alone in the pool: three free slots
            t = submit(pool, it["C"])
            assert len(pool.free_slots()) == 3
            pool.run_until_done()
            alone = pool.pop(t)["latents"].cpu()
            err = rel(among.numpy(), alone.numpy())
            print(f"pool f32 C alone against C among three others (A, B, D): {err:.3e} (bar 1e-5)")
            assert err < 1e-5
    finally:
        pool.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_philox_items_draw_what_they_draw_alone(dtype):
    s = setup("r84")
    e = engine("r84", dtype)
    it = s["items"]["D"]
    bar = TOL[dtype]["chain_small"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        other = submit(pool, s["items"]["A"])                    # company in another slot, already three steps in
        pool.step(3)
        t1 = pool.submit(wav=it["wav"].cuda(), n_steps=6, seed=1234)
        t2 = pool.submit(wav=it["wav"].cuda(), n_steps=6, seed=99)
        pool.run_until_done()
        a, b = pool.pop(t1)["latents"].cpu(), pool.pop(t2)["latents"].cpu()
        img, cond = e.pool_front(wav=it["wav"].cuda())
        e.reseed(1234)
        solo = e.denoise(img, cond, 6).cpu()
        err, apart = rel(a.numpy(), solo.numpy()), rel(b.numpy(), a.numpy())
        print(f"pool {dtype} Philox against the solo path: {err:.3e} (bar {bar:.3e}); two seeds apart: {apart:.3e}")
        assert err < bar and apart > 10 * bar
        pool.evict(other)
    finally:
        pool.close()


def test_refusals_leave_the_pool_usable():
    s = setup("r84")
    e, other = engine("r84", "f32"), engine("r84", "bf16")
    lib, it = L.load(), s["items"]
    T = 1000                                                      # timesteps of the schedule
    pool = e.open_pool(4, s["Tmax"])

    def refused(code, fn, *names):
        with pytest.raises(L.LdcError) as ei:
            fn()
        assert ei.value.code == code, (names, str(ei.value))
        for n in names:
            assert str(n) in str(ei.value), (n, str(ei.value))
    try:
        img, cond = e.pool_front(wav=it["D"]["wav"].cuda())
        Ld = img.shape[-1]
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, 4, img, cond, 4), "slot 4")
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, -1, img, cond, 4), "slot -1")
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, 0, img[..., :Ld - 1].contiguous(), cond, 4), Ld - 1)      # off the quantum
        big = torch.zeros(1, 128, s["Lmax"] + Ld, device="cuda")
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, 0, big, cond, 4), s["Lmax"] + Ld)                         # above Lmax
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, 0, img, cond, 0), "n_steps = 0")
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, 0, img, cond, T + 1), f"n_steps = {T + 1}")
        refused(L.E_INVALID, lambda: e.pool_step(pool._h, 0), "n = 0")
        refused(L.E_INVALID, lambda: e.pool_step(pool._h, -3), "n = -3")
        refused(L.E_INVALID, lambda: e.open_pool(0, s["Tmax"]), "slots = 0")
        refused(L.E_INVALID, lambda: e.open_pool(4, s["Tmax"] + s["hop"]), s["Lmax"] + 1)                            # Lmax off the quantum
        refused(L.E_INVALID, lambda: other.pool_step(pool._h, 1), "another context")
        refused(L.E_INVALID, lambda: L.check(lib.ldc_pool_admit(e._ctx, pool._h, 0, None, cond.data_ptr(), Ld, 4, None, 0, None)), "null pointer")
        refused(L.E_INVALID, lambda: L.check(lib.ldc_pool_take(e._ctx, pool._h, 0, None, None)), "null pointer")
        refused(L.E_STATE, lambda: e.pool_take(pool._h, 0, Ld), "slot 0", "free")
        t = pool.submit(wav=it["D"]["wav"].cuda(), n_steps=4, noise=it["D"]["tape"].cuda())
        refused(L.E_INVALID, lambda: e.pool_admit(pool._h, 0, img, cond, 4), "slot 0 is not free")
        pool.step(1)
        refused(L.E_STATE, lambda: e.pool_take(pool._h, 0, Ld), "slot 0", "running")
        x, c = s["x"].cuda(), s["cond"].cuda()
        refused(L.E_INVALID, lambda: e.unet_forward_items(x, (37, 1000, 0, 999), c, s["llens"]), "t_host[1] = 1000")
        refused(L.E_INVALID, lambda: e.unet_forward_items(x, (37, 499, -1, 999), c, s["llens"]), "t_host[2] = -1")
        rem = pool.remaining()
        assert rem == [3, -1, -1, -1]                             # the refusals moved nothing
        pool.run_until_done()
        check_item("f32", it["D"], pool.pop(t), "D after the refusals")
        run_schedule(pool, s, "f32", "after refusals")
    finally:
        pool.close()


def test_the_fp8_engine_refuses():
    s = setup("r84")
    e = engine("r84", "fp8")
    with pytest.raises(L.LdcError) as ei:
        e.open_pool(4, s["Tmax"])
    assert ei.value.code == L.E_INVALID and "fp8" in str(ei.value)
    with pytest.raises(L.LdcError) as ei:
        e.unet_forward_items(s["x"].cuda(), T_ITEMS, s["cond"].cuda(), s["llens"])
    assert ei.value.code == L.E_INVALID and "fp8" in str(ei.value)
    with pytest.raises(ValueError):
        e.open_pool(4, s["Tmax"], sampler="ddim")                # DDIM in a pool is refused, not approximated


def test_warm_pool_calls_never_wait_for_the_device():
    s = setup("r84")
    e = engine("r84", "f32")
    it = s["items"]
    pool = e.open_pool(4, s["Tmax"])
    try:
        def visit():
            ta = submit(pool, it["A"]); pool.step(2)
            td = submit(pool, it["D"]); pool.step(7); pool.step(1)
            return {"D": pool.pop(td), "A": pool.pop(ta)}
        visit()                                                  # plans built, graphs captured (5-step and single-step), codec ends warm
        torch.cuda.synchronize()
        before = L.load().ldc_debug_sync_count()
        outs = visit()
        torch.cuda.synchronize()
        assert L.load().ldc_debug_sync_count() == before
        for k, o in outs.items():
            check_item("f32", it[k], o, ("warm", k))
    finally:
        pool.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_diff_model_routes_a_mixed_time_tensor(dtype):
    s = setup("r84")
    e = engine("r84", dtype)
    u, up = s["u"], s["up"]
    n = s["llens"][3]                                            # equal lengths here: the facade has no lengths argument
    x, cond = s["x"][:, :, :n].contiguous(), s["cond"][:, :, :n // up].contiguous()
    model = _DiffModel(e)
    time = torch.tensor(T_ITEMS, dtype=torch.long)
    got = model(x.cuda(), time.cuda(), cond.cuda()).cpu()
    ref = O.unet_forward(s["sdm"], u, x, time, cond)              # the oracle takes a timestep per item too
    for b in range(4):
        check(dtype, "eps_small", rel(got[b:b + 1].numpy(), ref[b:b + 1].numpy()), ("facade", b))
    # routed to one shared timestep it could not pass: item 1 (t = 499) misses the oracle at item 0's timestep (37) by more than twice the
    # bar (on the oracle the two differ by 0.170 of the maximum here: at least 0.170 - bar = 0.128 > 2 x 0.042 is left for a bf16 result)
    miss = rel(got[1:2].numpy(), O.unet_forward(s["sdm"], u, x[1:2], time[0:1], cond[1:2]).numpy())
    assert miss > 2 * TOL[dtype]["eps_small"], (dtype, miss)
    # The same call made directly.  Two passes of one plan differ by the order in which the GroupNorm statistics are summed (atomics), and
    # eps leaves the UNet in the engine's storage format: in bf16 a value that moves at all moves by an ulp, 2^-8 of itself (3.9e-3 of the
    # maximum), so no bar below that can hold.  The bar is the one check 1 uses between two plans of the same launch forms, eps_small.
    direct = e.unet_forward_items(x.cuda(), T_ITEMS, cond.cuda()).cpu()
    err = rel(got.numpy(), direct.numpy())
    print(f"facade {dtype} against the direct call: {err:.3e} (bar {TOL[dtype]['eps_small']:.3e})")
    check(dtype, "eps_small", err, "facade against the direct call")
    same = model(x.cuda(), torch.full((4,), 37, dtype=torch.long), cond.cuda()).cpu()      # equal entries keep the one-t path
    check(dtype, "eps_small", rel(same.numpy(), e.unet_forward(x.cuda(), 37, cond.cuda()).cpu().numpy()), "equal entries")
