"""DPM-Solver++(2M) items in decode pools without a GPU: the export, the binding and the prototype of ldc_pool_admit_dpm, the refusals
that come before any GPU work, the bookkeeping of `DecodePool.submit(sampler="dpm")` on a stub engine with the three admit methods, and
the discrimination check of tests/test_gpu_pool_dpm.py's items: on the restatement (tests/dpm_restatement.py, CPU oracle, dim-32
fixture `r84`) each of `three`, `C` and `D` is more than 10 x the f32 latents bar away from the same run without its `b1` term and from
the same run fed another item's x0 history at iteration 1, so a pool that made either mistake could not pass the GPU test."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ladiffcodec_amd import lib as L
from ladiffcodec_amd.model import DecodePool
from drift_tolerances import TOL
import dpm_restatement as R
import pool_dpm_items as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.LIB_PATH


def test_admit_dpm_is_exported_bound_and_declared(built):
    dll = ctypes.CDLL(built)
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "ladiffcodec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    s = "ldc_pool_admit_dpm"
    assert hasattr(dll, s) and s in L.EXPORTS
    m = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)", text)
    assert m, f"{s} is not declared in include/ladiffcodec.h"
    assert len(m.group(1).split(",")) == 9, m.group(1)
    at = lib.ldc_pool_admit_dpm.argtypes
    assert len(at) == 9 and at[6] is ctypes.c_int32 and at[7] is ctypes.c_int32 and at[8] is ctypes.c_void_p
    assert not any(a in (ctypes.c_float, ctypes.c_uint64) for a in at), "a DPM item has no eta and no seed"


def test_admit_dpm_refuses_a_null_context(built):
    lib = L.load()
    assert lib.ldc_pool_admit_dpm(None, None, 0, None, None, 32, 40, 8, None) == L.E_INVALID
    assert "null pointer" in lib.ldc_last_error().decode()


@pytest.mark.parametrize("t_start,S", [(0, 1), (1001, 8), (10, 0), (10, 11)])
def test_admit_dpm_refuses_bad_schedules_before_any_gpu_work(built, t_start, S):
    assert L.load().ldc_pool_admit_dpm(None, None, 0, None, None, 32, t_start, S, None) == L.E_INVALID


class StubEngine:
    """tests/test_pool_ddim_cpu.py's stub with the third admit method: a host-side model of ldc_pool_remaining"""

    def __init__(self, hop=32):
        self.main_codec = SimpleNamespace(hop_length=hop, rep_dims=128)
        self.rem, self.ddpm, self.ddim, self.dpm = None, [], [], []

    def pool_create(self, slots, Lmax):
        self.rem = [-1] * slots
        return "pool"

    def pool_destroy(self, h):
        pass

    def pool_remaining(self, h, slots):
        return list(self.rem)

    def pool_front(self, wav=None, codes=None):
        n = wav if wav is not None else codes
        return SimpleNamespace(shape=(1, 128, n)), SimpleNamespace(shape=(1, 128, n // 10))

    def pool_admit(self, h, slot, img, cond, n_steps, noise=None, seed=0):      # (the signature of before: no sampler argument)
        self.rem[slot] = n_steps
        self.ddpm.append((slot, img.shape[-1], n_steps, noise, seed))
        return noise

    def pool_admit_ddim(self, h, slot, img, cond, t_start, n_steps, eta, noise=None, seed=0):
        self.rem[slot] = n_steps
        self.ddim.append((slot, img.shape[-1], t_start, n_steps, eta, noise, seed))
        return noise

    def pool_admit_dpm(self, h, slot, img, cond, t_start, n_steps):            # nothing is drawn: no noise, no seed, no eta
        self.rem[slot] = n_steps
        self.dpm.append((slot, img.shape[-1], t_start, n_steps))

    def pool_step(self, h, n):
        self.rem = [max(0, r - n) if r > 0 else r for r in self.rem]

    def pool_take(self, h, slot, Lz, keep=False):
        assert self.rem[slot] == 0
        if not keep:
            self.rem[slot] = -1
        return ("latents", slot, Lz)

    def pool_back(self, lat):
        return ("wav",) + lat[1:]


def test_submit_routes_a_dpm_item_on_a_stub_engine():
    eng = StubEngine()
    pool = DecodePool(eng, 4, 160 * 32)
    a = pool.submit(wav=96, n_steps=10)                                 # the old calls, sampler=None: by t_start
    b = pool.submit(wav=32, n_steps=4, t_start=40, eta=0.5, noise="tape")
    c = pool.submit(wav=64, n_steps=8, t_start=40, sampler="dpm")
    d = pool.submit(codes=64, n_steps=3, t_start=25, sampler="dpm")
    assert (a, b, c, d) == (0, 1, 2, 3)
    assert eng.ddpm == [(0, 96, 10, None, 0)]                           # positional arguments as before, the seed defaults to the ticket
    assert eng.ddim == [(1, 32, 40, 4, 0.5, "tape", 1)]
    assert eng.dpm == [(2, 64, 40, 8), (3, 64, 25, 3)]
    assert pool._info[c] == (64, None)                                  # no tape to keep alive
    assert pool.remaining() == [10, 4, 8, 3]                            # iterations for a DPM item, not timesteps
    pool.step(4)
    assert pool.finished() == [b, d] and pool.remaining() == [6, 0, 4, 0]
    assert pool.pop(b) == {"wav": ("wav", 1, 32), "latents": ("latents", 1, 32)}
    e = pool.submit(wav=32, n_steps=2, t_start=6, sampler="dpm")        # a DPM item into the slot a DDIM item left
    assert eng.dpm[-1] == (1, 32, 6, 2) and pool._slot_of[e] == 1
    pool.run_until_done()
    assert pool.finished() == [a, c, d, e]
    # the names of the two older routes
    pool.pop(d); pool.pop(e)
    f = pool.submit(wav=32, n_steps=5, sampler="ddpm", seed=9)
    g = pool.submit(wav=32, n_steps=5, t_start=20, eta=1.0, sampler="ddim")
    assert eng.ddpm[-1] == (1, 32, 5, None, 9) and eng.ddim[-1] == (3, 32, 20, 5, 1.0, None, g) and f == 5
    pool.close()


@pytest.mark.parametrize("kw,named", [(dict(noise="tape"), "noise"), (dict(seed=3), "seed"), (dict(eta=0.5), "eta"),
                                       (dict(t_start=0), "t_start"), (dict(sampler="heun"), "heun")])
def test_submit_dpm_refuses_what_it_would_ignore(kw, named):
    eng = StubEngine()
    pool = DecodePool(eng, 4, 160 * 32)
    a = dict(wav=64, n_steps=8, t_start=40, sampler="dpm")
    a.update(kw)
    with pytest.raises(ValueError, match=named):
        pool.submit(**a)
    assert eng.dpm == [] and eng.ddim == [] and eng.ddpm == [] and pool.remaining() == [-1] * 4 and pool._next == 0
    assert pool.submit(wav=64, n_steps=8, t_start=40, eta=0.0, sampler="dpm") == 0      # eta 0 says nothing
    pool.close()


def test_the_old_calls_are_unchanged_without_a_sampler():
    eng = StubEngine()
    pool = DecodePool(eng, 4, 160 * 32)
    pool.submit(wav=96, n_steps=10)
    pool.submit(wav=32, n_steps=8, t_start=40, eta=0.5, noise="tape")
    pool.submit(wav=64, n_steps=3, t_start=0, eta=0.9)                  # t_start 0 is DDPM whatever eta says
    assert eng.ddpm == [(0, 96, 10, None, 0), (2, 64, 3, None, 2)]
    assert eng.ddim == [(1, 32, 40, 8, 0.5, "tape", 1)] and eng.dpm == []
    pool.close()


def test_open_pool_refuses_dpm_as_a_pool_sampler():
    from ladiffcodec_amd.model import Engine
    with pytest.raises(ValueError, match=r'sampler="dpm"'):
        Engine.open_pool(None, 4, 5120, sampler="dpm")


@pytest.mark.parametrize("name,other", [("three", "C"), ("C", "D"), ("D", "three")])
def test_the_items_tell_the_mutants_apart(name, other):
    """`other`: the item whose x0 of iteration 0 sits in the slot's history when `name` reaches iteration 1"""
    sdm, u, items = P.fronts("r84")
    bar = TOL["f32"]["chain_small"]
    src, t_start, S = P.DPM[name]
    img, cond = items[src]
    own, _ = P.dpm_variant(sdm, u, img, cond, t_start, S)
    assert torch.equal(own, R.dpm_sample(sdm, u, img, cond, t_start, S)), "the unmutated variant is not the restatement"
    no_b1, _ = P.dpm_variant(sdm, u, img, cond, t_start, S, drop_b1=True)
    osrc, ot, _ = P.DPM[other]
    _, ohist = P.dpm_variant(sdm, u, items[osrc][0], items[osrc][1], ot, 1)      # (x0 of iteration 0 depends on t_start alone)
    stale, _ = P.dpm_variant(sdm, u, img, cond, t_start, S, foreign=P.stale_block(ohist[0], img.shape[-1]))
    d1, d2 = rel(no_b1.numpy(), own.numpy()), rel(stale.numpy(), own.numpy())
    print(f"restatement {name} ({t_start}, {S}): without b1 {d1:.3e}, with the x0 history of {other} at iteration 1 {d2:.3e} "
          f"(10 x bar {10 * bar:.3e})")
    assert d1 > 10 * bar and d2 > 10 * bar, (name, d1, d2)
