"""DDIM items in decode pools without a GPU: the export, the binding and the prototype of ldc_pool_admit_ddim, the refusals that come
before any GPU work, and the bookkeeping of `DecodePool.submit(t_start=..., eta=...)` on a stub engine that has both admit methods."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import pytest

from ladiffcodec_amd import lib as L
from ladiffcodec_amd.model import DecodePool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.LIB_PATH


def test_admit_ddim_is_exported_bound_and_declared(built):
    dll = ctypes.CDLL(built)
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "ladiffcodec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    s = "ldc_pool_admit_ddim"
    assert hasattr(dll, s) and s in L.EXPORTS
    assert re.search(r"\bint\s+" + s + r"\s*\(", text), f"{s} is not declared in include/ladiffcodec.h"
    at = lib.ldc_pool_admit_ddim.argtypes
    assert len(at) == 12 and at[10] is ctypes.c_uint64 and at[8] is ctypes.c_float


def test_admit_ddim_refuses_a_null_context(built):
    lib = L.load()
    assert lib.ldc_pool_admit_ddim(None, None, 0, None, None, 32, 40, 8, 0.0, None, 0, None) == L.E_INVALID
    assert "null pointer" in lib.ldc_last_error().decode()


@pytest.mark.parametrize("bad", [dict(eta=-0.1), dict(eta=1.5), dict(eta=math.nan), dict(eta=math.inf), dict(S=11), dict(S=0),
                                 dict(t_start=0), dict(t_start=1001)])
def test_admit_ddim_refuses_bad_schedules_before_any_gpu_work(built, bad):
    a = dict(t_start=10, S=10, eta=0.0)
    a.update(bad)
    rc = L.load().ldc_pool_admit_ddim(None, None, 0, None, None, 32, a["t_start"], a["S"], a["eta"], None, 0, None)
    assert rc == L.E_INVALID


class StubEngine:
    """tests/test_pool_cpu.py's stub with the second admit method: a host-side model of ldc_pool_remaining"""

    def __init__(self, hop=32):
        self.main_codec = SimpleNamespace(hop_length=hop, rep_dims=128)
        self.rem, self.ddpm, self.ddim = None, [], []

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

    def pool_step(self, h, n):
        self.rem = [max(0, r - n) if r > 0 else r for r in self.rem]

    def pool_take(self, h, slot, Lz, keep=False):
        assert self.rem[slot] == 0
        if not keep:
            self.rem[slot] = -1
        return ("latents", slot, Lz)

    def pool_back(self, lat):
        return ("wav",) + lat[1:]


def test_submit_routes_by_t_start_on_a_stub_engine():
    eng = StubEngine()
    pool = DecodePool(eng, 4, 160 * 32)
    a = pool.submit(wav=96, n_steps=10)                                 # DDPM: pool_admit with the old positional arguments
    b = pool.submit(wav=32, n_steps=8, t_start=40, eta=0.5, noise="tape")
    c = pool.submit(codes=64, n_steps=4, t_start=25, seed=77)
    d = pool.submit(wav=64, n_steps=3, t_start=0, eta=0.9)              # t_start 0 is DDPM whatever eta says
    assert (a, b, c, d) == (0, 1, 2, 3)
    assert eng.ddpm == [(0, 96, 10, None, 0), (3, 64, 3, None, 3)]      # the seed defaults to the ticket
    assert eng.ddim == [(1, 32, 40, 8, 0.5, "tape", 1), (2, 64, 25, 4, 0.0, None, 77)]
    assert pool._info[b] == (32, "tape")                                # the tape is kept alive with the ticket
    assert pool.remaining() == [10, 8, 4, 3]                            # iterations for the DDIM items, not timesteps
    pool.step(4)
    assert pool.finished() == [c, d] and pool.remaining() == [6, 4, 0, 0]
    assert pool.pop(c) == {"wav": ("wav", 2, 64), "latents": ("latents", 2, 64)}
    e = pool.submit(wav=32, n_steps=2, t_start=6, eta=1.0)              # a DDIM item into the slot a DDIM item left
    assert eng.ddim[-1] == (2, 32, 6, 2, 1.0, None, e)
    pool.run_until_done()
    assert pool.finished() == [a, b, d, e]
    pool.close()


def test_open_pool_points_to_submit_for_another_sampler():
    from ladiffcodec_amd.model import Engine
    with pytest.raises(ValueError, match=r"submit\(t_start="):
        Engine.open_pool(None, 4, 5120, sampler="ddim")
