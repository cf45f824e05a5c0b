"""Decode pools without a GPU: the exports, the bindings, the prototypes, the refusals that come before any GPU work, and the
bookkeeping of `DecodePool` driven by a stub engine (tickets map to slots, a popped slot is reused, `submit` raises when the pool
is full, `finished()` follows the remaining counts)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from ladiffcodec_amd import lib as L
from ladiffcodec_amd.model import DecodePool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ldc_unet_forward_items", "ldc_pool_create", "ldc_pool_destroy", "ldc_pool_admit", "ldc_pool_step", "ldc_pool_remaining",
           "ldc_pool_take", "ldc_pool_peek", "ldc_pool_evict"]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.LIB_PATH


def test_pool_symbols_are_exported_bound_and_declared(built):
    dll = ctypes.CDLL(built)
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "ladiffcodec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert hasattr(dll, s), f"{s} is not exported"
        assert s in L.EXPORTS
        assert getattr(lib, s).argtypes, f"{s} has no argtypes in lib.py"
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), f"{s} is not declared in include/ladiffcodec.h"
    assert "typedef struct ldc_pool ldc_pool;" in text
    assert len(lib.ldc_pool_admit.argtypes) == 10 and lib.ldc_pool_admit.argtypes[8] is ctypes.c_uint64
    assert len(lib.ldc_unet_forward_items.argtypes) == 10


def test_pool_calls_refuse_null_pointers_before_any_gpu_work(built):
    lib = L.load()
    out = ctypes.c_void_p()
    rem = (ctypes.c_int32 * 4)()
    for rc in (lib.ldc_pool_create(None, 4, 160, ctypes.byref(out)), lib.ldc_pool_admit(None, None, 0, None, None, 32, 4, None, 0, None),
               lib.ldc_pool_step(None, None, 1, None), lib.ldc_pool_take(None, None, 0, None, None), lib.ldc_pool_peek(None, None, 0, None, None),
               lib.ldc_pool_evict(None, 0), lib.ldc_pool_remaining(None, rem),
               lib.ldc_unet_forward_items(None, None, None, None, None, 2, 160, 16, None, None)):
        assert rc == L.E_INVALID
        assert "null pointer" in lib.ldc_last_error().decode()
    assert lib.ldc_pool_destroy(None) == 0


class StubEngine:
    """what DecodePool needs of an engine: the pool_* methods over a host-side model of ldc_pool_remaining"""

    def __init__(self, hop=32):
        self.main_codec = SimpleNamespace(hop_length=hop, rep_dims=128)
        self.rem, self.admitted, self.destroyed = None, [], False

    def pool_create(self, slots, Lmax):
        self.rem, self.Lmax = [-1] * slots, Lmax
        return "pool"

    def pool_destroy(self, h):
        self.destroyed = True

    def pool_remaining(self, h, slots):
        return list(self.rem)

    def pool_front(self, wav=None, codes=None):
        n = wav if wav is not None else codes
        return SimpleNamespace(shape=(1, 128, n)), SimpleNamespace(shape=(1, 128, n // 10))

    def pool_admit(self, h, slot, img, cond, n_steps, noise=None, seed=0):
        assert self.rem[slot] < 0
        self.rem[slot] = n_steps
        self.admitted.append((slot, img.shape[-1], n_steps, seed))
        return noise

    def pool_step(self, h, n):
        assert n > 0
        self.rem = [max(0, r - n) if r > 0 else r for r in self.rem]

    def pool_take(self, h, slot, Lz, keep=False):
        assert self.rem[slot] == 0
        if not keep:
            self.rem[slot] = -1
        return ("latents", slot, Lz)

    def pool_evict(self, h, slot):
        self.rem[slot] = -1

    def pool_back(self, lat):
        return ("wav",) + lat[1:]


def test_decode_pool_bookkeeping_on_a_stub_engine():
    eng = StubEngine()
    with pytest.raises(ValueError):
        DecodePool(eng, 2, 1000)                       # not a multiple of the hop
    pool = DecodePool(eng, 3, 160 * 32)
    assert pool.Lmax == 160 and pool.free_slots() == [0, 1, 2] and pool.finished() == []
    a = pool.submit(wav=96, n_steps=5)
    b = pool.submit(wav=32, n_steps=2, seed=77)
    c = pool.submit(codes=160, n_steps=9)
    assert (a, b, c) == (0, 1, 2) and [x[0] for x in eng.admitted] == [0, 1, 2]
    assert eng.admitted[0][3] == 0 and eng.admitted[1][3] == 77       # the seed defaults to the ticket
    with pytest.raises(RuntimeError, match="no free slot"):
        pool.submit(wav=32, n_steps=1)
    pool.step(2)
    assert pool.finished() == [b] and pool.running() == [a, c] and pool.remaining() == [3, 0, 7]
    assert pool.peek(b) == ("latents", 1, 32) and pool.finished() == [b]
    out = pool.pop(b)
    assert out == {"wav": ("wav", 1, 32), "latents": ("latents", 1, 32)}
    with pytest.raises(KeyError):
        pool.pop(b)
    d = pool.submit(wav=64, n_steps=4)                 # the popped slot is reused; tickets are never reused
    assert d == 3 and eng.admitted[-1][0] == 1
    pool.step(3)
    assert pool.finished() == [a]
    pool.run_until_done()                              # to the next finisher each time: d after 1, c after 3 more
    assert pool.finished() == [a, c, d] and pool.running() == []
    pool.evict(c)
    assert pool.finished() == [a, d] and pool.free_slots() == [2]
    for t in (a, d):
        pool.pop(t)
    assert pool.free_slots() == [0, 1, 2]
    pool.close()
    assert eng.destroyed
    pool.close()                                       # idempotent
