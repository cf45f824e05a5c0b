"""Item seeds without a GPU ("Item seeds"): the exports and their context-free refusals, the `--item_seeds` flag, the
file-to-seed mapping of a run, the samplers' seeded route and the tape-assembly helper the GPU tests build their references with.

`assembled_tape` is that helper: the `noise` argument of an ordinary batch call in which every item holds the tape of the item ALONE --
`oracle.philox_oracle.tape_item(seed_b, n_steps, C, len_b)` on the item's own length, zero behind it.  tests/test_gpu_item_seeds.py feeds
it to the existing explicit-tape paths; here it is held to `item_normals` element by element."""
import argparse
import ctypes as C

import numpy as np
import pytest

from ladiffcodec_amd import decompress, lib as L, sample, sample_ddim
from oracle import philox_oracle as P

NEW = ("ldc_sample_seeded", "ldc_decode_seeded", "ldc_decode_codes_seeded")
MASK64 = (1 << 64) - 1


def assembled_tape(seeds, n_steps, n_channels, lens, Lmax=None):
    """float64 [n_steps, B, C, Lmax]: item b = tape_item(seeds[b], n_steps, C, lens[b]) in its first lens[b] positions, 0 behind them"""
    Lmax = max(lens) if Lmax is None else int(Lmax)
    out = np.zeros((n_steps, len(seeds), n_channels, Lmax), np.float64)
    for b, (s, n) in enumerate(zip(seeds, lens)):
        out[:, b, :, :n] = P.tape_item(s, n_steps, n_channels, n)[:, 0]
    return out


def test_the_assembled_tape_is_every_item_alone():
    seeds, lens, n_ch = [3, 0xC0FFEE12_9E3779B1, MASK64], [80, 240, 160], 64
    tape = assembled_tape(seeds, 3, n_ch, lens, 240)
    assert tape.shape == (3, 3, n_ch, 240)
    for b, (s, n) in enumerate(zip(seeds, lens)):
        for j in range(3):
            assert np.array_equal(tape[j, b, :, :n], P.item_normals(s, j, n_ch, n)[0]), (b, j)
        assert not tape[:, b, :, n:].any()
    # what the old layout draws for the same key is something else: the padded length and the item's position enter it
    old = P.tape_steps(seeds[1], 3, 3, n_ch, 240, split=2, lens=lens)
    assert np.abs(old[:, 1] - tape[:, 1]).max() > 1.0 and np.abs(old[:, 0, :, :80] - assembled_tape([seeds[1]], 3, n_ch, [80])[:, 0]).max() > 1.0
    # a rectangular batch: item 0 of the first part is the one item whose batch-position layout IS the item-alone layout
    rect = P.tape_steps(seeds[0], 2, 3, n_ch, 80, split=2)
    assert np.array_equal(rect[:, 0], assembled_tape([seeds[0]], 2, n_ch, [80])[:, 0])


def test_exports_and_signatures_reach_the_binding():
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    u64p = C.POINTER(C.c_uint64)
    assert len(lib.ldc_sample_seeded.argtypes) == 12 and lib.ldc_sample_seeded.argtypes[7] is u64p
    assert len(lib.ldc_decode_seeded.argtypes) == 15 and lib.ldc_decode_seeded.argtypes[9] is u64p
    assert len(lib.ldc_decode_codes_seeded.argtypes) == 18 and lib.ldc_decode_codes_seeded.argtypes[13] is u64p
    header = open(L.os.path.join(L._HERE, "..", "include", "ladiffcodec.h")).read()
    integ = open(L.os.path.join(L._HERE, "..", "INTEGRATION.md")).read()
    for name in NEW:
        assert f"int {name}(" in header and name in integ, name


def calls(sampler, seeds):
    lib = L.load()
    return (lib.ldc_sample_seeded(None, None, None, sampler, 40, 6, 1.0, seeds, 3, 80, 8, None),
            lib.ldc_decode_seeded(None, None, None, 3, 2560, sampler, 40, 6, 1.0, seeds, None, None, None, None, None),
            lib.ldc_decode_codes_seeded(None, None, None, 0, 10, 6, 3, 8, None, sampler, 40, 6, 1.0, seeds, None, None, None, None))


def test_context_free_refusals_name_the_value():
    lib = L.load()
    seeds = (C.c_uint64 * 3)(1, 2, 3)
    for sampler in (2, -1, 7):                                    # DPM-Solver++ and nonsense: there is nothing to seed
        for rc in calls(sampler, seeds):
            assert rc == L.E_INVALID
            assert f"sampler {sampler}" in lib.ldc_last_error().decode()
    for sampler in (0, 1):
        for rc in calls(sampler, None):
            assert rc == L.E_INVALID
            assert "seeds NULL" in lib.ldc_last_error().decode()
        for rc in calls(sampler, seeds):                          # past the two: the null context is what is refused next
            assert rc != 0 and "seeds" not in lib.ldc_last_error().decode()


@pytest.mark.parametrize("mod", [sample, sample_ddim, decompress])
def test_the_flag_parses_and_is_absent_by_default(mod):
    p = mod.build_parser()
    assert not hasattr(p.parse_args([]), "item_seeds")
    a = p.parse_args(["--item_seeds"])
    assert a.item_seeds is True and sample.item_seeds_option(a)
    assert not sample.item_seeds_option(p.parse_args([]))
    assert sample.item_seeds_option(p.parse_args(["--item_seeds", "--ragged"]))
    with pytest.raises(SystemExit) as ei:
        sample.item_seeds_option(p.parse_args(["--item_seeds", "--chunk_sec", "2.4"]))
    assert "--chunk_sec" in str(ei.value)
    # a namespace from before the flag existed (and a bare one) reads as "off"
    assert not sample.item_seeds_option(argparse.Namespace())


@pytest.mark.parametrize("seed", [0, 7, MASK64 - 2])
def test_file_to_seed_mapping_over_a_sharded_ragged_packed_list(seed):
    """Whatever rank and batch a file lands in, under --ragged packing or equal-length batches, its seed is (seed + its index in the
    run's file list) mod 2^64 -- the index decode_files keeps through its trims (`keep`) and decompress through its passes."""
    q = 2560
    rng = np.random.default_rng(5)
    lengths = [int(rng.integers(1, 9)) * q + int(rng.integers(0, q)) for _ in range(23)]
    run_of = [i for i in range(len(lengths)) if i % 5 != 3]          # the files a run keeps (e.g. behind decode_files' 640-sample trim)
    kept = [lengths[i] for i in run_of]
    want = {i: (seed + i) % (1 << 64) for i in run_of}
    for world in (1, 2, 3):
        for plan in ("ragged", "equal"):
            got = {}
            for rank in range(world):
                if plan == "ragged":
                    work = sample.plan_ragged_batches(kept, [1] * len(kept), rank, world, 4, 0.25, q)
                else:
                    work = sample.plan_batches(kept, [1] * len(kept), rank, world, 4)
                for idxs, joint in work:
                    assert not joint
                    for i, s in zip(idxs, sample.item_seeds_for(seed, [run_of[i] for i in idxs])):
                        assert run_of[i] not in got                 # one writer, one seed
                        got[run_of[i]] = s
            assert got == want, (world, plan)
    assert all(0 <= s < (1 << 64) for s in want.values())


class FakeEngine:
    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.log.append((name, a, kw))
            return name
        return call


def test_samplers_carry_the_seeded_route_and_leave_the_unseeded_one_alone():
    wav, seeds = object(), [4, 5]
    rb = sample.RaggedBatch(wav, [5120, 2560])
    e = FakeEngine()
    sample.DdpmSampler(6)(e, wav, None, True, seeds=seeds)
    sample.DdpmSampler(6)(e, rb, None, True, seeds=seeds)
    sample.DdimSampler(40, 6, 1.0)(e, rb, None, True, want_stages=True, seeds=seeds)
    assert e.log == [
        ("decode_seeded", (wav, seeds, 6), dict(lengths=None, want_stages=False)),
        ("decode_seeded", (wav, seeds, 6), dict(lengths=[5120, 2560], want_stages=False)),
        ("decode_seeded", (wav, seeds, 6), dict(lengths=[5120, 2560], sampler="ddim", t_start=40, eta=1.0, want_stages=True))]
    e = FakeEngine()
    cb = sample.CodesBatch(packed="rows", n_q=6, F=16)
    rcb = sample.RaggedCodesBatch("rows", 6, [16, 8])
    sample.CodesSampler(sample.DdpmSampler(6))(e, cb, None, True, seeds=seeds)
    sample.CodesSampler(sample.DdimSampler(40, 6, 0.5))(e, rcb, None, True, seeds=seeds)
    assert e.log == [
        ("decode_codes_seeded", (seeds,), dict(codes=None, packed="rows", lengths=None, bits=10, n_q=6, F=16, n_steps=6, sampler="ddpm",
                                               t_start=0, eta=0.0, want_stages=False)),
        ("decode_codes_seeded", (seeds,), dict(codes=None, packed="rows", lengths=[16, 8], bits=10, n_q=6, F=None, n_steps=6, sampler="ddim",
                                               t_start=40, eta=0.5, want_stages=False))]
    for dpm in (sample.DpmSampler(40, 6), sample.CodesSampler(sample.DpmSampler(40, 6))):
        with pytest.raises(SystemExit) as ei:
            dpm(FakeEngine(), cb, None, True, seeds=seeds)
        assert "nothing to seed" in str(ei.value)
    # without seeds the calls are argument for argument what they were
    e = FakeEngine()
    assert sample.decode_with_retry(e, wav, 6, "tape", True) == "decode"
    assert sample.decode_with_retry(e, wav, 6, "tape", True, sample.DdimSampler(40, 6, 1.0)) == "decode_ddim"
    assert sample.decode_with_retry(e, rb, 6, None, True, sample.DdpmSampler(6)) == "decode_ragged"
    assert sample.decode_with_retry(e, wav, 6, None, True, seeds=seeds) == "decode_seeded"
    assert e.log[:3] == [
        ("decode", (wav, 6), dict(noise="tape", per_item=True)),
        ("decode_ddim", (wav, 40, 6, 1.0), dict(noise="tape", per_item=True, want_stages=False)),
        ("decode_ragged", (wav, [5120, 2560], 6), dict(noise=None, want_stages=False))]
