"""The host-only ground of coupled windows in batch parts ("Windows in parts"): ldc_window_layout_n against
ldc_window_layout and against the Python restatement beyond 32 windows, ldc_window_parts, the refusals, the part-boundary mutant on the
CPU oracle -- the discrimination condition a GPU test of a call in parts will rely on, asserted here on the reference alone --, the
segment plan at a raised cap and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from ladiffcodec_amd import lib as L, sample
from drift_tolerances import TOL
import windows_parts_restatement as WP
import windows_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(200, 80, 20), (180, 80, 40), (240, 80, 0), (81, 80, 40), (60, 80, 20), (80, 80, 40), (2560, 80, 0), (80 + 31 * 40, 80, 40)]


@pytest.mark.parametrize("triple", SMALL)
@pytest.mark.parametrize("cap", [32, 33, 64, 128])
def test_layout_n_is_the_layout_bit_for_bit_up_to_32_windows(triple, cap):
    Ltot, Lw, O_ = triple
    starts, w = L.window_layout(Ltot, Lw, O_, 1)
    lib = L.load()
    sn = (ctypes.c_int * cap)(*([-1] * cap))
    wn = np.full(w.shape, np.nan, np.float32)
    W = lib.ldc_window_layout_n(Ltot, Lw, O_, 1, cap, sn, wn.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    print(triple, "cap", cap, "->", W, "windows")
    assert W == len(starts) <= 32
    assert list(sn) == starts + [0] * (cap - W)                           # the convention of ldc_window_layout: zero behind W
    assert wn.tobytes() == w.tobytes()
    if cap != 32:
        s2, w2 = L.window_layout(Ltot, Lw, O_, 1, max_windows=cap)        # the wrapper's route through ldc_window_layout_n
        assert s2 == starts and w2.tobytes() == w.tobytes()


@pytest.mark.parametrize("W,Lw,O_", [(33, 80, 40), (64, 80, 40), (128, 80, 40), (33, 80, 20), (128, 160, 40)])
def test_layout_n_beyond_32_windows_against_the_restatement(W, Lw, O_, monkeypatch):
    monkeypatch.setattr(R, "MAX_WINDOWS", 128)                            # the restatement's cap, raised for this test alone
    Ltot = Lw + (W - 2) * (Lw - O_) + 20                                  # a short last hop: the right-aligned window, a triple cover at O = Lw / 2
    starts, w = L.window_layout(Ltot, Lw, O_, 1, max_windows=128)
    rs, rw, cover = R.weights(Ltot, Lw, O_)
    assert len(starts) == W and starts == rs and starts[-1] == Ltot - Lw
    assert w.dtype == np.float32 and w.tobytes() == rw.tobytes()          # double arithmetic, rounded once: bit for bit
    total = np.zeros(Ltot, np.float64)
    for k, s in enumerate(starts):
        total[s:s + Lw] += w[k].astype(np.float64)
    print((W, Lw, O_), "max |sum w - 1| =", np.abs(total - 1).max(), "largest cover", max(len(c) for c in cover))
    assert np.abs(total - 1).max() <= 1.2e-7
    assert all(c == list(range(c[0], c[0] + len(c))) and 1 <= len(c) <= 3 for c in cover)


@pytest.mark.parametrize("W,P", [(4, 2), (4, 3), (4, 4), (3, 4), (33, 2), (128, 4), (1, 1), (32, 1), (65, 3), (5, 2)])
def test_window_parts_is_the_floor_partition(W, P):
    first = L.window_parts(W, P)
    pe = min(P, W)
    print((W, P), "->", first)
    assert first == [p * W // pe for p in range(pe + 1)] == WP.partition(W, P)
    sizes = [b - a for a, b in zip(first, first[1:])]
    assert sum(sizes) == W and min(sizes) >= 1 and max(sizes) <= 32
    raw = (ctypes.c_int * (P + 1))()
    assert L.load().ldc_window_parts(W, P, raw) == pe and list(raw) == first + [W] * (P - pe)


def test_the_issues_partitions():
    assert L.window_parts(4, 2) == [0, 2, 4] and L.window_parts(4, 3) == [0, 1, 2, 4] and L.window_parts(4, 4) == [0, 1, 2, 3, 4]
    assert L.window_parts(3, 4) == [0, 1, 2, 3] and L.window_parts(33, 2) == [0, 16, 33] and L.window_parts(128, 4) == [0, 32, 64, 96, 128]


@pytest.mark.parametrize("cap", [1, 32, 33, 64, 128])
def test_one_window_too_many_is_refused_with_both_numbers(cap):
    Ltot = 80 + cap * 40                                                  # cap + 1 windows of 80 frames at overlap 40
    rc = L.load().ldc_window_layout_n(Ltot, 80, 40, 10, cap, None, None)
    assert rc == L.E_INVALID
    with pytest.raises(L.LdcError) as ei:
        L.check(rc)
    print(cap, "->", str(ei.value))
    assert ei.value.code == L.E_INVALID and f"{cap + 1} windows" in str(ei.value) and f"at most {cap}" in str(ei.value)
    assert len(L.window_layout(Ltot - 40, 80, 40, 10, max_windows=cap)[0]) == cap


@pytest.mark.parametrize("call,word", [
    (lambda: L.window_parts(4, 0), "parts 0"), (lambda: L.window_parts(4, 5), "parts 5"), (lambda: L.window_parts(0, 2), "W 0"),
    (lambda: L.window_parts(129, 4), "W 129"), (lambda: L.window_parts(33, 1), "W 33"), (lambda: L.window_parts(65, 2), "W 65"),
    (lambda: L.window_layout(180, 80, 40, 10, max_windows=0), "max_windows 0"),
    (lambda: L.window_layout(180, 80, 40, 10, max_windows=129), "max_windows 129"),
    (lambda: L.window_layout(180, 80, 45, 10, max_windows=64), "overlap 45"),
    (lambda: L.window_layout(185, 80, 40, 10, max_windows=64), "Ltot 185"),
])
def test_refusals_name_the_value(call, word):
    with pytest.raises(L.LdcError) as ei:
        call()
    print(word, "->", str(ei.value))
    assert ei.value.code == L.E_INVALID and word in str(ei.value), str(ei.value)


def test_the_layout_keeps_its_32_window_refusal():
    with pytest.raises(L.LdcError) as ei:
        L.window_layout(80 + 32 * 40, 80, 40, 10)
    assert ei.value.code == L.E_INVALID and "33 windows" in str(ei.value)


def test_the_part_boundary_mutant_is_visible_on_the_reference():
    """What the GPU comparison can tell apart, on the oracle alone: r84, Ltot 180, Lw 80, overlap 40 (windows {0, 1} and {2, 3}; the frames
    80..119 are covered by both parts, 100..119 by three windows), 40 steps, one tape."""
    bar = TOL["f32"]["chain_small"]
    ref = R.reference("r84", 180, 80, 40)
    mut = WP.mutant_reference("r84", 180, 80, 40, 2)
    m = float(ref.abs().max())
    d = float((ref - mut).abs().max()) / m
    inside = float((ref - mut)[..., 80:120].abs().max()) / m
    print(f"coupled vs the part-boundary mutant {d:.3e} of max|x| ({inside:.3e} on the frames both parts cover; bar {bar:.1e})")
    assert d >= 10 * bar


def test_forty_windows_are_one_segment_at_two_parts():
    Ltot = 80 + 39 * 40
    assert sample.plan_window_segments(Ltot, 80, 40, 10, max_windows=64) == [(0, Ltot)]
    assert len(sample.plan_window_segments(Ltot, 80, 40, 10)) == 2           # at the engine's cap of 32: two hard-joined segments
    assert len(L.window_layout(Ltot, 80, 40, 10, max_windows=64)[0]) == 40
    assert sample.plan_window_segments(80 + 63 * 40, 80, 40, 10, max_windows=64) == [(0, 80 + 63 * 40)]
    assert len(sample.plan_window_segments(80 + 64 * 40, 80, 40, 10, max_windows=64)) == 2


def test_the_new_symbols_are_exported_and_declared():
    text = open(os.path.join(ROOT, "include", "ladiffcodec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ("ldc_window_layout_n", "ldc_window_parts"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(dll, name) and name in L.EXPORTS
