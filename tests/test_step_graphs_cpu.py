"""The graph-length rule of the sampler loops on the host (ldc_graph_schedule: no context, no GPU): rows pinned by hand from the rule,
an exhaustive sweep against the Python restatement (tests/step_graphs_restatement.py), the refusals."""
import ctypes

import pytest

from ladiffcodec_amd import lib as L
import step_graphs_restatement as R

# (n_steps, parts, strided, option) -> K
PINNED = [
    ((50, 2, 0, 0), 5),
    ((50, 1, 0, 0), 10),
    ((13, 2, 0, 0), 5),
    ((12, 2, 0, 0), 4),       # 4 and 6 are equally near to 5: the smaller
    ((3, 2, 0, 0), 2),        # clamped to n_steps - 1
    ((4, 1, 0, 0), 3),        # likewise
    ((50, 3, 0, 0), 5),
    ((50, 2, 0, 7), 7),
    ((5, 2, 0, 7), 4),
    ((3, 2, 1, 0), 5),        # strided: one length whatever the step count
    ((20, 1, 1, 0), 5),
    ((20, 2, 1, 3), 3),
]


def schedule(n_steps, parts, strided, option):
    K, nb, ns = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.load().ldc_graph_schedule(n_steps, parts, strided, option, ctypes.byref(K), ctypes.byref(nb), ctypes.byref(ns))
    return rc, (K.value, nb.value, ns.value)


@pytest.mark.parametrize("args,K", PINNED)
def test_pinned_rows(args, K):
    rc, got = schedule(*args)
    print(args, "->", got)
    assert rc == 0
    assert got[0] == K
    assert got == R.schedule(*args)
    assert got[1:] == divmod(args[0], K)


def test_every_small_loop_against_the_restatement():
    n = 0
    for n_steps in range(1, 121):
        for parts in range(1, R.MAX_PARTS + 1):
            for strided in (0, 1):
                for option in (0, 1, 3, 5, 10, 25, 1000):
                    rc, (K, n_big, n_single) = schedule(n_steps, parts, strided, option)
                    where = (n_steps, parts, strided, option)
                    assert rc == 0, where
                    assert (K, n_big, n_single) == R.schedule(*where), where
                    assert n_big * K + n_single == n_steps, where
                    assert 1 <= K and 0 <= n_single < K and n_big >= 0, where
                    n += 1
    assert n == 120 * 4 * 2 * 7


def test_outputs_are_optional():
    lib = L.load()
    K = ctypes.c_int(-1)
    assert lib.ldc_graph_schedule(50, 2, 0, 0, ctypes.byref(K), None, None) == 0 and K.value == 5
    assert lib.ldc_graph_schedule(50, 2, 0, 0, None, None, None) == 0


@pytest.mark.parametrize("args,names", [
    ((0, 2, 0, 0), ("n_steps 0",)),
    ((-3, 2, 0, 0), ("n_steps -3",)),
    ((50, 0, 0, 0), ("parts 0", "[1, 4]")),
    ((50, 5, 0, 0), ("parts 5", "[1, 4]")),
    ((50, 2, 1, -1), ("graph_steps_option -1",)),
])
def test_refusals_name_the_value(args, names):
    rc, got = schedule(*args)
    msg = L.load().ldc_last_error().decode()
    print(args, "->", rc, msg)
    assert rc == L.E_INVALID
    assert got == (-1, -1, -1)                                     # nothing written
    for name in names:
        assert name in msg, (name, msg)
    with pytest.raises(ValueError):
        R.schedule(*args)
