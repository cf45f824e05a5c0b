"""Round 7: the lean conv kernel's unit kinds for the stride-2 downsamples (k = 4, pad 1) and init_conv (k = 7, two tap groups per chunk).

Like the k = 3 / k = 1 kinds they keep conv_fast_kernel's tiles, LDS image, MFMA order per accumulator, split-K slice order and epilogue
arithmetic, so ONE conv on the same operands must come out bit for bit the same through both kernels (ldc_conv_compare with tile_cfg + 100:
pass 0 with conv_lean off, pass 1 with it on).  Every case also proves through ldc_debug_lean_launches that the lean kernel of the expected
kind ran in pass 1 -- a case the launcher quietly kept on conv_fast_kernel would compare that kernel with itself.

Shapes: the smallest that reach every branch -- a partial last tile and tiles straddling items (M = B L not a multiple of the tile), an odd
number of units, one chunk only, both tile heights (64 and 128 rows: the k = 4 plane of a 128-row tile is copied as two runs), the residual
epilogue, split-K where the launcher splits (k = 4) and the proof that it does not (k = 7: its units alternate between the two tap groups).
Folded nearest upsampling (k = 3) needs no kind of its own: the k = 3 kind's fragment rows are (m + tap - 1) >> 1 already; its cases pin that."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L  # noqa: E402
from gpu_common import engine  # noqa: E402

K3, K4S2, K7 = 0, 3, 4   # unit kinds (conv_lean.inc)


def compare(B, Lx, c1, co, k, stride, ups, cfg, with_res, kind):
    e = engine("r84", "bf16")
    lib, ctx = e.lib, e._ctx
    before = lib.ldc_debug_lean_launches(kind)
    d, m, r = C.c_double(), C.c_double(), C.c_double()
    L.check(lib.ldc_conv_compare(ctx, L.LDC_BF16, B, Lx, c1, 0, co, k, stride, ups, 100 + cfg, 0, 0, with_res, C.byref(d), C.byref(m), C.byref(r)))
    ran = lib.ldc_debug_lean_launches(kind) - before
    return d.value, m.value, ran


# (B, L_in, cin, cout, k, stride, ups, tile_cfg (0: 64 x 64, 1: 128 x 64, 99: the launcher's choice), residual, kind)
CASES = [
    # folded nearest x2 upsampling on the k = 3 kind
    (3, 75, 64, 64, 3, 1, 1, 99, 0, K3),      # M = 450: partial last tile, tiles straddle items
    (2, 40, 96, 64, 3, 1, 1, 99, 0, K3),      # odd unit count
    (2, 40, 96, 128, 3, 1, 1, 0, 0, K3),      # 64 x 64 tiles
    # k = 4, stride 2, pad 1
    (3, 150, 64, 128, 4, 2, 0, 99, 0, K4S2),  # L 150 -> 75, M = 225
    (3, 150, 64, 128, 4, 2, 0, 0, 0, K4S2),   # ... 64-row tiles (plane of 144 rows, one run)
    (3, 150, 64, 128, 4, 2, 0, 1, 1, K4S2),   # ... 128-row tiles (272 rows, two runs), residual
    (1, 64, 96, 64, 4, 2, 0, 99, 0, K4S2),    # L 64 -> 32: one partial tile, odd unit count
    (2, 600, 64, 64, 4, 2, 0, 99, 1, K4S2),   # full 128-row tiles: every wave copies all five pieces
    # k = 7 (taps 0-3 | 4-6)
    (2, 200, 128, 64, 7, 1, 0, 99, 1, K7),    # residual (init_conv's x half: the condition's half arrives as the residual)
    (3, 75, 32, 64, 7, 1, 0, 99, 0, K7),      # one chunk: two units
    (3, 75, 96, 128, 7, 1, 0, 0, 0, K7),      # 64 x 64 tiles, three chunks
    (3, 75, 96, 128, 7, 1, 0, 1, 1, K7),      # 128 x 64 tiles
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_L%d_c%d-%d_k%d_s%d_u%d_t%d_r%d" % c[:9])
def test_lean_kind_is_bit_identical_to_conv_fast_kernel(case):
    B, Lx, c1, co, k, stride, ups, cfg, with_res, kind = case
    d, m, ran = compare(B, Lx, c1, co, k, stride, ups, cfg, with_res, kind)
    assert ran == 1, ("the lean kernel of kind %d did not take this launch" % kind, case)
    assert m > 0.1 and d == 0.0, (case, d, m)


def test_lean_k4_split_k_is_bit_identical_and_k7_is_never_split():
    """Cin = 1024 at one item of 75 output positions: 32 units on 2 x 16 tiles of 64 x 64 -- the launcher splits K in two (sk_u2 = 24) for
    k = 3 and k = 4; the slices are summed in slice order by whichever arrives last, so the result is still bit-identical.  k = 7 has
    64 units there but two tap groups per chunk: the launcher never splits it, and the lean kernel (which refuses a split k = 7 launch)
    must therefore have taken it."""
    d, m, ran = compare(1, 150, 1024, 1024, 4, 2, 0, 99, 0, K4S2)
    assert ran == 1 and m > 0.1 and d == 0.0, (d, m, ran)
    d, m, ran = compare(1, 37, 1024, 1024, 3, 1, 1, 99, 0, K3)   # (74 output positions through the folded upsampling)
    assert ran == 1 and m > 0.1 and d == 0.0, (d, m, ran)
    d, m, ran = compare(1, 75, 1024, 128, 7, 1, 0, 99, 0, K7)
    assert ran == 1 and m > 0.1 and d == 0.0, (d, m, ran)


def test_lean_all_off_keeps_the_new_kinds_on_conv_fast_kernel():
    """Option lean_all = 0 (A/B): k = 4 / k = 7 launches stay on conv_fast_kernel while the k = 3 / k = 1 kinds keep the lean kernel."""
    e = engine("r84", "bf16")
    e.set_option("lean_all", 0)
    try:
        for case in (CASES[3], CASES[9]):
            d, m, ran = compare(*case)
            assert ran == 0 and d == 0.0, (case, d, ran)
        d, m, ran = compare(*CASES[0])
        assert ran == 1 and d == 0.0, (d, ran)
    finally:
        e.set_option("lean_all", 1)
