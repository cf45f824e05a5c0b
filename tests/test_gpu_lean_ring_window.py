"""Round 10: the window ring of the lean conv kernel (conv_lean.inc, ring kind LEAN_RING_W; options ring3_window, ring3_window_tiles).

Where three workgroups of the full three-stage ring do not fit a CU's LDS but three of the window ring do -- the k = 3 128 x 64 tile
without the folded res_conv -- a launch of at most ring3_window_tiles workgroups keeps three WINDOW planes and two slab sets: the slabs of
unit j + 1 and then the window of unit j + 2 are issued during unit j, and the wait in front of unit j + 1 leaves that window outstanding.
Tiles, fragment addresses within a plane or slab, MFMA order per accumulator, split-K slice order and epilogues are those of the two-stage
loop, so every result must be bit for bit that of conv_fast_kernel (single convs: ldc_conv_compare with tile_cfg 101) and of the two-stage
loop (ResnetBlocks with the fused GroupNorm exchange).  (The 64 x 64 tile with the folded res_conv had the mode too while it was measured;
it lost there and was taken out again with its tests: profiles/r10_ring_window.md.)

Every case forces the mode with ring3_window = 1, ring3_window_tiles = 1 << 30 and ring3_wgs = 3 (the default: the full ring keeps the
tiles where three of it fit) and proves through ldc_debug_lean_launches(6) -- the counter of window-ring launches -- that the mode took
the launch, or that it did not.

Shapes: a trip of the loop is three units, so 1 to 6 units reach fewer units than window slots and one, two and three units left behind a
trip (bf16: 32 input channels per unit, f32: 16); the switch to the second input tensor follows the window, which runs one unit ahead
of the slabs: in unit 1, unit 2, the last unit, and at each of the three positions of a trip."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L  # noqa: E402
from gpu_common import engine  # noqa: E402
from test_gpu_lean_ring import engine_dim64  # noqa: E402

K3, K1, K4S2, K7, RING3, RINGW = 0, 1, 3, 4, 5, 6   # ldc_debug_lean_launches: unit kinds; 5 = full three-stage ring, 6 = window ring
ALL = 1 << 30
DEFAULT = {"ring3_tiles": 304, "ring3_wgs": 3, "ring3_window": 1, "ring3_window_tiles": 608, "conv_tile": -1, "conv_splitk": 1}   # ldc_kernels.h: ConvTune


class options:
    """engine options for the duration of the block, the library's defaults again behind it"""

    def __init__(self, e, **kw):
        self.e, self.kw = e, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.e.set_option(k, v)
        return self.e

    def __exit__(self, *exc):
        for k in self.kw:
            self.e.set_option(k, DEFAULT[k])


def forced(e, window=1, tiles=ALL, wgs=3, **kw):
    return options(e, **{"ring3_window": window, "ring3_window_tiles": tiles, "ring3_tiles": ALL, "ring3_wgs": wgs, **kw})


def compare(e, dtype, B, Lx, c1, c2, co, k, stride, ups, cfg, colmax, with_res):
    lib, ctx = e.lib, e._ctx
    dt = L.LDC_F32 if dtype == "f32" else L.LDC_BF16
    before = [lib.ldc_debug_lean_launches(i) for i in range(7)]
    d, m, r = C.c_double(), C.c_double(), C.c_double()
    L.check(lib.ldc_conv_compare(ctx, dt, B, Lx, c1, c2, co, k, stride, ups, 100 + cfg, 0, colmax, with_res, C.byref(d), C.byref(m), C.byref(r)))
    ran = [lib.ldc_debug_lean_launches(i) - before[i] for i in range(7)]
    return d.value, m.value, r.value, ran


# (what, dtypes, B, L, cin1, cin2, cout, ups, residual) -- all k = 3 on the 128 x 64 tile (tile_cfg 101)
SINGLE = [("units_c%d" % c, ("bf16", "f32"), 3, 75, c, 0, 64, 0, i & 1) for i, c in enumerate((32, 64, 96, 128, 160, 192))]
SINGLE += [("units_c%d" % c, ("f32",), 3, 75, c, 0, 64, 0, i & 1) for i, c in enumerate((16, 48, 80))]   # f32: 1, 3, 5 units
SINGLE += [
    ("cat_switch_in_unit_1", ("bf16", "f32"), 3, 75, 32, 96, 64, 0, 0),
    ("cat_switch_in_unit_2", ("bf16", "f32"), 3, 75, 64, 64, 64, 0, 1),
    ("cat_switch_in_last_unit", ("bf16", "f32"), 3, 75, 96, 32, 64, 0, 0),
    # nine bf16 units: the window of the first x2 chunk is issued at position 0 / 1 / 2 of the first trip
    ("cat_switch_at_trip_position_0", ("bf16", "f32"), 3, 75, 64, 224, 64, 0, 1),
    ("cat_switch_at_trip_position_1", ("bf16", "f32"), 3, 75, 96, 192, 64, 0, 0),
    ("cat_switch_at_trip_position_2", ("bf16", "f32"), 3, 75, 128, 160, 64, 0, 1),
    ("cat_switch_in_second_trip", ("bf16",), 3, 75, 192, 96, 64, 0, 0),
    ("folded_upsampling", ("bf16", "f32"), 2, 40, 96, 0, 64, 1, 0),
    ("folded_upsampling_res", ("bf16", "f32"), 2, 40, 96, 0, 64, 1, 1),
    ("partial_last_tile_L53", ("bf16", "f32"), 2, 53, 128, 0, 128, 0, 0),
    ("partial_last_tile_L53_res", ("bf16", "f32"), 2, 53, 128, 0, 128, 0, 1),
    ("waves_without_pieces", ("bf16", "f32"), 1, 20, 128, 0, 128, 0, 0),
    ("waves_without_pieces_res", ("bf16", "f32"), 1, 20, 96, 0, 64, 0, 1),
]
SINGLE_CASES = [pytest.param(c, dt, id="%s-%s" % (c[0], dt)) for c in SINGLE for dt in c[1]]


@pytest.mark.parametrize("case,dtype", SINGLE_CASES)
def test_window_ring_single_conv_is_bit_identical_to_conv_fast_kernel(case, dtype):
    what, _, B, Lx, c1, c2, co, ups, with_res = case
    with forced(engine("r84", dtype)) as e:
        d, m, r, ran = compare(e, dtype, B, Lx, c1, c2, co, 3, 1, ups, 1, 0, with_res)
    print(what, dtype, "diff", d, "max", m, "launches", ran)
    assert ran[RINGW] == 1 and ran[K3] == 1 and ran[RING3] == 0, ("the window ring did not take this launch", case, ran)
    assert m > 0.1 and d == 0.0 and r == 0.0, (case, dtype, d, m, r)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_window_ring_split_k_is_bit_identical(dtype):
    """Cin = 1024 at one item of 75 positions on the forced 128 x 64 tile: 1 x 16 tiles with 32 (bf16) / 64 (f32) units each, which the
    launcher still splits in K (sk_u2 = 24: two slices; f32, sk_u3 = 60: three): the later slices start at u_begin != 0, every slice
    runs its own prologue, trips and drain, and the slices are summed in slice order by whichever arrives last."""
    with forced(engine("r84", dtype)) as e:
        d, m, r, ran = compare(e, dtype, 1, 75, 1024, 0, 1024, 3, 1, 0, 1, 0, 0)
        with options(e, conv_splitk=0):
            d1, m1, r1, ran1 = compare(e, dtype, 1, 75, 1024, 0, 1024, 3, 1, 0, 1, 0, 0)
    print(dtype, "diff", d, "max", m, "launches", ran, "| unsplit diff", d1, "launches", ran1)
    assert ran[RINGW] == 1 and ran[K3] == 1 and ran[RING3] == 0, ran
    assert m > 0.1 and d == 0.0, (dtype, d, m)
    assert ran1[RINGW] == 1 and m1 > 0.1 and d1 == 0.0, (dtype, d1, m1, ran1)   # (the same conv as 32 / 64 units of one slice: ten and more trips)


def test_window_ring_preference_and_thresholds():
    """3 x 75 rows x 128 columns, k = 3.  On 64 x 64 tiles three full rings fit a CU: the FULL ring takes the launch.  On 128 x 64 tiles
    (2 x 2 = 4 workgroups) they do not: the window ring takes it at ring3_wgs 3, the full ring at ring3_wgs 2 (two of it fit), two stages
    with ring3_window 0 and with ring3_window_tiles below the grid.  The full ring's own threshold (ring3_tiles) does not gate it."""
    e = engine("r84", "bf16")
    #        tile, window, window tiles, wgs -> (full ring, window ring)
    table = [(0, 1, ALL, 3, (1, 0)),
             (1, 1, ALL, 3, (0, 1)),
             (1, 1, ALL, 2, (1, 0)),
             (1, 0, ALL, 3, (0, 0)),
             (1, 1, 4, 3, (0, 1)),
             (1, 1, 3, 3, (0, 0)),
             (1, 1, 0, 3, (0, 0))]
    for cfg, window, tiles, wgs, want in table:
        with forced(e, window, tiles, wgs):
            d, m, r, ran = compare(e, "bf16", 3, 75, 96, 0, 128, 3, 1, 0, cfg, 0, 0)
        assert ran[K3] == 1 and (ran[RING3], ran[RINGW]) == want and d == 0.0, (cfg, window, tiles, wgs, ran, d)
    with forced(e, 1, ALL, 3, ring3_tiles=0):
        d, m, r, ran = compare(e, "bf16", 3, 75, 96, 0, 128, 3, 1, 0, 1, 0, 0)
    assert ran[K3] == 1 and (ran[RING3], ran[RINGW]) == (0, 1) and d == 0.0, (ran, d)


def test_window_ring_is_on_by_default_for_the_128_row_tile():
    """The library's defaults (profiles/r10_ring_window.md): ring3_window 1, ring3_window_tiles 608, ring3_tiles 304, ring3_wgs 3."""
    e = engine("r84", "bf16")
    d, m, r, ran = compare(e, "bf16", 3, 75, 96, 0, 128, 3, 1, 0, 1, 0, 0)
    assert ran[K3] == 1 and (ran[RING3], ran[RINGW]) == (0, 1) and d == 0.0, (ran, d)
    d, m, r, ran = compare(e, "bf16", 3, 75, 96, 0, 128, 3, 1, 0, 0, 0, 0)
    assert ran[K3] == 1 and (ran[RING3], ran[RINGW]) == (1, 0) and d == 0.0, (ran, d)


def test_window_ring_leaves_k4_k7_and_1x1_alone():
    """k = 4 stride 2 and k = 7 (the launcher's tile) and a 1x1 conv on the 128 x 64 tile (three workgroups of neither ring fit) under
    the forced option: the lean kernel of their kind runs on two stages, the window ring's counter stays."""
    with forced(engine("r84", "bf16")) as e:
        for kind, (B, Lx, c1, co, k, stride, cfg, colmax) in ((K4S2, (3, 150, 64, 128, 4, 2, 99, 0)), (K7, (3, 75, 96, 128, 7, 1, 99, 0)), (K1, (3, 75, 192, 128, 1, 1, 1, 1))):
            d, m, r, ran = compare(e, "bf16", B, Lx, c1, 0, co, k, stride, 0, cfg, colmax, 0)
            assert ran[kind] == 1 and ran[RINGW] == 0 and ran[RING3] == 0, (kind, ran)
            assert m > 0.1 and d == 0.0 and r == 0.0, (kind, d, m, r)


# ------------------------------------------------------------------------------------------------ ResnetBlocks: fused GroupNorm, folded res_conv
# 256-channel blocks of the dim-64 engine: plain (down4.1, mid.2) | res_conv on a concatenated input (up0.1: 256 + 256, up1.2: 256 + 128)
# (what, dtype, further options, blocks, blocks whose res_conv must be folded into block1's conv)
BLOCK_CASES = [
    # 128-row tiles: both convs of a plain block (GN and GN + residual epilogues); block2 behind a block1 with the folded res_conv, which
    # itself stays on two stages (bf16); f32 splits the 512- and 384-channel convs in K, so there res_conv is a launch of its own and
    # block1 of up0.1 / up1.2 runs the fused epilogue under split-K
    ("128row", "bf16", {"conv_tile": 1}, ["down4.1", "mid.2", "up0.1", "up1.2"], ["up0.1", "up1.2"]),
    ("128row", "f32", {"conv_tile": 1}, ["down4.1", "mid.2", "up0.1", "up1.2"], []),
]


@pytest.mark.parametrize("Ln", [75, 150])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_window_ring_resnet_blocks_are_bit_identical_to_two_stages(case, Ln):
    """The forms a single-conv check cannot set up: the GroupNorm apply inside the conv epilogue with its in-launch exchange (granules
    summed in a fixed order: bit for bit), with and without a residual, split-K under the fused epilogue; B = 3 items whose tiles
    straddle.  Window ring on against off, everything else equal."""
    import resnet_restatement as R
    what, dtype, extra, blocks, folded = case
    e, u = engine_dim64(dtype)
    bt = R.block_table(u)
    lib = e.lib
    for name in blocks:
        c1, c2 = bt[name]["cin1"], bt[name]["cin2"]
        g = torch.Generator().manual_seed(2000 + Ln + len(name))
        x1 = torch.randn(3, c1, Ln, generator=g).cuda()
        x2 = torch.randn(3, c2, Ln, generator=g).cuda() if c2 else None
        res = {}
        for window in (0, 1):
            with forced(e, window, **extra):
                before = lib.ldc_debug_lean_launches(RINGW)
                got = e.debug_resnet_block(name, x1, x2, t=17)
                ran = lib.ldc_debug_lean_launches(RINGW) - before
            res[window] = (got["out"].cpu(), got["mid"].cpu(), got["info"], ran)
        info = res[1][2]
        print(what, name, Ln, dtype, info, "window-ring launches", res[0][3], res[1][3])
        assert info["epi1"] == 1 and info["epi2"] == 1, ("the case is meant for the fused GroupNorm epilogue", name, info)
        if name in folded:
            assert info["folded"], ("the case is meant for the folded res_conv", name, info)
        assert res[0][3] == 0 and res[1][3] >= 1, (name, res[0][3], res[1][3])
        assert torch.isfinite(res[1][0]).all() and float(res[1][0].abs().max()) > 0.1
        assert torch.equal(res[0][0], res[1][0]), (name, Ln, dtype, "out", float((res[0][0] - res[1][0]).abs().max()))
        assert torch.equal(res[0][1], res[1][1]), (name, Ln, dtype, "mid", float((res[0][1] - res[1][1]).abs().max()))
