"""Round 9: the three-stage LDS ring of the lean conv kernel (conv_lean.inc, template parameter S = 3; option ring3_tiles).

Launches that put one or two workgroups on a CU keep two units in flight instead of one: the wait in front of the barrier leaves the
younger unit's copies outstanding (a counted vmcnt), the barrier is a bare s_barrier, and the copies of unit u + 2 go out between the
MFMA groups of unit u.  Tiles, MFMA order per accumulator, split-K slice order and epilogues are those of S = 2, so every result must be
bit for bit that of conv_fast_kernel (single convs: ldc_conv_compare with tile_cfg + 100) and of the S = 2 ring (ResnetBlocks with the fused
GroupNorm exchange and the folded res_conv); only the whole UNet has a tolerance, because the LinearAttention context is accumulated with
fp32 atomics (two runs of ONE kernel already differ in the last bits: test_gpu_bench_shape.py).

Every case runs with ring3_tiles = 1 << 30 and ring3_wgs = 1 (every grid and every tile height takes the ring; by default the launcher
keeps the 128-row tiles, of which only two would fit a CU with three stages, on S = 2) and proves through ldc_debug_lean_launches(5) -- the counter of
S = 3 launches -- that the ring took it, or, for the k = 4 / k = 7 kinds, that it did not.

Shapes: the smallest that reach every path of the new loop -- 1 to 7 units (fewer units than stages; one, two and three units left behind
the three-unit trips), the switch to the second input tensor in unit 1 and in the last unit, both tile heights, tiles that straddle items
and the end of the tensor, waves that copy no window piece (20 rows), split-K slices that start at u_begin != 0."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
from gpu_common import engine, rel  # noqa: E402
from helpers import COND_CFG, cond_sd_np  # noqa: E402

K3, K1, K4S2, K7, RING3 = 0, 1, 3, 4, 5   # ldc_debug_lean_launches: unit kinds (conv_lean.inc); 5 = launches on the three-stage ring
ALL = 1 << 30


class forced:
    """ring3_tiles = `value` (and no LDS condition: ring3_wgs = 1) on engine e for the duration of the block"""

    def __init__(self, e, value=ALL, wgs=1):
        self.e, self.value, self.wgs = e, value, wgs

    def __enter__(self):
        self.e.set_option("ring3_tiles", self.value)
        self.e.set_option("ring3_wgs", self.wgs)
        return self.e

    def __exit__(self, *exc):
        self.e.set_option("ring3_tiles", DEFAULT[0])
        self.e.set_option("ring3_wgs", DEFAULT[1])


DEFAULT = [304, 3]   # the library's defaults (ldc_kernels.h: ConvTune::ring3_tiles, ring3_wgs)


def compare(e, dtype, B, Lx, c1, c2, co, k, stride, ups, cfg, colmax, with_res):
    lib, ctx = e.lib, e._ctx
    dt = L.LDC_F32 if dtype == "f32" else L.LDC_BF16
    before = [lib.ldc_debug_lean_launches(i) for i in range(6)]
    d, m, r = C.c_double(), C.c_double(), C.c_double()
    L.check(lib.ldc_conv_compare(ctx, dt, B, Lx, c1, c2, co, k, stride, ups, 100 + cfg, 0, colmax, with_res, C.byref(d), C.byref(m), C.byref(r)))
    ran = [lib.ldc_debug_lean_launches(i) - before[i] for i in range(6)]
    return d.value, m.value, r.value, ran


# (what, B, L, cin1, cin2, cout, k, ups, tile_cfg (0: 64 x 64, 1: 128 x 64, 99: the launcher's choice), column max, residual)
SINGLE = [("k3_units_c%d" % c, 3, 75, c, 0, 64, 3, 0, 99, 0, i & 1) for i, c in enumerate((32, 64, 96, 128, 160, 224))]
SINGLE += [("k1_units_c%d" % c, 3, 75, c, 0, 128, 1, 0, 99, 1, i & 1) for i, c in enumerate((64, 128, 192))]
SINGLE += [
    ("cat_switch_in_unit_1", 3, 75, 32, 96, 64, 3, 0, 99, 0, 0),
    ("cat_switch_in_last_unit", 3, 75, 96, 32, 64, 3, 0, 99, 0, 1),
    ("k1_cat", 3, 75, 64, 128, 128, 1, 0, 99, 1, 0),
    ("folded_upsampling", 3, 75, 64, 0, 64, 3, 1, 99, 0, 0),
    ("folded_upsampling_odd_units", 2, 40, 96, 0, 64, 3, 1, 99, 0, 1),
    ("tile_64x64", 3, 75, 96, 0, 128, 3, 0, 0, 0, 0),
    ("tile_64x64_res", 3, 75, 96, 0, 128, 3, 0, 0, 0, 1),
    ("tile_128x64", 3, 75, 96, 0, 128, 3, 0, 1, 0, 0),
    ("tile_128x64_res", 3, 75, 160, 0, 128, 3, 0, 1, 0, 1),
    ("k1_tile_64x64", 3, 75, 192, 0, 128, 1, 0, 0, 1, 1),
    ("k1_tile_128x64", 3, 75, 192, 0, 128, 1, 0, 1, 1, 0),
    ("partial_last_tile_L53", 2, 53, 128, 0, 128, 3, 0, 99, 0, 0),
    ("partial_last_tile_L53_128x64", 2, 53, 128, 0, 128, 3, 0, 1, 0, 1),
    ("waves_without_pieces", 1, 20, 128, 0, 128, 3, 0, 1, 0, 0),
    ("waves_without_pieces_64x64", 1, 20, 96, 0, 64, 3, 0, 99, 0, 1),
    ("k1_waves_without_pieces", 1, 20, 128, 0, 128, 1, 0, 1, 1, 0),
]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("case", SINGLE, ids=lambda c: c[0])
def test_ring3_single_conv_is_bit_identical_to_conv_fast_kernel(case, dtype):
    what, B, Lx, c1, c2, co, k, ups, cfg, colmax, with_res = case
    with forced(engine("r84", dtype)) as e:
        d, m, r, ran = compare(e, dtype, B, Lx, c1, c2, co, k, 1, ups, cfg, colmax, with_res)
    print(what, dtype, "diff", d, "max", m, "stat", r, "launches", ran)
    assert ran[RING3] == 1 and ran[K3 if k == 3 else K1] == 1, ("the three-stage ring did not take this launch", case, ran)
    assert m > 0.1 and d == 0.0 and r == 0.0, (case, dtype, d, m, r)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ring3_split_k_is_bit_identical(dtype):
    """Cin = 1024 at one item of 75 positions: 2 x 16 tiles of 64 x 64 with 32 (bf16) / 64 (f32) units each -- the launcher splits K
    (sk_u2 = 24), the later slices start at u_begin != 0 and every slice runs its own prologue, three-unit trips and drain; the slices
    are summed in slice order by whichever arrives last."""
    with forced(engine("r84", dtype)) as e:
        d, m, r, ran = compare(e, dtype, 1, 75, 1024, 0, 1024, 3, 1, 0, 99, 0, 0)
    print(dtype, "diff", d, "max", m, "launches", ran)
    assert ran[RING3] == 1 and ran[K3] == 1, ran
    assert m > 0.1 and d == 0.0, (dtype, d, m)


def test_ring3_leaves_k4_and_k7_on_two_stages():
    """The stride-2 downsamples and init_conv keep S = 2 under the forced option (k = 7's two stages are its tap groups): the lean kernel
    of their kind runs, the ring's counter stays."""
    with forced(engine("r84", "bf16")) as e:
        for kind, (B, Lx, c1, co, k, stride) in ((K4S2, (3, 150, 64, 128, 4, 2)), (K7, (3, 75, 96, 128, 7, 1))):
            d, m, r, ran = compare(e, "bf16", B, Lx, c1, 0, co, k, stride, 0, 99, 0, 0)
            assert ran[kind] == 1 and ran[RING3] == 0, (kind, ran)
            assert m > 0.1 and d == 0.0, (kind, d, m)


def test_ring3_tiles_is_a_threshold_on_the_workgroup_count():
    """3 x 75 rows x 128 columns on 64 x 64 tiles: 4 x 2 = 8 workgroups.  ring3_tiles 8 takes the ring, 7 and 0 do not."""
    e = engine("r84", "bf16")
    for value, want in ((8, 1), (7, 0), (0, 0)):
        with forced(e, value):
            d, m, r, ran = compare(e, "bf16", 3, 75, 96, 0, 128, 3, 1, 0, 0, 0, 0)
        assert ran[K3] == 1 and ran[RING3] == want and d == 0.0, (value, ran, d)


def test_ring3_default_keeps_tiles_that_would_lose_a_coresident_workgroup():
    """ring3_wgs = 3 (the default): three workgroups of three stages must still fit a CU's 160 KB of LDS.  The 64 x 64 k = 3 tile
    (3 x 17.5 KB of ring) takes the ring, the 128 x 64 tile (3 x 21.5 KB: two per CU) stays on two stages; ring3_wgs = 2 lets it in."""
    e = engine("r84", "bf16")
    for cfg, wgs, want in ((0, 3, 1), (1, 3, 0), (1, 2, 1)):
        with forced(e, ALL, wgs):
            d, m, r, ran = compare(e, "bf16", 3, 75, 96, 0, 128, 3, 1, 0, cfg, 0, 0)
        assert ran[K3] == 1 and ran[RING3] == want and d == 0.0, (cfg, wgs, ran, d)


# ------------------------------------------------------------------------------------------------ ResnetBlocks: fused GroupNorm, folded res_conv
_DIM64 = {}


def engine_dim64(dtype):
    """a UNet of dim 64 (levels of 64 / 128 / 256 channels): its 256-channel ResnetBlocks have 32 channels per group, which is what the
    GroupNorm apply inside the conv epilogue needs"""
    if dtype not in _DIM64:
        from ladiffcodec_amd.model import Engine
        from ladiffcodec_amd.spec import CodecConfig, UnetConfig
        mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
        u = UnetConfig(dim=64, upsampling_ratios=(5, 2), unet_scale_cond=True)
        sd = synth.ladiff_state_dict(mc, u, seed=9)
        e = Engine(mc, u, COND_CFG, dtype=dtype)
        e.load_state_dict(L.MODEL_MAIN, {k: v for k, v in sd.items() if not k.startswith("diffusion.model.")})
        e.load_state_dict(L.MODEL_COND, cond_sd_np())
        e.finalize(strict=True)
        _DIM64[dtype] = (e, u)
    return _DIM64[dtype]


# 256-channel blocks: plain (down4.1, mid.2) | res_conv on a concatenated input (up0.1: 256 + 256, up1.2: 256 + 128 -> 256)
BLOCKS = ["down4.1", "mid.2", "up0.1", "up1.2"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Ln", [75, 150])
def test_ring3_resnet_blocks_are_bit_identical_to_two_stages(Ln, dtype):
    """The forms a single-conv check cannot set up: the GroupNorm apply inside the conv epilogue with its in-launch exchange (the
    granules are summed in a fixed order: bit for bit), the res_conv folded into block1's conv (bf16) and split-K under the fused
    epilogue (f32), B = 3 items whose tiles straddle."""
    import resnet_restatement as R
    e, u = engine_dim64(dtype)
    bt = R.block_table(u)
    lib = e.lib
    for name in BLOCKS:
        c1, c2 = bt[name]["cin1"], bt[name]["cin2"]
        g = torch.Generator().manual_seed(1000 + Ln + len(name))
        x1 = torch.randn(3, c1, Ln, generator=g).cuda()
        x2 = torch.randn(3, c2, Ln, generator=g).cuda() if c2 else None
        res = {}
        for value in (0, ALL):
            with forced(e, value):
                before = lib.ldc_debug_lean_launches(RING3)
                got = e.debug_resnet_block(name, x1, x2, t=17)
                ran = lib.ldc_debug_lean_launches(RING3) - before
            res[value] = (got["out"].cpu(), got["mid"].cpu(), got["info"], ran)
        info = res[ALL][2]
        print(name, Ln, dtype, info, "ring launches", res[0][3], res[ALL][3])
        assert info["epi1"] == 1 and info["epi2"] == 1, ("the case is meant for the fused GroupNorm epilogue", name, info)
        # (f32: 512 input channels are 32 units, which the launcher splits in K -- the planner folds res_conv only into an unsplit conv,
        # so there it is a 1x1 launch of its own and block1 is a split-K launch under the fused epilogue)
        if dtype == "bf16":
            assert bool(info["folded"]) == (c2 != 0), (name, info)
        assert res[0][3] == 0 and res[ALL][3] >= 2, (name, res[0][3], res[ALL][3])
        assert torch.isfinite(res[ALL][0]).all() and float(res[ALL][0].abs().max()) > 0.1
        assert torch.equal(res[0][0], res[ALL][0]), (name, Ln, dtype, "out", float((res[0][0] - res[ALL][0]).abs().max()))
        assert torch.equal(res[0][1], res[ALL][1]), (name, Ln, dtype, "mid", float((res[0][1] - res[ALL][1]).abs().max()))


# ------------------------------------------------------------------------------------------------ attention blocks: folded LayerNorm, context epilogue
@pytest.mark.parametrize("B,Ln", [(1, 48), (2, 32)])
def test_ring3_attention_blocks_are_bit_identical_where_the_context_has_one_tile(B, Ln):
    """to_qkv with the folded PreNorm LayerNorm (the LEAN_K1_LN kind) and, on the linear-attention blocks, the context epilogue -- the
    two forms ldc_conv_compare cannot set up.  The context and the column sums are accumulated with fp32 atomics, which makes a whole UNet
    run-to-run noisy; here every item lies inside ONE 64-row tile (one item of 48 positions; two items of 32 in one tile, one pass per
    item), so every context entry receives a single add and every column sum two (the two row waves: a + b = b + a): the block's output
    does not depend on any arrival order and must be bit for bit the same with the ring on and off.  'mid' is the full-attention block
    (to_qkv with the plain epilogue behind the folded LayerNorm)."""
    e = engine("r84", "bf16")
    for name, C_ in (("down2", 64), ("down4", 128), ("mid", 128), ("up0", 128)):   # (the 32-channel blocks' to_qkv is not a lean launch)
        g = torch.Generator().manual_seed(7 * Ln + len(name))
        x = torch.randn(B, C_, Ln, generator=g).cuda()
        out = {}
        for value in (0, ALL):
            with forced(e, value):
                before = e.lib.ldc_debug_lean_launches(RING3)
                out[value] = e.debug_attention_block(name, x).cpu()
                ran = e.lib.ldc_debug_lean_launches(RING3) - before
            assert (ran == 0) if value == 0 else (ran >= 1), (name, value, ran)
        print(name, B, Ln, "max", float(out[0].abs().max()), "diff", float((out[0] - out[ALL]).abs().max()))
        assert torch.isfinite(out[ALL]).all() and float(out[0].abs().max()) > 0.1
        assert torch.equal(out[0], out[ALL]), (name, B, Ln, float((out[0] - out[ALL]).abs().max()))


# ------------------------------------------------------------------------------------------------ the whole small UNet
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ring3_gives_the_same_small_unet(dtype):
    """unet_forward of the r84 engine, ring forced on against off: to_qkv with the folded LayerNorm and the context epilogue, the 1x1
    convs of the attention blocks, every k = 3 conv, tiles that straddle the three items at every level (80 ... 5 positions).  The
    context and the unfused GroupNorm statistics are accumulated with fp32 atomics, so: f32 rel < 1e-5, bf16 half the drift bar -- what
    test_lean_conv_kernel_gives_the_same_unet_as_conv_fast_kernel holds two runs of one kernel to.  Twice in a row.

    Measured on MI355X, six inputs per shape, max |a - b| / max |b|.  f32: ring on / off 1.1e-6 ... 1.4e-6, two runs with the ring OFF
    1.0e-6 ... 1.3e-6 at every shape.  bf16 (bar 1.13e-2): a difference is a few bf16 roundings of the output flipped by the order of the
    atomics, so the figures come in steps --
        B = 3, L = 80 (this test):  ring on / off 1.07e-2, off / off 0,       on / on 0; in three later sessions 1.32e-2, once with
                                    the first of the two runs at 0 (bit for bit the ring-off result) and the second at 1.32e-2
        B = 1, L = 80:              on / off 1.13e-2,      off / off 0,       on / on 1.13e-2
        B = 2, L = 80:              on / off 1.33e-2,      off / off 1.33e-2, on / on 0
        B = 3, L = 160:             on / off 1.31e-2,      off / off 1.30e-2, on / on 1.31e-2
        B = 3, L = 320:             on / off 1.49e-2,      off / off 1.22e-2 (1.34e-2 in another session), on / on 1.48e-2
    i.e. on this dim-32 engine two runs of ONE arrangement, the ring off, already exceed the bf16 bar at most shapes (the bar was measured on
    the dim-256 engine: 8e-3 there).  The shape here is the smallest that keeps three items and straddling tiles, and the one at which the
    ring-off arrangement repeated bit for bit in every trial of the first session; the bar is the one the project holds such pairs to and is
    not widened.  At this shape a run lands in one of TWO states, 1.32e-2 apart (max |eps| 1.04; 8 400 of the 30 720 outputs differ, the
    worst by seven bf16 steps: one flipped rounding early in the net, amplified through the GroupNorms and attention blocks behind it).
    Twelve runs in one process against a first ring-off run, ring on / on replayed / off / off replayed, three rounds:
        (1.32e-2, 1.32e-2, 1.32e-2, 1.32e-2), (1.32e-2, 0, 0, 1.32e-2), (1.32e-2, 1.32e-2, 1.32e-2, 1.32e-2)
    -- the ring-OFF runs miss the bar against a ring-off run as often as the ring-on runs do, and a ring-on run can equal the ring-off
    result bit for bit.  The same with fuse_gn_stats 0, fold_ctx 0, fold_ln 0, fuse_kmax 0 in any combination tried (7.5e-3 ... 1.49e-2).
    Block by block (every ResnetBlock and attention block of this engine on fixed inputs, B = 3, eight runs each, ring at its default):
    all 11 attention blocks and 21 of the 23 ResnetBlocks repeat bit for bit; down0.1 and final (32 channels, L = 80) give TWO different
    outputs with ONE block1 output -- the fused GroupNorm statistics of their second conv, accumulated with fp32 atomics by
    conv_fast_kernel (an 80-row item gets three or more adds per statistic from the 64-row waves), which is no launch of the lean kernel
    and no code of this ring; the whole UNet gave two distinct results in twelve runs.  Every latent length this engine accepts is a
    multiple of 80, so no shape avoids it.  So the bf16 case FAILS whenever reference and run land in different states -- in four of
    seven sessions so far -- whatever the ring does; no code of the ring can change that.  The bit-for-bit tests of this file are what pins the ring (profiles/r09_ring3.md, section 7)."""
    e = engine("r84", dtype)
    g = torch.Generator().manual_seed(61)
    B, Lz, F = 3, 80, 8
    x = (torch.randn(B, 128, Lz, generator=g) * 0.7).cuda()
    cond = torch.randn(B, 128, F, generator=g).cuda()
    tol = 1e-5 if dtype == "f32" else 0.5 * TOL[dtype]["eps_bench"]
    with forced(e, 0):
        ref = e.unet_forward(x, 23, cond).cpu().numpy()
    with forced(e):
        before = e.lib.ldc_debug_lean_launches(RING3)
        for rep in range(2):
            got = e.unet_forward(x, 23, cond).cpu().numpy()
            err = rel(got, ref)
            print(dtype, rep, "rel", err, "bar", tol)
            assert np.isfinite(got).all()
            assert err < tol, (dtype, rep, err)
        assert e.lib.ldc_debug_lean_launches(RING3) - before >= 20
