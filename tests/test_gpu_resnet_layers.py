"""The ResnetBlock kernels one block at a time against an fp64 reference: the convs with the fused GroupNorm epilogue (conv_device.h
epilogue_gn_fused, conv_lean.inc lean_epilogue_gn), their unfused forms (atomic statistics, launch_gn_stats, launch_gn_apply with
lengths and per-item timesteps), the folded res_conv, the fused y_ln / row partials and the final block's tanh.

Every case goes through ldc_debug_resnet_block: the launches of PlanBuilder::resnet() itself on a private plan, so each option routes as
in a decode.  It returns the block's output, block1's stored output (`mid`), the (sum, sum of squares) per (item, group) of both convs
AS THE KERNELS ACCUMULATED THEM (the granules of the in-launch exchange, or the atomic / launch_gn_stats buffers), and the route.
Reference: tests/resnet_restatement.py, oracle.ldc_oracle.resnet_block restated in float64 (asserted equal to the oracle to 1e-12 per
case), followed by the attention file's block_ref for the (ResnetBlock, attention block) pairs.

Bars -- none comes from a GPU run.
  out, mid, attn_out   bf16: 2 x max|model - exact| + one bf16 ulp of max|exact|, per case and per arrangement (the rounding model of
                       resnet_restatement.py under the route the planner reports for the case, asked before anything is launched);
                       f32: 2e-5 of max|exact|, with the same arithmetic in float32 asserted within a quarter of it on the CPU.
  stats                1e-4 on both engines (the project's bar for fused statistics, ldc_conv_compare): the sum of squares relative, the
                       sum absolute against sqrt(n * sumsq_ref); against the fp64 sums of the conv output on the operands the kernel
                       read: conv 1 on the (bf16-grid) input and the rounded packed weight, conv 2 on the `mid` the GPU stored (itself
                       under its own bar) and the rounded packed weight; rounded to bf16 first where launch_gn_stats reads the stored
                       tensor.  The float32 model is asserted within a quarter of the bar on the CPU.
Power -- asserted per case on the CPU before anything is launched; the mutants never run on the GPU.  Each misses the bar of the
quantity it is aimed at by >= 4x:
  stats  (a) drop_last: the item's last row left out  (b) first_from_prev: the item's first row taken from the neighbour's last row
         (c) leak: the conv's rows outside an item taken from the neighbour instead of zero  (d) all_rows: ragged, the sums over all L rows
  mid    (e) no_plus_one: scale instead of scale + 1  (f) next_ss: the (scale | shift) row of the next block with as many channels
         (g) same_t: per-item plans, every item on item 0's timestep
  out    (h) no_res: the residual omitted  (i) no_res_bias: res_conv's bias omitted  (j) swapped: x1 and x2 swapped  (k) no_tanh
Inputs: Gaussian on the bf16 grid, rows 0, 1, L-2, L-1 and both sides of every multiple of 32 multiplied by 4.  The checkpoint is the
attention file's dim-256 checkpoint with every res_conv bias redrawn at unit scale (the synthetic biases leave (i) invisible under a bf16 bar)
and, for the large-mean case, block1.proj.bias of two groups of two blocks raised to |mean| / std = 4.

Modelled bars and measured errors, relative to max|exact| (MI355X; bars: smallest..largest of out / mid over the cases of the row;
measured: the largest; stats: the measure above, bar 1e-4; mutant: the smallest ratio of a mutant's error to the bar of its quantity).
f32 rows: the bar is 2e-5 throughout.  No case missed a bar.  `stored`: the unfused routes' stored conv outputs against the conv of the
same operands, in bf16 ulps of max|.| (bar 1).

  cases                     route (conv 1, conv 2)       dtype  n    bar out/mid          out       mid       stats     mutant
  every block, default      fused, fused (+ folded res)  bf16   46   8.85e-03..7.02e-02   3.32e-02  4.10e-03  4.62e-06  7.1x
                                                         f32    46                        6.99e-06  2.75e-06  2.78e-07  216x
  length sweep              fused / atomic by the gate   bf16   66   8.89e-03..1.80e-02   5.94e-03  5.20e-03  1.31e-05  6.8x
                                                         f32    66                        2.18e-06  3.08e-06  6.55e-07  92x
  fuse_gn_epi 0             atomic stats + gn_apply      bf16   5    1.12e-02..6.56e-02   3.08e-02  4.90e-03  4.17e-06  8.4x
                                                         f32    5                         6.99e-06  2.75e-06  2.95e-07  268x
  + fuse_gn_stats 0         gn_stats + gn_apply          bf16   5    1.30e-02..6.58e-02   3.09e-02  4.90e-03  3.52e-07  8.4x   stored 0.50
                                                         f32    5                         6.60e-06  2.75e-06  2.60e-07  268x
  fold_res 0                fused, res_conv on its own   bf16   5    9.67e-03..7.02e-02   3.32e-02  4.00e-03  4.34e-06  9.8x
                                                         f32    5                         6.99e-06  2.75e-06  2.37e-07  268x
  conv_lean 0               fused (conv_fast_kernel)     bf16   5    9.67e-03..7.02e-02   3.32e-02  4.00e-03  4.24e-06  9.8x
  dim 32                    atomic stats + gn_apply      bf16   3    1.09e-02..4.53e-02   2.07e-02  4.87e-03  1.24e-05  6.6x
                                                         f32    3                         1.63e-06  6.15e-07  2.89e-07  1062x
  ragged                    gn_stats + gn_apply, lens    bf16   10   1.01e-02..7.72e-02   3.67e-02  5.03e-03  3.04e-07  6.8x   stored 0.50
                                                         f32    10                        6.39e-06  4.65e-06  2.96e-07  4795x
  per-item                  the same, t per item         bf16   10   1.06e-02..7.22e-02   3.42e-02  5.71e-03  2.99e-07  4.4x   stored 0.50
                                                         f32    10                        5.97e-06  3.88e-06  2.99e-07  2755x
  large mean                fused, fused                 bf16   2    9.91e-03..1.45e-02   4.79e-03  2.59e-03  4.62e-06  8.7x
                                                         f32    2                         8.44e-07  1.86e-06  1.88e-07  380x
  pair (4 option states)    fused / atomic               bf16   32   9.88e-03..1.51e-02   4.60e-03  5.28e-03  3.36e-06  7.3x   attn_out 6.97e-03 (bar 1.33e-02..1.88e-02)
                                                         f32    32                        8.61e-07  1.20e-06  2.62e-07  216x   attn_out 8.62e-07
(the largest bars and `out` errors are the final block's: its output is tanh'ed, max|exact| = 1.)

Wall time on an MI355X box: this file's 376 tests take 18 s of the GPU suite's 197 s (1357 tests).
The whole dim-256 UNet on a ragged plan against its items alone (last row of section 5): 5.6e-3 bf16 (bar 4.24e-2), 1.2e-6 f32 (bar 2e-5).

Mutation check of this file (scratch builds, not committed, each run once; both change arithmetic only):
  * lean_epilogue_gn's publish loop leaves out the item's last row where a tile straddles items (`m < hi - 1`): 238 of the 374 block
    cases fail (every default, sweep-fused, large-mean and pair case and the fused fallbacks, both dtypes -- the f32 engine's convs run on the
    lean kernel too); of the existing whole-UNet tests only the lean-against-conv_fast A/B comparison fails, none of the
    reference-pinned bf16 tests of test_gpu_bench_shape.py / test_gpu_parity.py / test_gpu_ragged.py / test_gpu_pool.py does.
  * gn_apply's ragged forms divide by L instead of the item's rows: all 40 ragged / per-item cases fail and no other; this one the
    existing dim-32 ragged and pool tests see as well (15 of their 35 bf16 cases).

What the first runs of this file found.  (1) A ragged plan's planning passes run on a measuring arena where the lengths' address was
null, PlanBuilder::lens() therefore said "not ragged", and those passes planned the equal-length launch forms: on a model whose
ResnetBlocks fuse their GroupNorm apply (channels per group a multiple of 32: the dim-256 model; the dim-32 fixtures never fuse) the
arena of a ragged or per-item plan was measured without the two conv outputs per block its unfused forms store, and the real pass built
past its end.  Fixed in lens(); get_plan and this hook now refuse a plan that outgrows its measure.  Shown by the ragged cases'
planner report (epi1 = epi2 = 0 is asserted before anything runs).  (2) Two mistakes of this file's own reference: the oracle's
float64 weight standardisation rounds to another bf16 value than the engine's float32 fold for about one weight in 10^4, which the
statistics of a one- or two-row item see (1.2e-4 at B = 16, L = 2; 2e-7 with resnet_restatement.packed_fold); and no model predicts
the bf16 roundings of a STORED conv output element for element, so launch_gn_stats is compared with the sums of the tensor it read
(one flipped rounding in a one-row item is 2e-3).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L  # noqa: E402
from ladiffcodec_amd.model import Engine  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402
import resnet_restatement as R  # noqa: E402
from resnet_restatement import ATOMIC, FUSED, GN_STATS  # noqa: E402
from test_gpu_attention_layers import D, F32_TOL, H, U256, U32, bf16_ulp, block_ref, build_engine, err_vs, rbf, sd64_of, sd_c2, sharpen  # noqa: E402

F64 = torch.float64
STATS_TOL = 1e-4
T0 = 417
LARGE_MEAN = {"down1.1": (2, 5), "up3.2": (1, 6)}     # block -> the two groups whose conv-1 mean is raised to 4 std
ROUTES = {}                                            # case id -> info of its run (test_route_coverage)
_S = {}


# ------------------------------------------------------------------------------------------------ checkpoints and engines
def edged(x):
    Ln = x.shape[-1]
    rows = {0, 1, Ln - 2, Ln - 1}
    for m in range(32, Ln, 32):
        rows.update((m - 1, m))
    x = x.clone()
    x[..., sorted(p for p in rows if 0 <= p < Ln)] *= 4
    return x


def make_input(cin, B, Ln, seed):
    g = torch.Generator().manual_seed(seed)
    return rbf(edged(torch.randn(B, cin, Ln, generator=g, dtype=F64)))


def unet_of(tag):
    return U256 if tag == "c2" else U32


def table(tag):
    if ("table", tag) not in _S:
        _S[("table", tag)] = R.block_table(unet_of(tag))
    return _S[("table", tag)]


def state_dict(tag):
    """the numpy checkpoint of the engines of this file (see the module docstring)"""
    if ("sd", tag) in _S:
        return _S[("sd", tag)]
    if tag == "c2":
        base = sd_c2()
    else:
        from helpers import main_sd_np
        base = sharpen(main_sd_np("r84"), U32)
    sd = {k: np.array(v, copy=True) for k, v in base.items()}
    rng = np.random.default_rng(5)
    for k in sorted(sd):
        if k.startswith("diff_model.") and k.endswith(".res_conv.bias"):
            sd[k] = rng.standard_normal(sd[k].shape).astype(np.float32)
    if tag == "c2":   # large mean: the conv-1 bias of two groups raised to 4 x the group's standard deviation on this file's inputs
        sd64 = sd64_of(sd)
        u = unet_of(tag)
        for name, groups in LARGE_MEAN.items():
            rs = table(tag)[name]["rs"]
            W = R.block_weights(sd64, rs)
            h1 = R.conv3(make_input(rs.cin, 3, 37, 99), W["w1"], W["b1"])
            cpg = rs.cout // u.groups
            for gi in groups:
                sl = slice(gi * cpg, (gi + 1) * cpg)
                sd[rs.prefix + ".block1.proj.bias"][sl] += np.float32((-1) ** gi * 4.0 * float(h1[:, sl].std()))
    _S[("sd", tag)] = sd
    return sd


def sd64(tag):
    if ("sd64", tag) not in _S:
        _S[("sd64", tag)] = sd64_of(state_dict(tag))
    return _S[("sd64", tag)]


def eng(tag, dtype):
    if ("eng", tag, dtype) not in _S:
        if tag == "c2":
            e = build_engine(state_dict(tag), dtype)
        else:
            from helpers import CASES, COND_CFG, cond_sd_np
            mc, u, _ = CASES["r84"]
            e = Engine(mc, u, COND_CFG, dtype=dtype)
            e.load_state_dict(L.MODEL_MAIN, state_dict(tag))
            e.load_state_dict(L.MODEL_COND, cond_sd_np())
            e.finalize(strict=True)
        _S[("eng", tag, dtype)] = e
    return _S[("eng", tag, dtype)]


def weights(tag, name, kind):
    """the block's weights in float64 with the oracle's fold ('exact'), as the engines pack them: folded in float32 ('packed') and then
    rounded to bf16 ('bf16'), and the exact ones in float32 for the float32 model ('f32')"""
    key = ("w", tag, name)
    if _S.get("w_key") != key:        # one block at a time: the widest block's three copies are 150 MB
        rs = table(tag)[name]["rs"]
        W = R.block_weights(sd64(tag), rs)
        _S["w_key"], _S["w"] = key, dict(exact=W, bf16=R.block_weights(sd64(tag), rs, rbf, R.packed_fold), packed=R.block_weights(sd64(tag), rs, fold=R.packed_fold),
                                          f32={k: (v.float() if v is not None else None) for k, v in W.items()})
    return _S["w"][kind]


# ------------------------------------------------------------------------------------------------ a case on the CPU
def arrangement(info):
    """the rounding arrangement (resnet_restatement) of the route the planner reports"""
    unfused = ATOMIC if info["fuse_stats"] else GN_STATS
    return (FUSED if info["epi1"] else unfused, FUSED if info["epi2"] else unfused)


def level_rows(lens, shift):
    return None if lens is None else [int(v) >> shift for v in lens]


_CASES = {}


def make_case(tag, name, B, Ln, lens=None, shift=0, t_items=None, seed=0):
    """inputs, exact result, the float32 model's errors and the mutants' errors -- CPU only; the bf16 model and its bars per
    arrangement: model_of"""
    key = (tag, name, B, Ln, tuple(lens) if lens is not None else None, shift, tuple(t_items) if t_items is not None else None, seed)
    if key in _CASES:
        return _CASES[key]
    u, sd, bt = unet_of(tag), sd64(tag), table(tag)[name]
    rs, final, g = bt["rs"], bt["final"], unet_of(tag).groups
    rows = level_rows(lens, shift)
    x = make_input(rs.cin, B, Ln, 1000 * Ln + 7 * B + seed + len(name))
    tt = list(t_items) if t_items is not None else [T0]
    sc, sh = R.scale_shift(sd, u, rs, tt)
    W = weights(tag, name, "exact")
    ex = R.resnet_ref(W, x, sc, sh, g, lens=rows, final=final)
    # the restatement is the oracle's arithmetic: items alone, cut to their lengths, through oracle.resnet_block
    temb = O.time_embedding(sd, u, torch.as_tensor(tt, dtype=F64), "diff_model")
    for b in (sorted({0, B - 1}) if (rows is None and t_items is None) else range(B)):
        nb = Ln if rows is None else rows[b]
        o = O.resnet_block(sd, rs, x[b:b + 1, :, :nb], temb[b:b + 1] if t_items is not None else temb, g)
        o = torch.tanh(o) if final else o
        assert err_vs(ex["out"][b:b + 1, :, :nb], o) < 1e-12, (name, b)
    m32 = R.resnet_ref(weights(tag, name, "f32"), x.float(), sc.float(), sh.float(), g, lens=rows, final=final)
    f32_err = {q: err_vs(m32[q], ex[q]) for q in ("mid", "out")}
    f32_err["stats"] = max(R.stats_err(m32["s1"], ex["s1"], ex["n"]), R.stats_err(m32["s2"], ex["s2"], ex["n"]))
    # ---- mutants ----
    mut = {"stats": {}, "mid": {}, "out": {}}
    ragged = rows is not None and min(rows) < Ln
    for m in ("drop_last",) + (("first_from_prev", "leak") if B >= 2 else ()) + (("all_rows",) if ragged else ()):
        errs = []
        for h, s, src, w in (("h1", "s1", x * ex["vm"], W["w1"]), ("h2", "s2", ex["mid"], W["w2"])):
            hm = ex[h] + R.leak_delta(src, w) if m == "leak" else ex[h]
            errs.append(R.stats_err(R.group_sums(hm, g, ex["valid"], None if m == "leak" else m), ex[s], ex["n"]))
        mut["stats"][m] = min(errs)
    mid_of = lambda s_, h_: F.silu(ex["y1"] * s_ + h_) * ex["vm"]   # noqa: E731
    mut["mid"]["no_plus_one"] = err_vs(mid_of(sc, sh), ex["mid"])
    names = list(table(tag))
    i = names.index(name)
    peer = next(k for k in names[i + 1:] + names[:i] if table(tag)[k]["rs"].cout == rs.cout)
    sc2, sh2 = R.scale_shift(sd, u, table(tag)[peer]["rs"], tt)
    mut["mid"]["next_ss"] = err_vs(mid_of(sc2 + 1, sh2), ex["mid"])
    if t_items is not None:
        mut["mid"]["same_t"] = err_vs(mid_of(sc[:1] + 1, sh[:1]), ex["mid"])
    fin = (lambda t: torch.tanh(t)) if final else (lambda t: t)
    mut["out"]["no_res"] = err_vs(fin(ex["act2"]) * ex["vm"], ex["out"])
    if rs.has_res_conv:
        mut["out"]["no_res_bias"] = err_vs(fin(ex["act2"] + ex["res"] - W["br"][None, :, None]) * ex["vm"], ex["out"])
    if bt["cin2"]:   # (in float32: a whole chain more, and the mutant's error is far above float32's)
        xs = torch.cat((x[:, bt["cin1"]:], x[:, :bt["cin1"]]), 1).float()
        mut["out"]["swapped"] = err_vs(R.resnet_ref(weights(tag, name, "f32"), xs, sc.float(), sh.float(), g, lens=rows, final=final)["out"], ex["out"])
    if final:
        mut["out"]["no_tanh"] = err_vs((ex["act2"] + ex["res"]) * ex["vm"], ex["out"])
    case = dict(tag=tag, name=name, x=x, ex=ex, sc=sc, sh=sh, f32_err=f32_err, mut=mut, rows=rows, bt=bt, models={})
    if len(_CASES) > 3:
        _CASES.pop(next(iter(_CASES)))
    _CASES[key] = case
    return case


def model_of(case, arr):
    """the bf16 rounding model of the case under an arrangement and the bars it gives: (model, {mid, out})"""
    if arr not in case["models"]:
        ex, bt = case["ex"], case["bt"]
        mo = R.resnet_ref(weights(case["tag"], case["name"], "bf16"), case["x"], case["sc"], case["sh"], unet_of(case["tag"]).groups, r=rbf,
                          arr=arr, lens=case["rows"], final=bt["final"])
        bars = {}
        for q in ("mid", "out"):
            mx = float(ex[q].abs().max())
            bars[q] = 2.0 * err_vs(mo[q], ex[q]) + bf16_ulp(mx) / mx
        case["models"][arr] = (mo, bars)
    return case["models"][arr]


def tolerances(dtype, case, arr):
    if dtype == "bf16":
        return dict(model_of(case, arr)[1], stats=STATS_TOL)
    return dict(mid=F32_TOL, out=F32_TOL, stats=STATS_TOL)


def check_cpu(case, tol):
    """the float32 model within a quarter of the f32 bars; every mutant outside 4 x the bar of the quantity it is aimed at"""
    for q in ("mid", "out", "stats"):
        assert case["f32_err"][q] <= 0.25 * (STATS_TOL if q == "stats" else F32_TOL), ("float32 model", q, case["f32_err"][q])
        for m, e in case["mut"][q].items():
            assert e >= 4.0 * tol[q], f"mutant {m} is within 4x of the {q} bar: {e:.3e} vs {tol[q]:.3e}"


# ------------------------------------------------------------------------------------------------ a case on the GPU
def run_case(tag, dtype, name, B, Ln, label, lens=None, shift=0, t_items=None, expect=None, with_attention=False, seed=0):
    e = eng(tag, dtype)
    plan = e.debug_resnet_route(name, B, Ln, lens=lens, shift=shift, per_item=t_items is not None, with_attention=with_attention)
    for k, v in (expect or {}).items():
        assert plan[k] == v, f"{label} {name}: the planner reports {k} = {plan[k]}, the case is meant for {v} ({plan})"
    case = make_case(tag, name, B, Ln, lens, shift, t_items, seed)
    tol = tolerances(dtype, case, arrangement(plan))
    check_cpu(case, tol)
    bt, ex = case["bt"], case["ex"]
    x = case["x"].float()
    x1, x2 = (x[:, :bt["cin1"]], x[:, bt["cin1"]:]) if bt["cin2"] else (x, None)
    got = e.debug_resnet_block(name, x1.cuda(), x2.cuda() if x2 is not None else None, t=T0, lens=lens, shift=shift, t_items=t_items,
                               with_attention=with_attention)
    info = got["info"]
    ROUTES[(tag, dtype, label, name, B, Ln)] = dict(info, L=Ln, B=B, final=bt["final"], has_res=bt["rs"].has_res_conv)
    out, mid, stats = got["out"].cpu().to(F64), got["mid"].cpu().to(F64), torch.from_numpy(got["stats"]).to(F64)
    # the statistics against the fp64 sums of the conv outputs on the operands the kernels read; where launch_gn_stats reads the STORED
    # conv output (whose bf16 roundings no model predicts element for element), against the sums of that tensor, itself held to one
    # bf16 ulp of max|.| (f32: the f32 bar) against the conv of the same operands
    r = rbf if dtype == "bf16" else R.ident
    arr = arrangement(info)
    Wk = weights(tag, name, "bf16" if dtype == "bf16" else "packed")
    g = unet_of(tag).groups
    pre = got["pre"].cpu().to(F64)
    hs = (R.conv3(case["x"] * ex["vm"], Wk["w1"], Wk["b1"]), R.conv3(mid, Wk["w2"], Wk["b2"]))
    refs, pre_err = [], 0.0
    for k in (0, 1):
        if arr[k][0]:     # launch_gn_stats
            mx = float(hs[k].abs().max())
            pre_err = max(pre_err, float(((pre[k] - hs[k]) * ex["vm"]).abs().max() / mx) / (bf16_ulp(mx) / mx if dtype == "bf16" else F32_TOL))
            refs.append(R.group_sums(pre[k], g, ex["valid"]))
        else:
            refs.append(R.group_sums(hs[k], g, ex["valid"]))
    err = dict(out=err_vs(out, ex["out"]), mid=err_vs(mid, ex["mid"]),
               stats=max(R.stats_err(stats[0], refs[0], ex["n"]), R.stats_err(stats[1], refs[1], ex["n"])))
    mm = {q: min(v / tol[q] for v in case["mut"][q].values()) for q in ("out", "mid", "stats")}
    route = "".join("F" if info[k] else ("a" if info["fuse_stats"] else "s") for k in ("epi1", "epi2")) + ("+fold" if info["folded"] else "")
    print(f"RESNET {dtype} {label} {name} B={B} L={Ln} route={route} bm={info['bm1']}/{info['bm2']} "
          + " ".join(f"{q}={err[q]:.2e}/{tol[q]:.2e}" for q in ("out", "mid", "stats")) + f" minmut={min(mm.values()):.1f}x" + (f" stored={pre_err:.2f}ulp" if pre_err else ""))
    assert {k: info[k] for k in plan} == plan, ("the run took another route than the planner reported", info, plan)
    if info["epi1"] or info["epi2"]:
        assert info["tags_complete"] == 1 and info["stray_slots"] == 0, info
    if case["rows"] is not None:
        pad = ~ex["valid"][:, None, :].expand_as(out)
        assert bool((out[pad] == 0).all()) and bool((mid[pad] == 0).all()), "a padding row of out / mid is not exactly zero"
    assert pre_err <= 1.0, ("a stored conv output is further than the format allows from the conv of its operands", pre_err)
    for q in ("stats", "mid", "out"):
        assert err[q] <= tol[q], (dtype, label, name, B, Ln, q, err[q], tol[q])
    return case, got


ALL = list(R.block_table(U256))
assert len(ALL) == 23


# ------------------------------------------------------------------------------------------------ 1. every block, default options
@pytest.mark.parametrize("dtype", ["bf16", "f32"])      # (the first decorator varies fastest: both engines share a case's CPU work)
@pytest.mark.parametrize("B,Ln", [(3, 37), (13, 75)])
@pytest.mark.parametrize("name", ALL)
def test_every_block_against_fp64(dtype, name, B, Ln):
    """L = 37 puts three items into a 64-row tile; 13 x 75 rows are no multiple of any tile"""
    run_case("c2", dtype, name, B, Ln, "default", expect=dict(epi1=1, epi2=1))


# ------------------------------------------------------------------------------------------------ 2. lengths around the tile gate
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("Ln", [1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 150])
@pytest.mark.parametrize("name", ["down0.1", "up0.1"])
def test_length_sweep_around_the_tile_gate(dtype, name, B, Ln):
    """the fused epilogue is taken exactly where the tile is no taller than two items (t[0] <= 2 * L), per conv"""
    case, got = run_case("c2", dtype, name, B, Ln, "sweep")
    info = got["info"]
    for k in ("1", "2"):
        assert info["epi" + k] == int(0 < info["bm" + k] <= 2 * Ln), (Ln, info)


# ------------------------------------------------------------------------------------------------ 3. fallbacks
FALLBACKS = {"fuse_gn_epi": (("fuse_gn_epi",), dict(epi1=0, epi2=0, fuse_stats=1)),
             "fuse_gn_stats": (("fuse_gn_epi", "fuse_gn_stats"), dict(epi1=0, epi2=0, fuse_stats=0)),
             "fold_res": (("fold_res",), dict(folded=0)),
             "conv_lean": (("conv_lean",), dict(epi1=1, epi2=1))}


@pytest.mark.parametrize("dtype,option", [(d, o) for o in FALLBACKS for d in ("bf16", "f32") if not (d == "f32" and o == "conv_lean")])
@pytest.mark.parametrize("name", ["down0.1", "down2.2", "up0.1", "up4.2", "final"])
def test_fallback_arrangements(dtype, option, name):
    """fuse_gn_epi 0 (the recovery after [gn_wait]: conv + atomic statistics + gn_apply), + fuse_gn_stats 0 (launch_gn_stats),
    fold_res 0 (res_conv as its own launch on the side stream), conv_lean 0 (conv_fast_kernel's epilogue)"""
    e = eng("c2", dtype)
    offs, expect = FALLBACKS[option]
    try:
        for o in offs:
            e.set_option(o, 0)
        run_case("c2", dtype, name, 13, 75, option + "=0", expect=expect)
    finally:
        for o in offs:
            e.set_option(o, 1)


# ------------------------------------------------------------------------------------------------ 4. dim 32: never fused
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["down0.1", "up1.2", "final"])
def test_dim32_blocks_take_the_unfused_forms(dtype, name):
    """4 and 8 channels per group: no fused epilogue; atomic statistics by the power-of-two rule"""
    cpg = table("d32")[name]["rs"].cout // U32.groups
    run_case("d32", dtype, name, 3, 37, "dim32", expect=dict(epi1=0, epi2=0, fuse_stats=int(cpg >= 4 and cpg & (cpg - 1) == 0)))


# ------------------------------------------------------------------------------------------------ 5. ragged and per-item plans
def ragged_lens(B, Ln, shift):
    """level-0 lengths: the full length, 1 row, odd lengths, and (odd items) lengths that lose a row under >> shift"""
    rows = [Ln, 1, Ln - 6, 2, 32, 33, 31, Ln - 1, 17, 5, 8, Ln - 2, 3][:B]
    return [(min(max(r_, 1), Ln) << shift) + ((1 << shift) - 1 if b % 2 and min(max(r_, 1), Ln) < Ln else 0) for b, r_ in enumerate(rows)]


RAGGED = [("final", 0), ("down1.1", 1), ("up3.2", 1), ("down2.2", 2), ("up2.1", 2)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("per_item", [False, True])
@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("name,shift", RAGGED)
def test_ragged_and_per_item_plans(dtype, name, shift, B, per_item):
    """valid rows within the bars, statistics over the valid rows only, every padding row of out and mid exactly zero"""
    Ln = 37
    lens = ragged_lens(B, Ln, shift)
    assert lens[0] >> shift == Ln and lens[1] >> shift == 1 and any((v >> shift) % 2 for v in lens[2:]) and (shift == 0 or any(v & ((1 << shift) - 1) for v in lens))
    t_items = [(0, 500, 999, 250, 750)[b % 5] for b in range(B)] if per_item else None
    run_case("c2", dtype, name, B, Ln, "per_item" if per_item else "ragged", lens=lens, shift=shift, t_items=t_items,
             expect=dict(epi1=0, epi2=0, fuse_stats=0))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ragged_unet_of_the_dim256_model_equals_its_items_alone(dtype):
    """The whole UNet on a ragged plan of the model whose ResnetBlocks fuse their GroupNorm apply (the ragged tests' dim-32 fixtures
    never do): every item against the engine's own equal-length call on it alone, under the bar test_gpu_ragged.py holds that
    comparison to (f32: 2e-5, the bar of the fused against the separate GroupNorm apply).  Before PlanBuilder::lens() was fixed this
    plan was measured for the fused forms and built for the unfused ones; get_plan now refuses such a plan."""
    from drift_tolerances import TOL
    e = eng("c2", dtype)
    Lmax, lens, up = 160, [160, 80, 80], 10
    g = torch.Generator().manual_seed(3)
    x, cond = torch.randn(3, 128, Lmax, generator=g), torch.randn(3, 128, Lmax // up, generator=g)
    got = e.unet_forward_ragged(x.cuda(), 37, cond.cuda(), lens).cpu()
    tol = TOL["bf16"]["eps_small"] if dtype == "bf16" else F32_TOL
    for b, n in enumerate(lens):
        own = e.unet_forward(x[b:b + 1, :, :n].contiguous().cuda(), 37, cond[b:b + 1, :, :n // up].contiguous().cuda()).cpu()
        err = err_vs(got[b:b + 1, :, :n], own.to(F64))
        print(f"RESNET_RAGGED_UNET {dtype} item {b} len {n} err={err:.2e}/{tol:.2e}")
        assert err <= tol, (dtype, b, err, tol)
        assert not got[b, :, n:].any()


# ------------------------------------------------------------------------------------------------ 6. large mean
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(LARGE_MEAN))
def test_large_mean_groups(dtype, name):
    """|mean| / std = 4 in two groups of conv 1: the one-pass variance sumsq / n - mean^2 with a mean that matters (weight
    standardisation leaves 0.03 .. 0.08 on the synthetic checkpoints)"""
    case, _ = run_case("c2", dtype, name, 3, 37, "large_mean", expect=dict(epi1=1, epi2=1))
    ex = case["ex"]
    mean = ex["s1"][..., 0] / ex["n"][:, None]
    std = (ex["s1"][..., 1] / ex["n"][:, None] - mean * mean).sqrt()
    ratio = (mean.abs() / std)[:, list(LARGE_MEAN[name])]
    assert 3.0 <= float(ratio.min()) and float(ratio.max()) <= 5.5, ratio


# ------------------------------------------------------------------------------------------------ 7. the block and its attention block
PAIRS = {"default": ((), dict(rowstat=1, y_ln=0)),                    # the PreNorm folded into to_qkv on the fused epilogue's row partials
         "fold_ln": (("fold_ln",), dict(rowstat=0, y_ln=1, epi2=1)),   # fused epilogue, then launch_ln_rows writes the PreNorm output
         "fuse_gn_epi": (("fuse_gn_epi",), dict(rowstat=0, y_ln=1, epi2=0)),   # gn_apply writes y_ln on the way
         "fuse_ln": (("fold_ln", "fuse_ln"), dict(rowstat=0, y_ln=0))}  # the attention block's own LayerNorm launch


@pytest.mark.parametrize("dtype,option", [(d, o) for o in PAIRS for d in ("bf16", "f32")])
@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("name", ["down0.2", "down4.2", "mid.1", "up2.2"])
def test_block_with_its_attention_block(dtype, option, name, B):
    """the block and the attention block behind it, built as a step pairs them: default options, fold_ln 0, fuse_gn_epi 0 (y_ln from
    gn_apply itself) and fuse_ln 0"""
    e = eng("c2", dtype)
    offs, expect = PAIRS[option]
    try:
        for o in offs:
            e.set_option(o, 0)
        pair_case(e, dtype, name, B, 37, "pair " + (option + "=0" if offs else option), expect)
    finally:
        for o in offs:
            e.set_option(o, 1)


def pair_case(e, dtype, name, B, Ln, label, expect):
    case, got = run_case("c2", dtype, name, B, Ln, label, expect=expect, with_attention=True)
    p, linear = case["bt"]["attn"]
    sd = sd64("c2")
    exact = (O.linear_attention if linear else O.full_attention)(sd, p, case["ex"]["out"], H, D)
    kk = torch.einsum("ck,bkn->bcn", sd[p + ".fn.fn.to_qkv.weight"][128:256, :, 0], O.channel_layernorm(case["ex"]["out"], sd[p + ".fn.norm.g"]))
    assert float(kk.abs().max()) < 20.0
    assert err_vs(block_ref(sd, p, case["ex"]["out"], linear), exact) < 1e-12
    mx = float(exact.abs().max())
    tol = 2.0 * err_vs(block_ref(sd, p, model_of(case, arrangement(got["info"]))[0]["out"], linear, r=rbf), exact) + bf16_ulp(mx) / mx if dtype == "bf16" else F32_TOL
    err = err_vs(got["attn_out"].cpu(), exact)
    print(f"RESNET_PAIR {dtype} {label} {name} B={B} L={Ln} attn_out={err:.2e}/{tol:.2e}")
    assert err <= tol, (dtype, label, name, B, err, tol)


# ------------------------------------------------------------------------------------------------ 8. what ran
def test_route_coverage():
    """every arrangement the file is about was really taken by a run of this session (under a -k selection the planner's reports for
    one case of each kind stand in, which the runs above assert equal to the run's own)"""
    def planned(tag, dtype, name, B, Ln, opts=(), **kw):
        e = eng(tag, dtype)
        try:
            for o in opts:
                e.set_option(o, 0)
            info = e.debug_resnet_route(name, B, Ln, **kw)
        finally:
            for o in opts:
                e.set_option(o, 1)
        bt = table(tag)[name]
        return dict(info, L=Ln, B=B, final=bt["final"], has_res=bt["rs"].has_res_conv)
    recs = list(ROUTES.values())
    if len(recs) < 373:     # not every one of the 373 block cases above has run in this session
        recs += [planned("c2", "bf16", "down0.1", 16, 33), planned("c2", "bf16", "up0.1", 13, 75), planned("c2", "bf16", "up0.1", 13, 75, ("fold_res",)),
                planned("c2", "bf16", "final", 13, 75, ("fuse_gn_epi",)), planned("c2", "bf16", "final", 13, 75, ("fuse_gn_epi", "fuse_gn_stats")),
                planned("c2", "bf16", "down0.2", 3, 37, with_attention=True),
                planned("c2", "bf16", "down0.2", 3, 37, ("fold_ln", "fuse_gn_epi"), with_attention=True), planned("c2", "f32", "final", 3, 37)]

    def three_items(r_, k):   # a tile of conv k that holds rows of three items
        bm, Ln, B = r_["bm" + k], r_["L"], r_["B"]
        return r_["epi" + k] and any((min(m0 + bm, B * Ln) - 1) // Ln - m0 // Ln >= 2 for m0 in range(0, B * Ln, bm))
    assert any(r_["epi1"] for r_ in recs) and any(r_["epi2"] for r_ in recs)
    assert any(r_["folded"] for r_ in recs) and any(r_["has_res"] and not r_["folded"] for r_ in recs)
    assert any(not r_["epi1"] and r_["fuse_stats"] for r_ in recs), "atomic statistics"
    assert any(not r_["epi1"] and not r_["fuse_stats"] for r_ in recs), "launch_gn_stats"
    assert any(three_items(r_, "1") for r_ in recs) and any(three_items(r_, "2") for r_ in recs)
    assert any(r_["y_ln"] for r_ in recs) and any(r_["rowstat"] for r_ in recs)
    assert any(r_["final"] and r_["epi2"] for r_ in recs) and any(r_["final"] and not r_["epi2"] for r_ in recs), "final's tanh, fused and in gn_apply"
