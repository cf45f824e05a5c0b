"""The attention kernels one layer at a time against an fp64 reference (attention.hip, conv_lean.inc: lean_epilogue_qkv_ctx).

Core level (ldc_debug_attn_core): qkv on the bf16 grid -> the four launch arrangements of a plan
  linattn             launch_linattn, own column-max pass          linattn_kmax_fused   the maxima prepared as to_qkv's epilogue leaves them
  linattn_ctx_tail    launch_linattn_ctx + launch_linattn_tail     attn_full            the bottleneck's softmax attention
against the arithmetic of oracle.ldc_oracle.linear_attention / full_attention between to_qkv and to_out in float64.
Block level (ldc_debug_attention_block): Residual(PreNorm(.)) of the dim-256 UNet's levels through the plan builder's own attention(),
default options and each off-switch (fold_ctx, fuse_attn_tail, fuse_kmax, fold_ln), against those oracle functions on a float64
state dict.

Tolerances.  f32 engine: 2e-5 of max|reference| (the bar of the fp32 kernels with fast exp, test_slstm_all_kernel_variants).
bf16 engine: NOT from a GPU run.  The rounding model (the r argument of lin_core, full_core, tail, block_ref) is the fp64 reference with a round-to-bf16 where the kernels store a value
or feed the MFMA in bf16 (p = exp(k - max), v, ctx' = ctx / ksum * scale, the q softmax, the core's output, to_out's operands, the
block's qkv rows and its output); the bar of a case is 2 x max|model - exact| + one bf16 ulp of max|exact| (2: fp32 summation order
and __expf), computed on the CPU per case.

Power.  A position dropped from a 1200-long softmax is invisible under a bf16 bar on Gaussian data, so every case plants sentinels
(positions 0, L-1, both sides of the multiples of 32 up to 256 and of the last 32- and 64-row tile boundary: +8 on four k columns,
v = +-3) and asserts on the CPU, before the GPU is touched, that three mutants of the fp64 reference miss the case's bar by >= 4x:
(a) the last position of item 0 omitted, (b) item 1's first position attributed to item 0 (B >= 2), (c) `scale` omitted (not for
softmax attention at L = 1, where it changes nothing) -- while max|k| < 20.  The mutants never run on the GPU.

Modelled bars and measured errors, relative to max|exact| (MI355X; bars: smallest..largest over the cases of the row, measured: the
largest).  Core rows: L in {75 .. 1200} x B in {1, 3, 16} and the ragged L in {1, 31, 33, 53, 77, 127, 129, 560} at B = 3; block
rows: every level of the dim-256 UNet at B in {3, 13} (off-switches: B = 13).  No case missed its modelled bar.  The f32 figures move in
their second digit from run to run (fp32 atomics).

  level  arrangement           kernels                 bf16 bar (model)       bf16 measured   f32 measured (bar 2e-5)
  core   linattn               ctx_mfma + out_mfma     1.08e-02..2.21e-02     8.17e-03        1.03e-06
  core   linattn_kmax_fused    ctx_mfma + out_mfma     1.08e-02..2.21e-02     8.17e-03        9.73e-07
  core   linattn_ctx_tail      ctx_mfma + tail_mfma    9.57e-03..1.49e-02     3.64e-03        (bf16 only)
  core   attn_full             attn_full_kernel        5.21e-03..1.05e-02     2.62e-03        1.93e-06
  block  default               linear levels           1.15e-02..1.72e-02     5.04e-03        7.86e-07
  block  default               mid (attn_full)         1.76e-02..2.12e-02     6.47e-03        1.74e-06
  block  fold_ctx 0            linear levels           1.20e-02..1.30e-02     4.58e-03        (bf16 only)
  block  fuse_attn_tail 0      linear levels           1.20e-02..1.30e-02     5.43e-03        (bf16 only)
  block  fuse_kmax 0           linear levels           1.20e-02..1.30e-02     5.43e-03        7.86e-07
  block  fold_ln 0             linear levels / mid     1.20e-02..2.12e-02     7.92e-03        8.96e-07
  block  dim 32 (no tail)      linear levels / mid     1.34e-02..1.80e-02     5.31e-03        5.13e-07
  k-range block, default (fails with [ctx_range], recovered through fold_ctx 0)
                                                       1.31e-02..1.38e-02     3.49e-03        2.61e-07
  k-range block, fold_ctx 0 / fuse_attn_tail 0 / fuse_kmax 0
                                                       1.31e-02..1.38e-02     4.01e-03        -
  k-range core  linattn / linattn_kmax_fused           1.28e-02..1.51e-02     4.78e-03        1.39e-06
  k-range core  linattn_ctx_tail                       1.01e-02..1.06e-02     3.16e-03        (bf16 only)

Mutation check of this file (not committed): with lean_epilogue_qkv_ctx's `in` test ignoring `hi`, 20 of the 22 bf16 default block cases
fail (all but the two of `mid`); with linattn_ctx_mfma_kernel's column sum one 8-wide piece short, 57 of the 69 bf16 linattn core cases.

k-range contract (section 3 of the module): a block input whose fp64 reference is finite either comes back within the case's bar or
fails with LDC_E_HIP and "device-side failure [ctx_range]", and sample.apply_device_fallback recovers through fold_ctx 0.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, spec, synth  # noqa: E402
from ladiffcodec_amd.model import Engine  # noqa: E402
from ladiffcodec_amd.spec import CodecConfig, UnetConfig  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402
from gpu_common import engine  # noqa: E402

H, D, HD = 4, 32, 128
SCALE = D ** -0.5
F32_TOL = 2e-5
F64 = torch.float64


def rbf(t):
    """round to nearest even onto the bf16 grid, back in float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def ident(t):
    return t


def bf16_ulp(m):
    return 2.0 ** (math.floor(math.log2(m)) - 7) if m > 0 else 0.0


def err_vs(got, exact):
    """max |got - exact| / max |exact|; anything not finite is an infinite error"""
    got = got.to(F64)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - exact).abs().max() / exact.abs().max())


# ------------------------------------------------------------------------------------------------ inputs
def sentinel_positions(Ln):
    s = {0, Ln - 1}
    for m in range(32, 257, 32):
        s.update((m - 1, m))
    for tile in (32, 64):
        t = (Ln // tile) * tile
        s.update((t - 1, t))
    return sorted(p for p in s if 0 <= p < Ln)


def make_qkv(B, Ln, seed):
    """Gaussian qkv [B, 384, L] on the bf16 grid with the sentinels planted in every item"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * HD, Ln, generator=g, dtype=F64)
    k = qkv[:, HD:2 * HD].reshape(B, H, D, Ln)
    v = qkv[:, 2 * HD:].reshape(B, H, D, Ln)
    e = torch.arange(D)
    for i, n in enumerate(sentinel_positions(Ln)):
        cols = [(3 * i + 8 * j) % D for j in range(4)]
        k[:, :, cols, n] += 8.0
        pat = 3.0 * torch.where(((e + i) // (1 + i % 3)) % 2 == 0, 1.0, -1.0).to(F64)
        for b in range(B):                                   # the sign alternates from item to item: a neighbour's position is not a duplicate
            v[b, :, :, n] = pat if b % 2 == 0 else -pat
    return rbf(qkv)


# ------------------------------------------------------------------------------------------------ fp64 reference, rounding model, mutants
def split_heads(qkv):
    B, _, Ln = qkv.shape
    return tuple(t.reshape(B, H, D, Ln) for t in qkv.chunk(3, dim=1))


def lin_core(qkv, r=ident, mutant=None):
    """oracle.linear_attention between to_qkv and to_out; r rounds where linattn_ctx_mfma_kernel / linattn_out_mfma_kernel do"""
    q, k, v = split_heads(qkv)
    B, Ln = q.shape[0], q.shape[3]
    qs = r(q.softmax(dim=-2))
    outs = []
    for b in range(B):
        kb, vb = k[b], v[b]
        if mutant == "drop_last" and b == 0:
            kb, vb = kb[..., :-1], vb[..., :-1]
        if mutant == "leak_next" and b == 0 and B > 1:
            kb, vb = torch.cat((kb, k[1][..., :1]), -1), torch.cat((vb, v[1][..., :1]), -1)
        if kb.shape[-1] == 0:
            outs.append(torch.full((H, D, Ln), float("nan"), dtype=F64))
            continue
        p = r(torch.exp(kb - kb.amax(dim=-1, keepdim=True)))
        ctx = torch.einsum("hdn,hen->hde", p, r(vb)) / p.sum(-1)[..., None]
        ctx = r(ctx if mutant == "no_scale" else ctx * SCALE)
        outs.append(r(torch.einsum("hde,hdn->hen", ctx, qs[b])))
    return torch.stack(outs).reshape(B, HD, Ln)


def full_core(qkv, r=ident, mutant=None):
    """oracle.full_attention between to_qkv and to_out; attn_full_kernel computes in fp32 from the stored rows and rounds its output"""
    q, k, v = split_heads(qkv)
    B, Ln = q.shape[0], q.shape[3]
    outs = []
    for b in range(B):
        kb, vb = k[b], v[b]
        if mutant == "drop_last" and b == 0:
            kb, vb = kb[..., :-1], vb[..., :-1]
        if mutant == "leak_next" and b == 0 and B > 1:
            kb, vb = torch.cat((kb, k[1][..., :1]), -1), torch.cat((vb, v[1][..., :1]), -1)
        if kb.shape[-1] == 0:
            outs.append(torch.full((H, D, Ln), float("nan"), dtype=F64))
            continue
        sim = torch.einsum("hdi,hdj->hij", q[b] if mutant == "no_scale" else q[b] * SCALE, kb)
        outs.append(r(torch.einsum("hij,hdj->hdi", sim.softmax(dim=-1), vb)))
    return torch.stack(outs).reshape(B, HD, Ln)


def ln_c(x, g):
    return O.channel_layernorm(x, g)


def tail(core, w, b, g, resid, r=ident):
    """to_out 1x1 conv + bias, channel LayerNorm, + x (unet.py:216-222): linattn_tail_mfma_kernel's phases 2 and 3"""
    y = torch.einsum("ck,bkn->bcn", r(w), core) + b[None, :, None]
    return r(ln_c(y, g[None, :, None]) + resid)


MUTANTS = ("drop_last", "leak_next", "no_scale")
_CASES = {}


def tail_params(B, Ln, C, core_exact, seed):
    """to_out weight / bias / gain / residual on the bf16 grid; the bias is as large as the conv's output, so that a wrong `scale`
    survives the LayerNorm behind it"""
    g = torch.Generator().manual_seed(seed + 1)
    w = rbf(torch.randn(C, HD, generator=g, dtype=F64) / math.sqrt(HD))
    sd = float(torch.einsum("ck,bkn->bcn", w, core_exact).std())
    b = rbf(torch.randn(C, generator=g, dtype=F64) * sd)
    gain = rbf(1.0 + 0.25 * torch.randn(C, generator=g, dtype=F64))
    resid = rbf(torch.randn(B, C, Ln, generator=g, dtype=F64))
    return w, b, gain, resid


def core_case(kind, B, Ln, C=256):
    """inputs, fp64 result, modelled bf16 bar and the mutants' errors of one core case -- CPU only"""
    key = ("full" if kind == "attn_full" else ("tail" if kind == "linattn_ctx_tail" else "lin"), B, Ln, C)
    if key in _CASES:
        return _CASES[key]
    qkv = make_qkv(B, Ln, 1000 * Ln + B)
    assert float(qkv[:, HD:2 * HD].abs().max()) < 20.0
    core = full_core if key[0] == "full" else lin_core
    tp = None
    if key[0] == "tail":
        tp = tail_params(B, Ln, C, lin_core(qkv), 7 * Ln + B)
        fn = lambda r=ident, mutant=None: tail(lin_core(qkv, r, mutant), *tp, r=r)   # noqa: E731
    else:
        fn = lambda r=ident, mutant=None: core(qkv, r, mutant)   # noqa: E731
    exact = fn()
    mx = float(exact.abs().max())
    bar = 2.0 * err_vs(fn(r=rbf), exact) + bf16_ulp(mx) / mx
    # (b) needs a second item; (c) does not exist for softmax attention over a single key (the one weight is 1 whatever the scale)
    mut = {m: err_vs(fn(mutant=m), exact) for m in MUTANTS if not (m == "leak_next" and B < 2) and not (m == "no_scale" and key[0] == "full" and Ln == 1)}
    case = dict(qkv=qkv, tp=tp, exact=exact, bar=bar, mut=mut)
    if len(_CASES) > 6:
        _CASES.pop(next(iter(_CASES)))
    _CASES[key] = case
    return case


def check_power(case, tol):
    for m, e in case["mut"].items():
        assert e >= 4.0 * tol, f"mutant {m} is within 4x of the bar: {e:.3e} vs {tol:.3e}"


# ------------------------------------------------------------------------------------------------ 1. core kernels
GRID = [(B, Ln) for Ln in (75, 150, 300, 600, 1200) for B in (1, 3, 16)]
RAGGED = [(3, Ln) for Ln in (1, 31, 33, 53, 77, 127, 129, 560)]
KINDS = ("linattn", "linattn_kmax_fused", "linattn_ctx_tail", "attn_full")


def run_core(e, kind, case):
    to_out = None
    if kind == "linattn_ctx_tail":
        w, b, g, resid = case["tp"]
        to_out = (w.numpy(), b.numpy(), g.numpy(), resid.float().cuda())
    return e.debug_attn_core(kind, case["qkv"].float().cuda(), to_out).cpu()


@pytest.mark.parametrize("B,Ln", GRID + RAGGED)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_attention_core_against_fp64(dtype, kind, B, Ln):
    if kind == "linattn_ctx_tail" and dtype == "f32":
        with pytest.raises(L.LdcError):     # the fused tail is a bf16 kernel: a missing kernel is an error, not a fallback
            engine("r84", "f32").debug_attn_core(kind, torch.zeros(1, 3 * HD, 8), (np.zeros((256, HD)), np.zeros(256), np.zeros(256), torch.zeros(1, 256, 8)))
        return
    C = (256, 512, 1024)[(B + Ln) % 3]
    case = core_case(kind, B, Ln, C)
    tol = case["bar"] if dtype == "bf16" else F32_TOL
    check_power(case, tol)
    got = run_core(engine("r84", dtype), kind, case)
    err = err_vs(got, case["exact"])
    print(f"ATTN_CORE {dtype} {kind} B={B} L={Ln} C={C} err={err:.3e} bar={tol:.3e} mutants={ {m: f'{v:.2e}' for m, v in case['mut'].items()} }")
    assert err <= tol, (dtype, kind, B, Ln, err, tol)


# ------------------------------------------------------------------------------------------------ 2. blocks of the loaded UNet
_FULL = {}
U256 = UnetConfig(dim=256, upsampling_ratios=(5, 2), unet_scale_cond=True)
MC = CodecConfig(enc_ratios=(8, 4), quantization=False)
CC = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0)


QKV_GAIN = 3.0


def sharpen(sd, u):
    """The synthetic checkpoints give k a spread of a few tenths, so no single position can hold a visible share of a column's softmax
    whatever x is.  The block tests run on the same checkpoint with the k and v rows of every to_qkv (all rows at the bottleneck)
    multiplied by QKV_GAIN: max|k| stays below 20 (asserted per case) and the sentinels get their share."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    for name, (p, C, Ln, linear) in blocks(u).items():
        for pre in ("diff_model.", "diffusion.model."):
            key = pre + p[len("diff_model."):] + ".fn.fn.to_qkv.weight"
            if key in sd:
                sd[key][HD if linear else 0:] *= QKV_GAIN
    return sd


def sd_c2(raw=False):
    if "sd" not in _FULL:
        _FULL["raw"] = synth.ladiff_state_dict(MC, U256, seed=1)
        _FULL["sd"] = sharpen(_FULL["raw"], U256)
    return _FULL["raw" if raw else "sd"]


def build_engine(sd, dtype, u=U256):
    e = Engine(MC, u, CC, dtype=dtype)
    e.load_state_dict(L.MODEL_MAIN, {k: v for k, v in sd.items() if not k.startswith("diffusion.model.")})
    e.load_state_dict(L.MODEL_COND, synth.codec_state_dict(CC, seed=11))
    e.finalize(strict=True)
    return e


def full_engine(dtype):
    """the dim-256 configuration of test_gpu_bench_shape.full_engine("c2", dtype) on the sharpened checkpoint (sharpen)"""
    if dtype not in _FULL:
        _FULL[dtype] = build_engine(sd_c2(), dtype)
    return _FULL[dtype]


def blocks(u, L0=1200):
    """name -> (key prefix, C, L, linear) of every attention block at latent length L0"""
    g = spec.unet_graph(u, "diff_model")
    out, Ln = {}, L0
    for i, lv in enumerate(g.downs):
        out[f"down{i}"] = (lv.attn_prefix, lv.attn_dim, Ln, True)
        if lv.resample_kind == "down":
            Ln //= 2
    out["mid"] = ("diff_model.mid_attn", u.dims[-1], Ln, False)
    for i, lv in enumerate(g.ups):
        out[f"up{i}"] = (lv.attn_prefix, lv.attn_dim, Ln, True)
        if lv.resample_kind == "up":
            Ln *= 2
    return out


BLOCKS = blocks(U256)


def block_ref(sd, p, x, linear, r=ident, mutant=None):
    """oracle.linear_attention / full_attention with the rounding points of the bf16 engine (r) and the mutants"""
    g = sd[p + ".fn.norm.g"]
    xn = r(ln_c(x, g))
    qkv = r(torch.einsum("ck,bkn->bcn", r(sd[p + ".fn.fn.to_qkv.weight"][:, :, 0]), xn))
    if linear:
        return tail(lin_core(qkv, r, mutant), sd[p + ".fn.fn.to_out.0.weight"][:, :, 0], sd[p + ".fn.fn.to_out.0.bias"],
                    sd[p + ".fn.fn.to_out.1.g"][0, :, 0], x, r=r)
    y = torch.einsum("ck,bkn->bcn", r(sd[p + ".fn.fn.to_out.weight"][:, :, 0]), full_core(qkv, r, mutant))
    return r(y + sd[p + ".fn.fn.to_out.bias"][None, :, None] + x)


def block_input(sd, p, B, C, Ln, seed):
    """Gaussian x on the bf16 grid; at the sentinel positions x leans towards one k row per head of to_qkv (through the PreNorm), by as
    much as raises those k by about 9, so that the position holds a large share of those columns' softmax"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, Ln, generator=g, dtype=F64)
    wk = sd[p + ".fn.fn.to_qkv.weight"][HD:2 * HD, :, 0] * sd[p + ".fn.norm.g"][0, :, 0][None, :]   # k = wk @ LayerNorm(x)
    for i, n in enumerate(sentinel_positions(Ln)):
        rows = [h * D + (5 * i + h) % D for h in range(H)]
        d = wk[rows].sum(0)
        d = (d - d.mean()) / d.std()
        a = min(0.9, 9.0 * len(rows) / float((wk[rows] @ d).sum()))
        x[:, :, n] = a * d[None, :] + math.sqrt(1 - a * a) * x[:, :, n]
    return rbf(x)


_BLOCK_CASES = {}


def block_case(tag, sd64, name, B, seed=0):
    key = (tag, name, B)
    if key not in _BLOCK_CASES:
        p, C, Ln, linear = (BLOCKS if tag != "d32" else BLOCKS32)[name]
        x = block_input(sd64, p, B, C, Ln, 31 * Ln + B + seed)
        exact = (O.linear_attention if linear else O.full_attention)(sd64, p, x, H, D)
        kk = torch.einsum("ck,bkn->bcn", sd64[p + ".fn.fn.to_qkv.weight"][HD:2 * HD, :, 0], ln_c(x, sd64[p + ".fn.norm.g"]))
        assert float(kk.abs().max()) < 20.0
        mine = block_ref(sd64, p, x, linear)
        assert err_vs(mine, exact) < 1e-12                       # the mutants and the model are variations of the oracle's own arithmetic
        mx = float(exact.abs().max())
        bar = 2.0 * err_vs(block_ref(sd64, p, x, linear, r=rbf), exact) + bf16_ulp(mx) / mx
        mut = {m: err_vs(block_ref(sd64, p, x, linear, mutant=m), exact) for m in MUTANTS}
        if len(_BLOCK_CASES) > 4:
            _BLOCK_CASES.pop(next(iter(_BLOCK_CASES)))
        _BLOCK_CASES[key] = dict(x=x, exact=exact, bar=bar, mut=mut)
    return _BLOCK_CASES[key]


def sd64_of(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(F64) for k, v in sd.items() if k.startswith("diff_model.")}


def sd64_c2():
    if "sd64" not in _FULL:
        _FULL["sd64"] = sd64_of(sd_c2())
    return _FULL["sd64"]


def check_block(e, dtype, case, name, label):
    tol = case["bar"] if dtype == "bf16" else F32_TOL
    check_power(case, tol)
    got = e.debug_attention_block(name, case["x"].float().cuda()).cpu()
    err = err_vs(got, case["exact"])
    print(f"ATTN_BLOCK {dtype} {label} {name} B={case['x'].shape[0]} C={case['x'].shape[1]} L={case['x'].shape[2]} err={err:.3e} bar={tol:.3e} "
          f"mutants={ {m: f'{v:.2e}' for m, v in case['mut'].items()} }")
    assert err <= tol, (dtype, label, name, err, tol)


@pytest.mark.parametrize("B", [3, 13])
@pytest.mark.parametrize("name", list(BLOCKS))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_attention_block_against_fp64_oracle(dtype, name, B):
    check_block(full_engine(dtype), dtype, block_case("c2", sd64_c2(), name, B), name, "default")


OFF_SWITCHES = [("bf16", "fold_ctx"), ("bf16", "fuse_attn_tail"), ("bf16", "fuse_kmax"), ("bf16", "fold_ln"), ("f32", "fuse_kmax"), ("f32", "fold_ln")]


@pytest.mark.parametrize("name", ["down0", "down1", "down2", "down3", "down4", "up0", "mid"])
@pytest.mark.parametrize("dtype,option", OFF_SWITCHES)
def test_attention_block_option_off_switches_against_fp64_oracle(dtype, option, name):
    """each fallback arrangement against the oracle itself (B = 13: rows are no multiple of any tile, tiles straddle items at L = 75, 150)"""
    e = full_engine(dtype)
    case = block_case("c2", sd64_c2(), name, 13)
    try:
        e.set_option(option, 0)
        check_block(e, dtype, case, name, option + "=0")
    finally:
        e.set_option(option, 1)


U32 = UnetConfig(dim=32, upsampling_ratios=(5, 2), unet_scale_cond=True)
BLOCKS32 = blocks(U32, 160)


@pytest.mark.parametrize("name", ["down4", "down2", "mid"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_attention_block_dim32_routes_away_from_the_fold(dtype, name):
    """dim 32: C in {64, 128} has no fused tail: launch_linattn + to_out conv + ln_rows"""
    from helpers import CASES, main_sd_np
    mc, u, _ = CASES["r84"]
    assert u.dim == 32
    if "sd32" not in _FULL:
        _FULL["sd32"] = sharpen(main_sd_np("r84"), U32)
        _FULL["sd64_32"] = sd64_of(_FULL["sd32"])
    if ("d32", dtype) not in _FULL:
        from helpers import COND_CFG, cond_sd_np
        e = Engine(mc, u, COND_CFG, dtype=dtype)
        e.load_state_dict(L.MODEL_MAIN, _FULL["sd32"])
        e.load_state_dict(L.MODEL_COND, cond_sd_np())
        e.finalize(strict=True)
        _FULL[("d32", dtype)] = e
    check_block(_FULL[("d32", dtype)], dtype, block_case("d32", _FULL["sd64_32"], name, 3), name, "dim32")


# ------------------------------------------------------------------------------------------------ 3. the k-range contract
K_RANGES = {"down0": ("below", -140.0, -100.0), "down1": ("wide", 0.0, 100.0), "down2": ("high", 40.0, 100.0)}
_KR = {}


def k_range_setup():
    """The synthetic dim-256 checkpoint with the k rows of three levels' to_qkv rescaled and shifted along norm.g, and per level an x
    with a constant component e, so that k = s * k_old + m * (e . LayerNorm(x)) / C lands in the level's range (asserted here)."""
    if _KR:
        return _KR
    sd = {k: np.array(v, copy=True) for k, v in sd_c2(raw=True).items()}
    xs = {}
    targets = {"below": (-120.0, 3.0), "wide": (46.0, 8.0), "high": (70.0, 4.0)}
    for name, (kind, lo, hi) in K_RANGES.items():
        p, C, Ln, _ = BLOCKS[name]
        centre, spread = targets[kind]
        g = torch.Generator().manual_seed(len(name) + Ln)
        e = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).to(F64)
        x = rbf(torch.randn(3, C, Ln, generator=g, dtype=F64) + 4.0 * e[None, :, None])
        w = torch.from_numpy(sd[p + ".fn.fn.to_qkv.weight"]).to(F64)
        gn = torch.from_numpy(sd[p + ".fn.norm.g"]).to(F64)
        u = ln_c(x, torch.ones_like(gn))
        k_old = torch.einsum("ck,bkn->bcn", w[HD:2 * HD, :, 0] * gn[0, :, 0][None, :], u)
        proj = torch.einsum("k,bkn->bn", e, u) / C                                    # ~ 0.97, constant sign
        s = spread / float(k_old.std())
        m = centre / float(proj.mean())
        w[HD:2 * HD, :, 0] = s * w[HD:2 * HD, :, 0] + m * (e / gn[0, :, 0] / C)[None, :]
        sd[p + ".fn.fn.to_qkv.weight"] = w.float().numpy()
        for pre in ("diffusion.model.",):
            alt = pre + p[len("diff_model."):] + ".fn.fn.to_qkv.weight"
            if alt in sd:
                sd[alt] = sd[p + ".fn.fn.to_qkv.weight"]
        xs[name] = x
    sd64 = sd64_of(sd)
    for name, (kind, lo, hi) in K_RANGES.items():
        p, C, Ln, _ = BLOCKS[name]
        k = torch.einsum("ck,bkn->bcn", sd64[p + ".fn.fn.to_qkv.weight"][HD:2 * HD, :, 0], ln_c(xs[name], sd64[p + ".fn.norm.g"]))
        assert lo <= float(k.min()) and float(k.max()) <= hi, (name, float(k.min()), float(k.max()))
        if kind == "wide":
            assert int((k > 60).sum()) >= 8 and float(k.min()) < 40
        if kind == "high":
            assert abs(float(k.mean()) - 70.0) < 2.0 and int((k > 60).sum()) > k.numel() // 2
    _KR.update(sd=sd, sd64=sd64, xs=xs)
    return _KR


def k_range_case(name):
    kr = k_range_setup()
    p, C, Ln, linear = BLOCKS[name]
    x = kr["xs"][name]
    exact = O.linear_attention(kr["sd64"], p, x, H, D)
    assert bool(torch.isfinite(exact).all())
    mx = float(exact.abs().max())
    bar = 2.0 * err_vs(block_ref(kr["sd64"], p, x, True, r=rbf), exact) + bf16_ulp(mx) / mx
    return x, exact, bar


def k_range_engine(dtype):
    if dtype not in _KR:
        _KR[dtype] = build_engine(k_range_setup()["sd"], dtype)
    return _KR[dtype]


@pytest.mark.parametrize("name", list(K_RANGES))
@pytest.mark.parametrize("dtype,option", [("bf16", None), ("bf16", "fold_ctx"), ("bf16", "fuse_attn_tail"), ("bf16", "fuse_kmax"), ("f32", None)])
def test_k_range_contract_blocks(dtype, option, name):
    """within the bar, or LDC_E_HIP with the tagged message and recovery through the option the CLI's fallback picks -- never a wrong
    result as success"""
    from ladiffcodec_amd import sample as cli
    x, exact, bar = k_range_case(name)
    tol = bar if dtype == "bf16" else F32_TOL
    e = k_range_engine(dtype)
    try:
        if option:
            e.set_option(option, 0)
        try:
            got = e.debug_attention_block(name, x.float().cuda()).cpu()
            outcome = "returned"
        except L.LdcError as err:
            assert option is None and dtype == "bf16", f"a shifted path failed: {err}"
            assert err.code == L.E_HIP and "device-side failure" in str(err) and "[ctx_range]" in str(err)
            calls = []
            real = e.set_option
            e.set_option = lambda n, v: (calls.append((n, v)), real(n, v))[1]
            try:
                assert cli.apply_device_fallback(e, err)
            finally:
                e.set_option = real
            assert calls == [("fold_ctx", 0)]
            got = e.debug_attention_block(name, x.float().cuda()).cpu()
            outcome = "failed loudly, recovered with fold_ctx 0"
        err_ = err_vs(got, exact)
        print(f"K_RANGE {dtype} {option or 'default'} {name} {K_RANGES[name][0]} {outcome} err={err_:.3e} bar={tol:.3e}")
        assert err_ <= tol, (dtype, option, name, outcome, err_, tol)
    finally:
        e.set_option("fold_ctx", 1)
        if option:
            e.set_option(option, 1)


@pytest.mark.parametrize("rng", ["below", "wide", "high"])
@pytest.mark.parametrize("dtype,kind", [("bf16", "linattn"), ("bf16", "linattn_kmax_fused"), ("bf16", "linattn_ctx_tail"), ("f32", "linattn"),
                                        ("f32", "linattn_kmax_fused")])   # (the fused tail is a bf16 kernel)
def test_k_range_contract_cores(dtype, kind, rng):
    """the shifted core kernels fed the same k ranges directly (B = 3, L = 300)"""
    B, Ln, C = 3, 300, 256
    g = torch.Generator().manual_seed(99)
    qkv = torch.randn(B, 3 * HD, Ln, generator=g, dtype=F64)
    centre, spread = {"below": (-120.0, 4.0), "wide": (46.0, 9.0), "high": (70.0, 5.0)}[rng]
    qkv[:, HD:2 * HD] = (centre + spread * qkv[:, HD:2 * HD]).clamp(centre - 4.4 * spread, centre + 4.4 * spread)
    qkv = rbf(qkv)
    tp = tail_params(B, Ln, C, lin_core(qkv), 5) if kind == "linattn_ctx_tail" else None
    fn = (lambda r=ident: tail(lin_core(qkv, r), *tp, r=r)) if tp else (lambda r=ident: lin_core(qkv, r))
    exact = fn()
    mx = float(exact.abs().max())
    tol = 2.0 * err_vs(fn(rbf), exact) + bf16_ulp(mx) / mx if dtype == "bf16" else F32_TOL
    got = run_core(engine("r84", dtype), kind, dict(qkv=qkv, tp=tp))
    err = err_vs(got, exact)
    print(f"K_RANGE_CORE {dtype} {kind} {rng} err={err:.3e} bar={tol:.3e}")
    assert err <= tol, (dtype, kind, rng, err, tol)
