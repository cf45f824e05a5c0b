"""ResnetBlock.forward (oracle.ldc_oracle.resnet_block) restated in float64 so that it returns its intermediate tensors and the
per-(item, group) GroupNorm sums, takes the engine's rounding points, a ragged batch and per-item timesteps, and can be varied into
the mutants of tests/test_gpu_resnet_layers.py.  CPU only: nothing here touches a GPU.

Rounding model (the r argument; rbf for the bf16 engine, the identity for the exact reference and the f32 engine):
  * the inputs (already on the grid when the tests make them) and the packed weights -- the weight-standardised block1 / block2
    weights, folded in the engine's own float32 arithmetic (packed_fold), and res_conv's weight -- are rounded; biases, GroupNorm
    gains and the (scale | shift) row stay fp32;
  * a conv with the fused GroupNorm epilogue (and the atomic statistics of the unfused pipelined conv) accumulates its sums from the
    un-rounded accumulator, and the fused epilogue normalises the un-rounded accumulator;
  * the unfused gn_apply, and launch_gn_stats (fuse_gn_stats 0, ragged plans), read the conv output as stored: rounded;
  * block1's output b, res_conv's output rr and the block's output (after the residual add and the final block's tanh) are rounded
    once each.
`arr` says which of these holds per conv: ((stats_rounded, apply_rounded) of conv 1, the same of conv 2).
"""
import torch
import torch.nn.functional as F

from ladiffcodec_amd import spec
from oracle import ldc_oracle as O

F64 = torch.float64
FUSED = (False, False)          # fused epilogue: statistics and normalisation on the accumulator
ATOMIC = (False, True)          # conv + atomic statistics + gn_apply
GN_STATS = (True, True)         # conv + launch_gn_stats + gn_apply


def ident(t):
    return t


def block_table(u, prefix="diff_model"):
    """name -> dict(rs, cin1, cin2, attn (prefix, linear) or None, final) of every ResnetBlock, in execution order"""
    g = spec.unet_graph(u, prefix)
    out = {}
    for i, lv in enumerate(g.downs):
        out[f"down{i}.1"] = dict(rs=lv.block1, cin1=lv.block1.cin, cin2=0, attn=None)
        out[f"down{i}.2"] = dict(rs=lv.block2, cin1=lv.block2.cin, cin2=0, attn=(lv.attn_prefix, True))
    out["mid.1"] = dict(rs=g.mid1, cin1=g.mid1.cin, cin2=0, attn=(prefix + ".mid_attn", False))
    out["mid.2"] = dict(rs=g.mid2, cin1=g.mid2.cin, cin2=0, attn=None)
    for i, lv in enumerate(g.ups):
        c = lv.block1.cout
        out[f"up{i}.1"] = dict(rs=lv.block1, cin1=c, cin2=lv.block1.cin - c, attn=None)
        out[f"up{i}.2"] = dict(rs=lv.block2, cin1=c, cin2=lv.block2.cin - c, attn=(lv.attn_prefix, True))
    out["final"] = dict(rs=g.final, cin1=u.dim, cin2=g.final.cin - u.dim, attn=None)
    for k, v in out.items():
        v["final"] = k == "final"
    return out


def packed_fold(w):
    """the weight-standardised conv weight as the engine packs it (build_resnet's fold): mean and variance in double, then float32
    arithmetic (w - float(mean)) * (1 / sqrt(float(var) + 1e-5)); returned in float64.  Rounded to bf16 afterwards, this is the
    bf16 engine's operand bit for bit -- the oracle's fold in float64 lands on the other side of a bf16 rounding boundary for about one
    weight in 10^4, which a GroupNorm sum over a 32-element (one-row) item sees above the 1e-4 bar"""
    w32 = w.to(torch.float32)
    flat = w32.flatten(1).to(F64)
    mean = flat.mean(1)
    var = ((flat - mean[:, None]) ** 2).mean(1)
    rs = torch.ones((), dtype=torch.float32) / torch.sqrt(var.to(torch.float32) + torch.tensor(1e-5, dtype=torch.float32))
    return ((w32 - mean.to(torch.float32)[:, None, None]) * rs[:, None, None]).to(F64)


def block_weights(sd, rs, r=ident, fold=O.ws_fold):
    p = rs.prefix
    W = dict(w1=r(fold(sd[p + ".block1.proj.weight"])), b1=sd[p + ".block1.proj.bias"], g1=sd[p + ".block1.norm.weight"],
             be1=sd[p + ".block1.norm.bias"], w2=r(fold(sd[p + ".block2.proj.weight"])), b2=sd[p + ".block2.proj.bias"],
             g2=sd[p + ".block2.norm.weight"], be2=sd[p + ".block2.norm.bias"], wr=None, br=None)
    if rs.has_res_conv:
        W["wr"] = r(sd[p + ".res_conv.weight"])
        W["br"] = sd[p + ".res_conv.bias"]
    return W


def scale_shift(sd, u, rs, t, prefix="diff_model"):
    """(scale, shift) [B, cout, 1] of the timesteps t (a list, one per item) in float64"""
    temb = O.time_embedding(sd, u, torch.as_tensor(t, dtype=F64), prefix)
    return O.block_scale_shift(sd, rs, temb)


def conv3(x, w, b):
    """k = 3, zero padding 1, as one GEMM over the three shifted copies (F.conv1d's arithmetic up to the order of the sums)"""
    B, C, Ln = x.shape
    xp = F.pad(x, (1, 1))
    X = torch.cat([xp[:, :, k:k + Ln] for k in range(3)], dim=1).permute(1, 0, 2).reshape(3 * C, B * Ln)
    Wm = w.permute(0, 2, 1).reshape(w.shape[0], 3 * C)
    return (Wm @ X).reshape(-1, B, Ln).permute(1, 0, 2) + b[None, :, None]


def leak_delta(x, w):
    """what the flat [B * L] row layout adds to conv3 when an item's outside rows are its neighbours' rows rather than zero: [B, Co, L]"""
    B, _, Ln = x.shape
    d = torch.zeros(B, w.shape[0], Ln, dtype=x.dtype)
    if B > 1:
        d[1:, :, 0] += x[:-1, :, -1] @ w[:, :, 0].T
        d[:-1, :, -1] += x[1:, :, 0] @ w[:, :, 2].T
    return d


def row_mask(B, Ln, lens):
    if lens is None:
        return torch.ones(B, Ln, dtype=torch.bool)
    return torch.arange(Ln)[None, :] < torch.as_tensor(lens)[:, None]


def group_sums(h, groups, valid, mutant=None):
    """(sum, sum of squares) [B, groups, 2] of h [B, C, L] over each item's valid rows; the mutants of the statistics:
    drop_last: the item's last row left out; first_from_prev: the item's first row taken from the neighbour's last row (items >= 1);
    all_rows: the sums run over all L rows whatever the item's length"""
    B, C, Ln = h.shape
    valid = valid.clone()
    if mutant == "all_rows":
        valid[:] = True
    if mutant == "drop_last":
        last = valid.sum(1) - 1
        valid[torch.arange(B), last] = False
    if mutant == "first_from_prev" and B > 1:
        h = h.clone()
        prev_last = valid.sum(1) - 1
        for b in range(1, B):
            h[b, :, 0] = h[b - 1, :, int(prev_last[b - 1])]
    hm = h * valid[:, None, :].to(h.dtype)
    hg = hm.reshape(B, groups, (C // groups) * Ln)
    return torch.stack((hg.sum(-1), (hg * hg).sum(-1)), dim=-1)


def group_norm(h, sums, n, groups, gamma, beta):
    """GroupNorm from the one-pass sums, as the kernels evaluate it: var = sumsq / n - mean^2 (clamped at 0), eps 1e-5"""
    B, C, Ln = h.shape
    mean = sums[..., 0] / n[:, None]
    var = (sums[..., 1] / n[:, None] - mean * mean).clamp_min(0)
    rstd = (var + 1e-5).rsqrt()
    cpg = C // groups
    mean, rstd = mean.repeat_interleave(cpg, 1)[:, :, None], rstd.repeat_interleave(cpg, 1)[:, :, None]
    return (h - mean) * rstd * gamma[None, :, None] + beta[None, :, None]


def resnet_ref(W, x, scale, shift, groups, r=ident, arr=(FUSED, FUSED), lens=None, final=False, mutant=None):
    """The block on x [B, cin, L] (the concatenation, where the block reads one) -> dict of h1, s1, mid, h2, s2, act2, res, out.
    scale / shift [B or 1, cout, 1]; lens: the items' valid rows AT THIS LEVEL (x is masked behind them, the sums run over them, mid
    and out are zero behind them).  Mutants (whole-chain ones; those of the statistics are group_sums', applied to the exact h1 / h2):
    no_plus_one: `scale` instead of `scale + 1`; no_res: the residual omitted; no_res_bias: res_conv's bias omitted; no_tanh."""
    B, _, Ln = x.shape
    dt = x.dtype
    valid = row_mask(B, Ln, lens)
    vm = valid[:, None, :].to(dt)
    cpg = W["w1"].shape[0] // groups
    n = valid.sum(1).to(dt) * cpg
    x = x * vm
    h1 = conv3(x, W["w1"], W["b1"])
    s1 = group_sums(r(h1) if arr[0][0] else h1, groups, valid)
    y1 = group_norm(r(h1) if arr[0][1] else h1, s1, n, groups, W["g1"], W["be1"])
    sc = scale if mutant == "no_plus_one" else scale + 1
    mid = r(F.silu(y1 * sc + shift)) * vm
    h2 = conv3(mid, W["w2"], W["b2"])
    s2 = group_sums(r(h2) if arr[1][0] else h2, groups, valid)
    y2 = group_norm(r(h2) if arr[1][1] else h2, s2, n, groups, W["g2"], W["be2"])
    act2 = F.silu(y2)
    if W["wr"] is not None:
        rr = W["wr"][:, :, 0] @ x
        res = r(rr if mutant == "no_res_bias" else rr + W["br"][None, :, None])
    else:
        res = x
    o = act2 if mutant == "no_res" else act2 + res
    if final and mutant != "no_tanh":
        o = torch.tanh(o)
    return dict(h1=h1, s1=s1, y1=y1, mid=mid, h2=h2, s2=s2, act2=act2, res=res, out=r(o) * vm, n=n, valid=valid, vm=vm)


def stats_err(got, ref, n):
    """the project's measure for fused statistics (ldc_conv_compare): the sum of squares relative, the sum absolute against
    sqrt(n * sumsq_ref); the largest over (item, group)"""
    got, ref = got.to(F64), ref.to(F64)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    es = (got[..., 0] - ref[..., 0]).abs() / (n.to(F64)[:, None] * ref[..., 1]).sqrt()
    eq = (got[..., 1] - ref[..., 1]).abs() / ref[..., 1]
    return float(torch.maximum(es, eq).max())
