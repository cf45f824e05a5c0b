"""The SEANet conv kernels one layer at a time against an fp64 reference (conv_gemm.hip: conv_gemm_kernel, conv_splitk_reduce_kernel;
seanet.hip: conv_cin1_rows_kernel, conv_cin1_kernel; conv_device.h: gather_row, tile_window).

Primitive level (ldc_debug_sea_conv): one SConv1d / SConvTranspose1d on caller weights through sea_conv() itself -- the ConvCall, the
split-K workspace (option sea_splitk) and the arena of a real encode / decode -- or, for Cin = 1, through launch_conv_cin1.  The hook
reports the route: cin1_rows | cin1_generic | pipelined | generic, and for the generic kernel its tile configuration <WM,WN,TM,TN>,
split-K factor and taps per LDS group tg; the last test of the file asserts that every configuration launch_conv can pick was hit.
Op level (ldc_debug_sea_op): every op of the encoder and decoder of the cond codec (ratios 8 5 4 2) and of r84's main codec (8 4) through
run_seanet, at the lengths of a 2.4 s clip (38400 samples) and of a 4123-sample one (a remainder against either hop), B in {3, 13}.

Reference: oracle.ldc_oracle.sconv1d / sconvtr1d / _resblock / lstm_skip on float64 tensors (F.elu in float64 where the kernel has a
pre-ELU).  Bars, relative to max|exact| (gpu_common.rel), are the project's fp32 bars: 1e-5 without ELU in the path
(test_sconv1d_against_reference_vectors), 2e-5 with ELU or an LSTM (fast_elu uses __expf; test_slstm_all_kernel_variants).  Every case
asserts on the CPU, before the GPU is touched, that the same arithmetic in float32 stays within a quarter of its bar.

Power, asserted on the CPU per case and never run on the GPU: mutants of the float64 reference must miss the bar by >= 4x --
(a) zero and (b) replicate padding instead of reflect (where the conv pads at all), (c) for B >= 2 the padding rows of an item taken
from its neighbours' rows, as a flat window with a wrong seam would (where the conv pads), (d) the last 16-channel chunk of K dropped,
(e) transposed: the trim shifted by one, (f) the residual (resblock: the shortcut conv) omitted.  The first and last two positions of
every item are multiplied by 4 so that the edge outputs are never the small ones.

Short inputs (L <= max(pad_left, right_pad + extra)): the reference's pad1d zero-extends such an input before it reflects (conv.py:81-98).
gather_row mirrors about ConvKArgs::reflect_len for it, so the generic kernel follows the reference there; the Cin = 1
kernels refuse L <= k - 1.  test_short_input_contract: within the bar, or LDC_E_INVALID naming the length and the pad, never another value.

Measured: NOT YET.  No MI355X run of this file has been recorded: the per-row table of largest GPU error and smallest mutant error,
the file's wall time beside the suite's (about 2 minutes) and the counts of the scratch mutation check (gather_row mirroring about
leff instead of leff - 1; conv_splitk_reduce_kernel summing one slice short) are all still owed.  Every test prints its row
("SEANET row=... case=... bar=... err=... min_mutant=...") under -s, which is what the table is to be filled from.  What is known, from
the CPU alone: the fp32 model of every case stays within a quarter of its bar, the mutants (a)-(f) of every case miss their bar by
>= 4x (the test asserts both before it touches the GPU), and on the short inputs the single mirror about L - 1 that gather_row did
before section 5b measures 0.38 to 1.12 relative to max|exact|, four orders above the bar.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, spec, synth  # noqa: E402
from oracle import ldc_oracle as O  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import engine, rel  # noqa: E402

F64 = torch.float64
BAR_PLAIN, BAR_ELU = 1e-5, 2e-5
ROUTES = {}      # grid case id -> route report of its default run (test_route_coverage)


def eng():
    return engine("r84", "f32")


def geom(Lx, k, s, d, causal):
    """(pad_left, right_pad + extra) of SConv1d.forward (conv.py:217-232)"""
    total = (k - 1) * d - (s - 1)
    extra = O.extra_padding_for_conv1d(Lx, k, s, total)
    if causal:
        return total, extra
    return total - total // 2, total // 2 + extra


def edged(x):
    x = x.clone()
    x[..., :2] *= 4
    x[..., -2:] *= 4
    return x


def padded(x, left, right, mode):
    if mode == "reflect":
        return O.pad1d_reflect(x, left, right)
    if mode == "zero":
        return F.pad(x, (left, right))
    if mode == "replicate":
        return F.pad(x, (left, right), mode="replicate")
    assert mode == "seam"                      # a flat [B*L] window: an item's pads are its neighbours' rows
    B, C, Lx = x.shape
    flat = x.permute(1, 0, 2).reshape(C, B * Lx)
    out = O.pad1d_reflect(x, left, right).clone()
    for b in range(B):
        if b > 0 and left:
            out[b, :, :left] = flat[:, b * Lx - left:b * Lx]
        if b < B - 1 and right:
            out[b, :, left + Lx:] = flat[:, (b + 1) * Lx:(b + 1) * Lx + right]
    return out


def drop_last_chunk(w, cin_axis):
    """the weights with the last 16-channel chunk of the input channels zeroed"""
    w = w.clone()
    cin = w.shape[cin_axis]
    lo = (cin - 1) // 16 * 16
    idx = [slice(None)] * w.dim()
    idx[cin_axis] = slice(lo, cin)
    w[tuple(idx)] = 0
    return w


def conv_mutants(xa, w, b, s, d, causal, res, B):
    """mutants (a) (b) (c) (d) (f) of a plain conv on the (already activated) input xa"""
    left, right = geom(xa.shape[-1], w.shape[-1], s, d, causal)
    add = res if res is not None else 0
    out = {}
    if left + right > 0:
        for name, mode in (("a_zero", "zero"), ("b_replicate", "replicate")) + ((("c_seam", "seam"),) if B >= 2 else ()):
            out[name] = F.conv1d(padded(xa, left, right, mode), w, b, stride=s, dilation=d) + add
    if w.shape[1] > 1:
        out["d_chunk"] = O.sconv1d(xa, drop_last_chunk(w, 1), b, s, d, causal) + add
    if res is not None:
        out["f_residual"] = O.sconv1d(xa, w, b, s, d, causal)
    return out


def convtr_mutants(xa, w, b, s, causal):
    k = w.shape[-1]
    full = F.conv_transpose1d(xa, w, b, stride=s)
    total = k - s
    right = total if causal else total // 2
    left = total - right
    shifted = full[..., left + 1:full.shape[-1] - right + 1] if right >= 1 else full[..., left - 1:full.shape[-1] - 1]
    return {"d_chunk": O.sconvtr1d(xa, drop_last_chunk(w, 0), b, s, causal), "e_trim": shifted}


def check_power(tag, exact, mutants, bar):
    worst = min((rel(m.numpy(), exact.numpy()) for m in mutants.values()), default=float("inf"))
    for name, m in mutants.items():
        r = rel(m.numpy(), exact.numpy())
        assert r >= 4 * bar, (tag, "mutant within 4x of the bar", name, r)
    return worst


def report(row, tag, bar, err, power, extra=""):
    print(f"SEANET row={row} case={tag} bar={bar:.0e} err={err:.3e} min_mutant={power:.3e} {extra}")


# ------------------------------------------------------------------------------------------------ 1. primitive grid
# plain: (B, Cin, Cout, L, k, stride, dilation, causal, pre_elu, residual)
PLAIN = [
    (3, 512, 128, 121, 7, 1, 1, 1, 1, 0),      # several items per 128-row tile, split-K
    (2, 256, 512, 1203, 16, 8, 1, 1, 1, 0),    # L % stride != 0, tg < taps at bn = 64, split-K
    (5, 64, 32, 77, 3, 1, 9, 1, 1, 0),         # bn = 32, dilation 9
    (13, 128, 256, 263, 10, 5, 1, 1, 0, 0),    # L_rows = 53, extra > 0
    (2, 40, 24, 9, 4, 2, 1, 0, 0, 0),          # Cin not a multiple of 16, n != n_pad
    (32, 64, 512, 128, 7, 1, 1, 1, 1, 1),      # <2,2,2,2>, tg < taps at bn = 128, exact tile
    (32, 16, 64, 512, 3, 1, 2, 1, 1, 0),       # <2,2,2,1>
    (3, 64, 128, 127, 3, 1, 3, 0, 0, 0),       # <2,2,1,1> unsplit (4 chunks), non-causal
    (3, 128, 256, 129, 1, 1, 1, 1, 1, 1),      # a resblock's conv2: k = 1, ELU, residual through the split-K reduce
    (1, 256, 96, 150, 7, 1, 1, 0, 1, 0),       # Cout = 96: bn = 32
    (13, 64, 64, 3, 4, 4, 1, 1, 0, 0),         # L_rows = 1, extra = 1
    (32, 128, 64, 7, 3, 1, 1, 1, 1, 1),        # L_rows = 7: 18 items per tile
    (2, 16, 32, 7, 7, 1, 1, 1, 0, 0),          # L = pad_left + 1
    (3, 128, 256, 601, 10, 4, 1, 0, 1, 0),     # stride 4, non-causal, extra = 3
    (13, 256, 512, 240, 4, 2, 1, 1, 1, 0),     # the cond encoder's stride-2 conv
    (2, 16, 32, 200, 3, 1, 9, 0, 0, 0),        # dilation 9, non-causal: 9 rows reflected at either end
    (3, 40, 96, 128, 3, 1, 2, 1, 1, 1),        # Cin 40 -> 48, bn = 32, residual on the unsplit epilogue
    (1, 16, 24, 1203, 7, 1, 1, 0, 1, 0),
    (3, 64, 128, 1200, 16, 8, 1, 1, 1, 0),     # causal, L % stride == 0: no right padding
    (13, 512, 128, 120, 7, 1, 1, 1, 1, 0),     # the cond encoder's last conv
    (32, 64, 64, 105, 4, 2, 1, 0, 0, 0),       # L_rows = 53, two to three items per tile
    (2, 512, 512, 15, 7, 1, 1, 1, 0, 0),       # the cond decoder's first conv at 15 frames
]
# transposed: (B, Cin, Cout, L, stride, causal, pre_elu)
TRANSPOSED = [
    (1, 512, 256, 15, 8, 1, 1),                # the cond decoder's first convtr, split-K
    (3, 512, 256, 120, 8, 1, 1),
    (13, 512, 256, 15, 8, 0, 0),
    (3, 64, 32, 2, 2, 0, 1),
    (13, 128, 64, 1, 5, 1, 0),                 # L = 1, split-K
    (3, 128, 64, 601, 5, 0, 1),
    (1, 256, 128, 120, 4, 0, 0),               # non-causal trim in the split-K reduce
    (1, 256, 128, 120, 4, 0, 1),
    (13, 64, 32, 15, 2, 1, 0),
    (1, 16, 24, 601, 4, 1, 1),                 # bn = 32
    (3, 512, 256, 2, 8, 1, 0),
]
# Cin = 1: (B, Cout, k, L)
CIN1 = [(1, 32, 7, 7), (3, 32, 7, 8), (32, 32, 7, 255), (3, 32, 7, 256), (1, 32, 7, 257), (3, 32, 7, 38400),
        (1, 48, 7, 7), (3, 48, 7, 8), (3, 48, 7, 255), (32, 48, 7, 256), (1, 48, 7, 257), (3, 48, 7, 38400),
        (3, 32, 9, 9), (3, 32, 9, 10), (1, 32, 9, 257), (32, 32, 9, 255), (3, 32, 9, 38400)]


def plain_data(case, seed=0):
    B, Cin, Cout, Lx, k, s, d, causal, elu, res = case
    g = torch.Generator().manual_seed(1000 + seed + 7 * B + Cin + 3 * Cout + Lx + 11 * k)
    x = edged(torch.randn(B, Cin, Lx, generator=g))
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(B, Cout, -(-Lx // s), generator=g) if res else None
    return x, w, b, r


def plain_ref(x, w, b, r, case, dt):
    _, _, _, _, _, s, d, causal, elu, _ = case
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    xa = F.elu(x) if elu else x
    y = O.sconv1d(xa, w, b, s, d, bool(causal))
    return (y + r.to(dt) if r is not None else y), xa, w, b


def run_plain(case, x, w, b, r):
    _, _, _, _, _, s, d, causal, elu, _ = case
    y, rep = eng().debug_sea_conv(x.cuda(), w.numpy(), b.numpy(), stride=s, dilation=d, causal=bool(causal), pre_elu=bool(elu),
                                  residual=r.cuda() if r is not None else None)
    return y.cpu().double(), rep


def with_and_without_splitk(run, exact, bar, tag):
    """the default run; where it split K, once more with sea_splitk 0: both within the bar, and within 1e-5 of each other"""
    y, rep = run()
    err = rel(y.numpy(), exact.numpy())
    if rep.get("ksplit", 1) > 1:
        # the option is 0 or 1 and has no getter; sea_conv splits K only under 1, so the run above has just shown that the engine's
        # value is 1 -- an engine started with it off never comes here and is left as it was
        e, before = eng(), 1
        try:
            e.set_option("sea_splitk", 0)
            y0, rep0 = run()
        finally:
            e.set_option("sea_splitk", before)
        assert rep0["route"] == "generic" and rep0["ksplit"] == 1, (tag, rep0)
        err0 = rel(y0.numpy(), exact.numpy())
        print(f"SEANET   {tag}: split-K {rep['ksplit']} err {err:.3e}, unsplit err {err0:.3e}, apart {rel(y.numpy(), y0.numpy()):.3e}")
        assert err0 <= bar, (tag, "sea_splitk 0", err0, bar)
        assert rel(y.numpy(), y0.numpy()) <= 1e-5, (tag, "split-K and unsplit runs apart", rel(y.numpy(), y0.numpy()))
        err = max(err, err0)
    return err, rep


def row_of(rep):
    if rep["route"] != "generic":
        return rep["route"]
    return "generic<%d,%d,%d,%d>%s" % (*rep["tile"], " split-K" if rep["ksplit"] > 1 else "")


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: "B%d-%dto%d-L%d-k%ds%dd%d-c%de%dr%d" % c)
def test_plain_conv(case):
    B, Cin, Cout, Lx, k, s, d, causal, elu, res = case
    left, right = geom(Lx, k, s, d, causal)
    assert Lx > max(left, right), "a short input belongs to test_short_input_contract"
    bar = BAR_ELU if elu else BAR_PLAIN
    x, w, b, r = plain_data(case)
    exact, xa, w64, b64 = plain_ref(x, w, b, r, case, F64)
    model = plain_ref(x, w, b, r, case, torch.float32)[0]
    assert rel(model.numpy(), exact.numpy()) <= bar / 4, ("fp32 model", rel(model.numpy(), exact.numpy()))
    power = check_power(case, exact, conv_mutants(xa, w64, b64, s, d, bool(causal), r.double() if res else None, B), bar)
    err, rep = with_and_without_splitk(lambda: run_plain(case, x, w, b, r), exact, bar, case)
    ROUTES[("plain", case)] = rep
    report("plain " + row_of(rep), "B%d-%dto%d-L%d-k%ds%dd%d-c%de%dr%d" % case, bar, err, power, str(rep))
    assert rep["route"] == "generic", rep
    assert err <= bar, (case, err, bar, rep)


def tr_data(case):
    B, Cin, Cout, Lx, s, causal, elu = case
    g = torch.Generator().manual_seed(2000 + 7 * B + Cin + 3 * Cout + Lx + 11 * s)
    x = edged(torch.randn(B, Cin, Lx, generator=g))
    w = torch.randn(Cin, Cout, 2 * s, generator=g) / math.sqrt(2 * Cin)
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


def run_tr(case, x, w, b):
    _, _, _, _, s, causal, elu = case
    y, rep = eng().debug_sea_conv(x.cuda(), w.numpy(), b.numpy(), stride=s, causal=bool(causal), transposed=True, pre_elu=bool(elu))
    return y.cpu().double(), rep


@pytest.mark.parametrize("case", TRANSPOSED, ids=lambda c: "B%d-%dto%d-L%d-s%d-c%de%d" % c)
def test_transposed_conv(case):
    B, Cin, Cout, Lx, s, causal, elu = case
    bar = BAR_ELU if elu else BAR_PLAIN
    x, w, b = tr_data(case)
    act = F.elu if elu else (lambda t: t)
    exact = O.sconvtr1d(act(x.double()), w.double(), b.double(), s, bool(causal))
    model = O.sconvtr1d(act(x), w, b, s, bool(causal))
    assert rel(model.numpy(), exact.numpy()) <= bar / 4, ("fp32 model", rel(model.numpy(), exact.numpy()))
    power = check_power(case, exact, convtr_mutants(act(x.double()), w.double(), b.double(), s, bool(causal)), bar)
    err, rep = with_and_without_splitk(lambda: run_tr(case, x, w, b), exact, bar, case)
    ROUTES[("tr", case)] = rep
    report("transposed " + row_of(rep), "B%d-%dto%d-L%d-s%d-c%de%d" % case, bar, err, power, str(rep))
    assert rep["route"] == "generic", rep
    assert err <= bar, (case, err, bar, rep)


def cin1_data(case):
    B, Cout, k, Lx = case
    g = torch.Generator().manual_seed(3000 + 7 * B + Cout + 11 * k + Lx)
    x = edged(torch.randn(B, 1, Lx, generator=g))
    w = torch.randn(Cout, 1, k, generator=g) / math.sqrt(k)
    b = torch.randn(Cout, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize("case", CIN1, ids=lambda c: "B%d-1to%d-k%d-L%d" % c)
def test_cin1_conv(case):
    B, Cout, k, Lx = case
    x, w, b = cin1_data(case)
    exact = O.sconv1d(x.double(), w.double(), b.double())
    model = O.sconv1d(x, w, b)
    assert rel(model.numpy(), exact.numpy()) <= BAR_PLAIN / 4
    power = check_power(case, exact, conv_mutants(x.double(), w.double(), b.double(), 1, 1, True, None, B), BAR_PLAIN)
    y, rep = eng().debug_sea_conv(x.cuda(), w.numpy(), b.numpy())
    err = rel(y.cpu().numpy(), exact.numpy())
    report(rep["route"], "B%d-1to%d-k%d-L%d" % case, BAR_PLAIN, err, power)
    assert rep["route"] == ("cin1_rows" if (Cout, k) == (32, 7) else "cin1_generic"), rep
    assert err <= BAR_PLAIN, (case, err)


def test_cin1_route_is_causal_only():
    x, w, b = cin1_data((1, 32, 7, 64))
    with pytest.raises(L.LdcError) as ei:
        eng().debug_sea_conv(x.cuda(), w.numpy(), b.numpy(), causal=False)
    assert ei.value.code == L.E_INVALID


# ------------------------------------------------------------------------------------------------ 2. op level
CODECS = {"cond": (L.MODEL_COND, COND_CFG), "main": (L.MODEL_MAIN, CASES["r84"][0])}
T_CLIP, T_REM = 38400, 4123
_SD = {}


def codec_sd(name):
    if name not in _SD:
        sd = cond_sd_np() if name == "cond" else main_sd_np("r84")
        _SD[name] = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items() if k.startswith(("encoder.", "decoder."))}
    return _SD[name]


def ops_of(cfg, decoder, T):
    """[(layer, pre_elu, L_in)] of the stack's ops in engine order (an ELU in front of a conv is that conv's prologue)"""
    layers = spec.seanet_decoder_layers(cfg) if decoder else spec.seanet_encoder_layers(cfg)
    Lx = -(-T // cfg.hop_length) if decoder else T
    out, elu = [], False
    for ly in layers:
        if ly.kind == "elu":
            elu = True
            continue
        out.append((ly, elu, Lx))
        elu = False
        if ly.kind == "conv":
            Lx = -(-Lx // ly.stride)
        elif ly.kind == "convtr":
            Lx *= ly.stride
    return out


OP_CASES = [(name, dec, i, T, B) for name, (_, cfg) in CODECS.items() for dec in (0, 1) for i in range(len(ops_of(cfg, dec, T_CLIP)))
            for T in (T_CLIP, T_REM) for B in (3, 13)]


def res_variant(x, sd, p, ly, mode="reflect", drop=False, no_shortcut=False):
    w1, b1 = O._wn(sd, p + ".block.1.conv.conv")
    w2, b2 = O._wn(sd, p + ".block.3.conv.conv")
    ws, bs = O._wn(sd, p + ".shortcut.conv.conv")
    if drop:
        w1 = drop_last_chunk(w1, 1)
    h = F.conv1d(padded(F.elu(x), 2 * ly.dilation, 0, mode), w1, b1, dilation=ly.dilation)
    h = O.sconv1d(F.elu(h), w2, b2)
    return h if no_shortcut else O.sconv1d(x, ws, bs) + h


def op_ref(x, sd, p, ly, elu):
    xa = F.elu(x) if elu else x
    if ly.kind == "conv":
        w, b = O._wn(sd, p + ".conv.conv")
        return O.sconv1d(xa, w, b, stride=ly.stride)
    if ly.kind == "convtr":
        w, b = O._wn(sd, p + ".convtr.convtr")
        return O.sconvtr1d(xa, w, b, ly.stride, causal=True)
    if ly.kind == "res":
        return O._resblock(x, sd, p, ly)
    return O.lstm_skip(x, sd, p, ly.layers)


def op_mutants(x, sd, p, ly, elu, B):
    xa = F.elu(x) if elu else x
    if ly.kind == "conv":
        w, b = O._wn(sd, p + ".conv.conv")
        return conv_mutants(xa, w, b, ly.stride, 1, True, None, B)
    if ly.kind == "convtr":
        w, b = O._wn(sd, p + ".convtr.convtr")
        return convtr_mutants(xa, w, b, ly.stride, True)
    if ly.kind == "res":
        out = {"a_zero": res_variant(x, sd, p, ly, "zero"), "b_replicate": res_variant(x, sd, p, ly, "replicate"),
               "d_chunk": res_variant(x, sd, p, ly, drop=True), "f_shortcut": res_variant(x, sd, p, ly, no_shortcut=True)}
        if B >= 2:
            out["c_seam"] = res_variant(x, sd, p, ly, "seam")
        return out
    return {}


@pytest.mark.parametrize("name,dec,i,T,B", OP_CASES, ids=lambda v: str(v))
def test_codec_op(name, dec, i, T, B):
    which, cfg = CODECS[name]
    ly, elu, Lx = ops_of(cfg, dec, T)[i]
    sd32 = codec_sd(name)
    sd64 = {k: v.double() for k, v in sd32.items() if k.startswith(f"{'decoder' if dec else 'encoder'}.model.{ly.index}.")}
    p = f"{'decoder' if dec else 'encoder'}.model.{ly.index}"
    bar = BAR_ELU if (elu or ly.kind in ("res", "lstm")) else BAR_PLAIN
    g = torch.Generator().manual_seed(4000 + 100 * i + 7 * B + dec + (T == T_REM))
    x = edged(torch.randn(B, ly.cin, Lx, generator=g))
    exact = op_ref(x.double(), sd64, p, ly, elu)
    model = op_ref(x, sd32, p, ly, elu)
    assert rel(model.numpy(), exact.numpy()) <= bar / 4, ("fp32 model", rel(model.numpy(), exact.numpy()))
    power = check_power((name, dec, i, T, B), exact, op_mutants(x.double(), sd64, p, ly, elu, B), bar)
    e = eng()
    kind, cin, cout, Lo = e.debug_sea_op_info(which, bool(dec), i, B, Lx)
    want = "conv_cin1" if (ly.kind == "conv" and ly.cin == 1) else ly.kind
    assert (kind, cin, cout, Lo) == (want, ly.cin, exact.shape[1], exact.shape[2]), (kind, cin, cout, Lo)
    y = e.debug_sea_op(which, bool(dec), i, x.cuda()).cpu()
    err = rel(y.numpy(), exact.numpy())
    report("op " + kind, f"{name}-{'dec' if dec else 'enc'}{i}-{ly.cin}to{cout}-L{Lx}-B{B}", bar, err, power)
    assert err <= bar, (name, dec, i, T, B, err, bar)


# ------------------------------------------------------------------------------------------------ 3. short inputs
# (B, Cin, Cout, L, k, stride, dilation, causal, pre_elu, residual); Cin = 1 rows go to launch_conv_cin1
SHORT = [(3, 64, 32, 2, 7, 1, 1, 0, 0, 0), (3, 64, 32, 3, 7, 1, 1, 0, 1, 0), (3, 64, 32, 4, 7, 1, 1, 0, 0, 0),
         (3, 64, 64, 2, 4, 4, 1, 1, 0, 0), (2, 128, 128, 5, 16, 8, 1, 0, 1, 0), (2, 128, 128, 9, 16, 8, 1, 0, 0, 0),
         (3, 512, 128, 2, 7, 1, 1, 1, 1, 0), (13, 512, 128, 6, 7, 1, 1, 1, 1, 0), (3, 64, 32, 5, 3, 1, 9, 1, 1, 0),
         (3, 1, 32, 6, 7, 1, 1, 1, 0, 0), (1, 1, 32, 1, 7, 1, 1, 1, 0, 0), (3, 1, 48, 5, 7, 1, 1, 1, 0, 0), (3, 1, 32, 8, 9, 1, 1, 1, 0, 0)]


def single_mirror_padded(x, left, right):
    """the padding gather_row did before reflect_len: one mirror at 0, one about L - 1, and zero for whatever is still outside"""
    Lx = x.shape[-1]
    u = torch.arange(-left, Lx + right).abs()
    u = torch.where(u >= Lx, 2 * (Lx - 1) - u, u)
    inside = (u >= 0) & (u < Lx)
    return x[..., u.clamp(0, Lx - 1)] * inside.to(x.dtype)


@pytest.mark.parametrize("case", SHORT, ids=lambda c: "B%d-%dto%d-L%d-k%ds%dd%d-c%de%dr%d" % c)
def test_short_input_contract(case):
    """Within the bar of oracle.sconv1d (the reference's zero-extend-then-reflect) or LDC_E_INVALID naming length and pad.
    On the CPU first: the fp32 model of the case within a quarter of the bar, and the single mirror about L - 1 that gather_row did
    before it followed the reference misses the bar by >= 4x, so a pass here tells the two apart
    (at the boundary of the short set, non-causal k = 7 at L = 4, and at L = 1 both paddings agree and there is no such mutant)."""
    B, Cin, Cout, Lx, k, s, d, causal, elu, res = case
    left, right = geom(Lx, k, s, d, causal)
    is_short = Lx <= max(left, right)
    bar = BAR_ELU if elu else BAR_PLAIN
    x, w, b, r = plain_data(case, seed=5)
    exact, xa, w64, b64 = plain_ref(x, w, b, r, case, F64)
    model = plain_ref(x, w, b, r, case, torch.float32)[0]
    assert rel(model.numpy(), exact.numpy()) <= bar / 4, ("fp32 model", rel(model.numpy(), exact.numpy()))
    xp = single_mirror_padded(xa, left, right)
    if is_short and Lx > 1:
        power = check_power(case, exact, {"single_mirror": F.conv1d(xp, w64, b64, stride=s, dilation=d)}, bar)
    else:       # no mutant: one past the short set (non-causal k = 7 at L = 4), or L = 1 with nothing to mirror, the paddings are the same
        power = float("inf")
        assert torch.equal(xp, O.pad1d_reflect(xa, left, right)), case
    try:
        y, rep = run_plain(case, x, w, b, r)
    except L.LdcError as ex:
        assert ex.code == L.E_INVALID, ex
        assert f"L={Lx}" in str(ex) and f"pad={max(left, right)}" in str(ex), str(ex)
        assert is_short, (case, "a refusal outside the short set")
        print(f"SEANET row=short case={case} min_mutant={power:.3e} refused: {ex}")
        if Cin == 1 and Lx <= 6:       # the encoder's own first conv (op 0 of the cond encoder: k = 7) refuses in the same words
            with pytest.raises(L.LdcError) as ei:
                eng().debug_sea_op(L.MODEL_COND, False, 0, x.cuda())
            assert ei.value.code == L.E_INVALID and f"L={Lx}" in str(ei.value) and "pad=6" in str(ei.value), str(ei.value)
        ok = (2, 16, 32, 7, 7, 1, 1, 1, 0, 0)       # the engine is still usable
        x2, w2, b2, _ = plain_data(ok)
        y2, _ = run_plain(ok, x2, w2, b2, None)
        assert rel(y2.numpy(), plain_ref(x2, w2, b2, None, ok, F64)[0].numpy()) <= BAR_PLAIN
        return
    err = rel(y.numpy(), exact.numpy())
    report("short " + row_of(rep), "B%d-%dto%d-L%d-k%ds%dd%d-c%de%dr%d" % case, bar, err, power)
    assert err <= bar, (case, "a value that differs from the reference returned as success", err)


# ------------------------------------------------------------------------------------------------ 4. route coverage
def test_route_coverage():
    """Every generic tile configuration launch_conv can pick (conv_gemm.hip) was hit by the grid above; a grid case that has not run in
    this session (a -k selection) runs here on the GPU alone."""
    for case in PLAIN:
        if ("plain", case) not in ROUTES:
            ROUTES[("plain", case)] = run_plain(case, *plain_data(case))[1]
    for case in TRANSPOSED:
        if ("tr", case) not in ROUTES:
            ROUTES[("tr", case)] = run_tr(case, *tr_data(case))[1]
    reps = list(ROUTES.values())
    assert all(r["route"] == "generic" for r in reps)
    tiles = {(r["tile"], r["ksplit"] > 1) for r in reps}
    for cfg in ((2, 2, 2, 2), (2, 2, 2, 1), (4, 1, 1, 1), (2, 2, 1, 1)):
        assert (cfg, False) in tiles, ("no unsplit case on tile configuration", cfg)
    splits = {r["ksplit"] for r in reps if r["tile"] == (2, 2, 1, 1) and r["ksplit"] > 1}
    print("SEANET split-K factors hit:", sorted(splits))
    assert len(splits) >= 2, splits
    taps = {("plain", c): c[4] for c in PLAIN}
    taps.update({("tr", c): 2 for c in TRANSPOSED})
    assert any(r["tg"] < taps[key] for key, r in ROUTES.items()), "no case with tg < taps"
    assert any(r["tg"] == taps[key] for key, r in ROUTES.items()), "no case with tg == taps"
    assert {r["bn"] for r in reps} == {32, 64, 128}
