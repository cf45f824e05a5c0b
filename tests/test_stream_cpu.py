"""CPU-side checks of the stream sessions (chunked SEANet encode / decode that carries state): the ABI, the first-chunk minimum against
the oracle, the compress flag, and the power of the GPU test's schedule."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ladiffcodec_amd import lib as L, synth
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np, rel_err
from oracle import ldc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ldc_stream_min_first", "ldc_stream_create", "ldc_stream_reset", "ldc_stream_destroy", "ldc_seanet_encode_stream",
           "ldc_seanet_decode_stream", "ldc_get_cond_stream"]
SCHEDULE = (7, 1, 1, 5, 10)      # frames; tests/test_gpu_stream.py pushes the same schedule through ldc_get_cond_stream
BAR = 1e-5                       # streamed against whole on the GPU: same fp32 arithmetic, another kernel or summation order


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.LIB_PATH


def ldc_config(codec):
    cfg = L.LdcConfig()
    cfg.rep_dims, cfg.n_filters = codec.rep_dims, codec.n_filters
    cfg.n_residual_layers, cfg.lstm = codec.n_residual_layers, codec.lstm
    cfg.n_enc_ratios = len(codec.enc_ratios)
    for i, r in enumerate(codec.enc_ratios):
        cfg.enc_ratios[i] = r
    cfg.has_cond_model = 1
    return cfg


def test_stream_symbols_are_exported_and_declared(built):
    dll = ctypes.CDLL(built)
    text = open(os.path.join(ROOT, "include", "ladiffcodec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert hasattr(dll, s), f"{s} is not exported"
        assert re.search(r"\b" + s + r"\s*\(", text), f"{s} is not declared in include/ladiffcodec.h"
        assert s in L.EXPORTS
    assert "typedef struct ldc_stream ldc_stream;" in text
    assert re.search(r"#define\s+LDC_STREAM_ENCODER\s+0", text) and re.search(r"#define\s+LDC_STREAM_DECODER\s+1", text)


CODECS = {"cond": (COND_CFG, L.MODEL_COND, cond_sd_np), "r84": (CASES["r84"][0], L.MODEL_MAIN, lambda: main_sd_np("r84")),
          "r8": (CASES["r8"][0], L.MODEL_MAIN, lambda: main_sd_np("r8"))}


@pytest.mark.parametrize("side", [L.STREAM_ENCODER, L.STREAM_DECODER])
@pytest.mark.parametrize("tag", sorted(CODECS))
def test_min_first_is_where_a_prefix_stops_depending_on_what_follows(built, tag, side):
    codec, which, sd_fn = CODECS[tag]
    sd = synth.to_torch(sd_fn())
    hop = codec.hop_length
    unit = hop if side == L.STREAM_ENCODER else 1
    mf = L.stream_min_first(ldc_config(codec), which, side)
    assert mf > 0 and mf % unit == 0
    if tag == "cond" and side == L.STREAM_ENCODER:
        assert mf == 7 * 320 == 2240          # the boundary ldc_get_cond_ragged documents
    g = torch.Generator().manual_seed(17)
    n_max = mf + 2 * unit
    if side == L.STREAM_ENCODER:
        x = torch.from_numpy(synth.synthetic_wav(1, 2 * n_max, seed=5)) * 0.5
        run = lambda t: O.seanet_encode(sd, codec, t)
    else:
        x = torch.randn(1, codec.rep_dims, 2 * n_max, generator=g)
        run = lambda t: O.seanet_decode(sd, codec, t)
    for n in range(unit, n_max + 1, unit):
        short = run(x[..., :n]).numpy()
        long_ = run(x[..., :2 * n]).numpy()[..., :short.shape[-1]]
        err = rel_err(short, long_)
        if n >= mf:
            assert err <= BAR, (tag, side, n, err)
        elif n == mf - unit:
            assert err > BAR, (tag, side, n, err)


def test_compress_parser_takes_stream_sec():
    from ladiffcodec_amd import compress
    p = compress.build_cli_parser()
    assert p.parse_args([]).stream_sec == 0
    assert p.parse_args(["--stream_sec", "1.5"]).stream_sec == 1.5
    with pytest.raises(SystemExit):
        p.parse_args(["--stream_sec", "-1"])
    a = p.parse_args([])
    a.stream_sec = -0.5
    with pytest.raises(SystemExit):
        compress.stream_options(a)


def test_independent_chunks_miss_the_whole_sequence_by_far():
    """What today's whole-sequence calls give when a caller chunks by hand -- reflect padding and a zero LSTM state per chunk -- is
    nowhere near the whole-sequence encode: the GPU test's bar tells a state-carrying implementation from a stateless one."""
    sd = synth.to_torch(cond_sd_np())
    wav = torch.from_numpy(synth.synthetic_wav(3, 7680, seed=300)) * 0.5
    assert sum(SCHEDULE) * 320 == wav.shape[-1]
    whole = O.seanet_encode(sd, COND_CFG, wav).numpy()
    parts, at = [], 0
    for f in SCHEDULE:
        parts.append(O.seanet_encode(sd, COND_CFG, wav[..., at:at + f * 320]).numpy())
        at += f * 320
    err = rel_err(np.concatenate(parts, axis=-1), whole)
    assert err >= 100 * BAR, err
