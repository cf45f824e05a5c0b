"""Decode from RVQ codes without a GPU: the C entries' argument refusals, the ECDC container layer and the two CLIs' flags."""
import ctypes as C
import io
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from ladiffcodec_amd import bitstream as BS, lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_exported():
    for name in ("ldc_decode_codes", "ldc_decode_codes_ddim"):
        assert name in L.EXPORTS
        assert hasattr(C.CDLL(L.LIB_PATH), name), name


def _err():
    return L.load().ldc_last_error().decode()


def test_decode_codes_refusals_without_context():
    lib = L.load()
    codes, packed, out = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64)     # never dereferenced: refused before any use
    nb = int(lib.ldc_packed_bytes(6, 20, 10))

    def ddpm(codes_p, packed_p, stride=nb, bits=10, n_q=6, steps=4):
        return lib.ldc_decode_codes(None, codes_p, packed_p, stride, bits, n_q, 2, 20, steps, None, 1, out, None, None, None)

    def ddim(codes_p, packed_p, stride=nb, bits=10, n_q=6, t_start=30, steps=6, eta=0.0):
        return lib.ldc_decode_codes_ddim(None, codes_p, packed_p, stride, bits, n_q, 2, 20, t_start, steps, eta, None, 1, out, None,
                                         None, None)

    for fn in (ddpm, ddim):
        assert fn(codes, packed) == L.E_INVALID and "exactly one" in _err()
        assert fn(None, None) == L.E_INVALID and "exactly one" in _err()
        assert fn(codes, None, n_q=0) == L.E_INVALID and "n_q" in _err()
        assert fn(None, packed, bits=0) == L.E_INVALID and "bits" in _err()
        assert fn(None, packed, bits=17) == L.E_INVALID and "bits" in _err()
        assert fn(None, packed, stride=nb - 1) == L.E_INVALID and "packed_stride" in _err()
        assert fn(codes, None) == L.E_INVALID and "null ctx" in _err()       # valid arguments: only the context is missing
    assert ddpm(codes, None, steps=0) == L.E_INVALID and "n_steps" in _err()
    for kw in (dict(eta=-0.1), dict(eta=1.5), dict(eta=float("nan")), dict(t_start=0), dict(steps=0), dict(t_start=10, steps=11)):
        assert ddim(codes, None, **kw) == L.E_INVALID, kw
        assert "null ctx" not in _err(), kw


def _blob(meta, payload, magic=b"ECDC", version=0):
    fo = io.BytesIO()
    m = json.dumps(meta).encode()
    fo.write(struct.pack("!4sBI", magic, version, len(m)))
    fo.write(m)
    fo.write(payload)
    return fo.getvalue()


def test_container_round_trip_multichannel():
    rng = np.random.default_rng(0)
    n_q, al = 6, 6400
    F = al // 320
    nb = BS.packed_bytes(n_q, F, 10)
    assert nb == int(L.load().ldc_packed_bytes(n_q, F, 10))
    pays = [rng.integers(0, 256, nb, dtype=np.uint8).tobytes() for _ in range(3)]
    blob = BS.ecdc_container(pays, al, n_q)
    assert len(blob) == BS._encodec_header_struct.size + len(json.dumps(BS.ecdc_meta(al, n_q, channels=3)).encode()) + 3 * nb
    meta, rows, F2 = BS.parse_ecdc(blob, "x.ecdc", 6)
    assert meta == {"m": BS.MODEL_NAME, "al": al, "nc": n_q, "lm": False, "hop": 320, "ch": 3}
    assert F2 == F and rows.shape == (3, nb)
    assert [r.tobytes() for r in rows] == pays
    mono = BS.ecdc_container(pays[:1], al, n_q)
    meta1, rows1, _ = BS.parse_ecdc(mono, "y.ecdc", 6)
    assert "ch" not in meta1 and rows1.shape == (1, nb)
    # the reference reader (binary.py:43-52 mirror) reads the same header
    assert BS.read_ecdc_header(io.BytesIO(mono)) == meta1


@pytest.mark.parametrize("case", ["model", "lm", "ac", "nc", "short", "magic", "version", "hop", "long"])
def test_container_refusals_name_the_file(case):
    n_q, al = 6, 6400
    nb = BS.packed_bytes(n_q, al // 320, 10)
    meta = BS.ecdc_meta(al, n_q)
    payload = bytes(nb)
    magic, version = b"ECDC", 0
    if case == "model":
        meta["m"] = "encodec_24khz"
    elif case == "lm":
        meta["lm"] = True
    elif case == "ac":
        meta["ac"] = "static"
    elif case == "nc":
        meta["nc"] = 7
        payload = bytes(BS.packed_bytes(7, al // 320, 10))
    elif case == "short":
        payload = payload[:-1]
    elif case == "long":
        payload = payload + b"\0"
    elif case == "magic":
        magic = b"ECDX"
    elif case == "version":
        version = 1
    elif case == "hop":
        meta["hop"] = 640
    with pytest.raises(ValueError, match="bad_file.ecdc"):
        BS.parse_ecdc(_blob(meta, payload, magic, version), "dir/bad_file.ecdc", 6)


def test_host_unpack_matches_bitpacker_order():
    from ladiffcodec_amd.decompress import unpack_rows
    rng = np.random.default_rng(1)
    n_q, B, F, bits = 3, 2, 5, 10
    codes = rng.integers(0, 1 << bits, (n_q, B, F))
    rows = []
    for b in range(B):                                  # BitPacker: for t: for k, LSB first
        acc, nbit, out = 0, 0, bytearray()
        for t in range(F):
            for k in range(n_q):
                acc |= int(codes[k, b, t]) << nbit
                nbit += bits
                while nbit >= 8:
                    out.append(acc & 0xFF); acc >>= 8; nbit -= 8
        if nbit:
            out.append(acc & 0xFF)
        rows.append(np.frombuffer(bytes(out), np.uint8))
    assert len(rows[0]) == BS.packed_bytes(n_q, F, bits)
    assert np.array_equal(unpack_rows(np.stack(rows), n_q, F, bits), codes)


def test_cli_parsers_take_the_sample_flags():
    from ladiffcodec_amd import compress, decompress, sample
    base = ["--model_for_cond", "c.amlt", "--model_path", "m.amlt", "--enc_ratios", "8", "4", "--input_dir", "in/",
            "--output_dir", "out/", "--midway_t", "30", "--in_flight", "1", "--seed", "3", "--chunk_sec", "2.0", "--cond_bandwidth", "1.5"]
    ref = vars(sample.build_parser().parse_args(base))
    a = vars(compress.build_parser().parse_args(base))
    assert a == ref
    d = decompress.build_parser().parse_args(base + ["--ddim_steps", "7", "--ddim_eta", "0.5"])
    assert {k: v for k, v in vars(d).items() if k not in ("ddim_steps", "ddim_eta")} == ref
    assert d.ddim_steps == 7 and d.ddim_eta == 0.5
    assert decompress.build_parser().parse_args(base).ddim_steps == 0
    s = decompress.sampler_from_args(decompress.build_parser().parse_args(base))
    assert isinstance(s, sample.CodesSampler) and isinstance(s.inner, sample.DdpmSampler) and s.draws == 30
    s = decompress.sampler_from_args(d)
    assert isinstance(s.inner, sample.DdimSampler) and (s.inner.t_start, s.inner.n_steps, s.inner.eta) == (30, 7, 0.5)
    with pytest.raises(SystemExit):
        decompress.sampler_from_args(decompress.build_parser().parse_args(base + ["--ddim_steps", "31"]))
    with pytest.raises(SystemExit):
        decompress.sampler_from_args(decompress.build_parser().parse_args(base + ["--ddim_steps", "3", "--ddim_eta", "2"]))


@pytest.mark.parametrize("mod", ["compress", "decompress"])
def test_cli_help_as_module(mod):
    r = subprocess.run([sys.executable, "-m", f"ladiffcodec_amd.{mod}", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--cond_bandwidth" in r.stdout and "--input_dir" in r.stdout
    assert ("--ddim_steps" in r.stdout) == (mod == "decompress")


def test_code_batches_move_like_tensors():
    import torch
    from ladiffcodec_amd.sample import CodesBatch, output_path
    b = CodesBatch(packed=torch.zeros(2, 15, dtype=torch.uint8), n_q=6, F=2)
    m = b.to("cpu", non_blocking=True)
    assert m.packed.shape == (2, 15) and m.codes is None and (m.n_q, m.F, m.bits) == (6, 2, 10)
    c = CodesBatch(codes=torch.zeros(3, 2, 8, dtype=torch.int64)).to("cpu")
    assert (c.n_q, c.F) == (3, 8)
    assert output_path("in/a/b.ecdc", "in/", "/o/", ".ecdc") == "/o/a/b.wav"
    assert output_path("in/a/b.wav", "in/", "/o/", ".wav", ".ecdc") == "/o/a/b.ecdc"
    assert output_path("in/a/b.wav", "in/", "/o/") == "/o/a/b.wav"
