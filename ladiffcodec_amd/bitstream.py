"""On-wire format of the RVQ codes: host-side mirror of the reference's
`srcs/encodec/binary.py` (ECDC header, BitPacker / BitUnpacker) and `srcs/quantization/ac.py` (arithmetic coder) on
top of the C ABI.  The byte work runs on the GPU (csrc/bitstream.hip), one independent stream per utterance; the
container (header + per-utterance payload) is assembled on the host exactly as `srcs/encodec/compress.py:28-84` lays it out.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import struct
import typing as tp

from . import lib as L

_encodec_header_struct = struct.Struct("!4sBI")      # binary.py:19
_ENCODEC_MAGIC = b"ECDC"


def write_ecdc_header(fo: tp.IO[bytes], metadata: tp.Any):
    """binary.py:22-28."""
    meta_dumped = json.dumps(metadata).encode("utf-8")
    fo.write(_encodec_header_struct.pack(_ENCODEC_MAGIC, 0, len(meta_dumped)))
    fo.write(meta_dumped)
    fo.flush()


def _read_exactly(fo: tp.IO[bytes], size: int) -> bytes:
    buf = b""
    while len(buf) < size:
        new_buf = fo.read(size)
        if not new_buf:
            raise EOFError("Impossible to read enough data from the stream, " f"{size} bytes remaining.")
        buf += new_buf
        size -= len(new_buf)
    return buf


def read_ecdc_header(fo: tp.IO[bytes]):
    """binary.py:43-52."""
    magic, version, meta_size = _encodec_header_struct.unpack(_read_exactly(fo, _encodec_header_struct.size))
    if magic != _ENCODEC_MAGIC:
        raise ValueError("File is not in ECDC format.")
    if version != 0:
        raise ValueError("Version not supported.")
    return json.loads(_read_exactly(fo, meta_size).decode("utf-8"))


MODEL_NAME = "ladiffcodec_16khz"      # the container's `m`


def packed_bytes(n_q: int, F: int, bits: int = 10) -> int:
    """ldc_packed_bytes on the host: BitPacker bytes of n_q * F codes of `bits` bits."""
    return (int(n_q) * int(F) * int(bits) + 7) // 8


def ecdc_meta(audio_length: int, n_q: int, model_name: str = MODEL_NAME, hop_length: int = 320, channels: int = 1) -> dict:
    """Header fields as compress.py:47-71 writes them (lm: plain packing); a multi-channel container adds `ch`."""
    meta = {"m": model_name, "al": int(audio_length), "nc": int(n_q), "lm": False, "hop": int(hop_length)}
    if channels > 1:
        meta["ch"] = int(channels)
    return meta


def ecdc_container(payloads: tp.Sequence[bytes], audio_length: int, n_q: int, model_name: str = MODEL_NAME,
                   hop_length: int = 320) -> bytes:
    """One container: header + the packed payloads of its channels back to back (one channel: the reference's layout)."""
    fo = io.BytesIO()
    write_ecdc_header(fo, ecdc_meta(audio_length, n_q, model_name, hop_length, len(payloads)))
    for p in payloads:
        fo.write(p)
    return fo.getvalue()


def parse_ecdc(blob: bytes, name: str, n_q_layers: int, bits: int = 10, model_name: str = MODEL_NAME, hop_length: int = 320):
    """Validate a plainly packed container on the host -> (meta, payload rows uint8 [ch, packed_bytes], F).  Every refusal is a
    ValueError naming `name`: bad magic / version, another model, an LM-coded (`lm: true`) or arithmetic-coded (`ac`) payload,
    nc outside [1, n_q_layers], another hop, a payload that is not exactly ch x packed_bytes(nc, F, bits) long."""
    import numpy as np
    fo = io.BytesIO(blob)
    try:
        meta = read_ecdc_header(fo)
    except (ValueError, EOFError, struct.error, UnicodeDecodeError) as e:
        raise ValueError(f"{name}: {e}") from None
    if not isinstance(meta, dict):
        raise ValueError(f"{name}: header metadata is not an object")
    if meta.get("m") != model_name:
        raise ValueError(f"{name}: model {meta.get('m')!r}, expected {model_name!r}")
    if meta.get("lm", False) is not False:
        raise ValueError(f"{name}: payload is coded with a language model (lm: true): not decodable here")
    if "ac" in meta:
        raise ValueError(f"{name}: payload is arithmetic-coded (ac: {meta['ac']!r}): not decodable here")
    nc, al, hop, ch = meta.get("nc"), meta.get("al"), meta.get("hop", 320), meta.get("ch", 1)
    if not all(isinstance(v, int) and not isinstance(v, bool) for v in (nc, al, hop, ch)):
        raise ValueError(f"{name}: nc / al / hop / ch must be integers")
    if not 1 <= nc <= n_q_layers:
        raise ValueError(f"{name}: nc {nc} outside [1, {n_q_layers}]")
    if hop != hop_length:
        raise ValueError(f"{name}: hop {hop}, expected {hop_length}")
    if al < 1 or ch < 1:
        raise ValueError(f"{name}: al {al} / ch {ch} must be positive")
    F = -(-al // hop)
    nb = packed_bytes(nc, F, bits)
    payload = fo.read()
    if len(payload) != ch * nb:
        raise ValueError(f"{name}: payload of {len(payload)} bytes, expected {ch} x {nb}")
    return meta, np.frombuffer(payload, np.uint8).reshape(ch, nb), F


class Bitstream:
    """GPU bit packer / range coder bound to an Engine's context and stream."""

    def __init__(self, eng):
        self.eng, self.lib, self.torch = eng, eng.lib, eng.torch

    # ---- BitPacker / BitUnpacker over code frames ---------------------------------------------------------------
    def pack_codes(self, codes, bits: int = 10):
        """codes [n_q, B, F] int64 -> uint8 [B, ceil(n_q*F*bits/8)], every row = BitPacker over `for t: for k: codes[k, b, t]`
        (compress.py:74-84) + flush."""
        t = self.torch
        codes = codes.to(self.eng.device, t.int64).contiguous()
        n_q, B, F = codes.shape
        nb = int(self.lib.ldc_packed_bytes(n_q, F, bits))
        out = t.empty(B, max(nb, 1), dtype=t.uint8, device=self.eng.device)
        if nb == 0:                       # an empty frame packs to nothing (BitPacker.flush without a push writes no byte)
            return out[:, :0]
        s = self.eng._enter()
        L.check(self.lib.ldc_pack_codes(self.eng._ctx, codes.data_ptr(), n_q, B, F, bits, out.data_ptr(), out.stride(0), s))
        self.eng._exit()
        return out[:, :nb]

    def unpack_codes(self, data, n_q: int, F: int, bits: int = 10):
        t = self.torch
        data = data.to(self.eng.device, t.uint8).contiguous()
        B = data.shape[0]
        if data.shape[1] < int(self.lib.ldc_packed_bytes(n_q, F, bits)):
            raise EOFError("The stream ended sooner than expected.")       # compress.py:148-149
        codes = t.empty(n_q, B, F, dtype=t.int64, device=self.eng.device)
        s = self.eng._enter()
        L.check(self.lib.ldc_unpack_codes(self.eng._ctx, data.data_ptr(), data.stride(0), n_q, B, F, bits, codes.data_ptr(), s))
        self.eng._exit()
        return codes

    # ---- arithmetic coder -----------------------------------------------------------------------------------------
    def build_cdf(self, pdf, total_range_bits: int = 24, roundoff: float = 1e-8, min_range: int = 2):
        """build_stable_quantized_cdf (ac.py:18-53) of every row of pdf [..., card] -> int32 cdf of the same shape."""
        t = self.torch
        pdf = pdf.to(self.eng.device, t.float32).contiguous()
        card = pdf.shape[-1]
        rows = pdf.numel() // card
        cdf = t.empty(pdf.shape, dtype=t.int32, device=self.eng.device)
        s = self.eng._enter()
        L.check(self.lib.ldc_ac_build_cdf(self.eng._ctx, pdf.data_ptr(), rows, card, total_range_bits, float(roundoff), min_range,
                                          cdf.data_ptr(), s))
        self.eng._exit()
        return cdf

    def ac_encode(self, symbols, cdf, static: bool = False, total_range_bits: int = 24, capacity: tp.Optional[int] = None,
                  n_sym: tp.Optional[tp.Sequence[int]] = None):
        """symbols [B, S]; cdf [B, S, card] (static=False) or [n, card] with symbol s using table s % n (static=True).
        -> list of B `bytes` (ArithmeticCoder pushes + flush of every stream).  n_sym (optional, B counts <= S): stream b codes its
        first n_sym[b] symbols only (ldc_ac_encode_ragged) -- the bytes of a call on the item alone with S = n_sym[b]."""
        t = self.torch
        symbols = symbols.to(self.eng.device, t.int32).contiguous()
        cdf = cdf.to(self.eng.device, t.int32).contiguous()
        B, S = symbols.shape
        card = cdf.shape[-1]
        cap = int(capacity) if capacity else S * 4 + 64           # 30-bit range: a symbol costs < 32 bits
        out = t.empty(B, cap, dtype=t.uint8, device=self.eng.device)
        nbytes = t.empty(B, dtype=t.int64, device=self.eng.device)
        s = self.eng._enter()
        if n_sym is None:
            L.check(self.lib.ldc_ac_encode(self.eng._ctx, symbols.data_ptr(), cdf.data_ptr(), B, S, card, cdf.shape[0] if static else 0,
                                           total_range_bits, out.data_ptr(), out.stride(0), nbytes.data_ptr(), s))
        else:
            cnt = self._counts(n_sym, B, S)
            L.check(self.lib.ldc_ac_encode_ragged(self.eng._ctx, symbols.data_ptr(), cnt.data_ptr(), cdf.data_ptr(), B, S, card,
                                                  cdf.shape[0] if static else 0, total_range_bits, out.data_ptr(), out.stride(0),
                                                  nbytes.data_ptr(), s))
        self.eng._exit()
        n = nbytes.cpu().tolist()
        if min(n) < 0:
            raise ValueError("arithmetic coder: a symbol lies outside its table or the output capacity is too small")
        host = out.cpu().numpy()
        return [host[b, :n[b]].tobytes() for b in range(B)]

    def _counts(self, n_sym, B: int, S: int):
        n_sym = [int(v) for v in n_sym]
        if len(n_sym) != B or min(n_sym) < 0 or max(n_sym) > S:
            raise ValueError(f"n_sym: {B} counts in [0, {S}] expected")
        return self.torch.tensor(n_sym, dtype=self.torch.int32, device=self.eng.device)

    def ac_decode(self, streams: tp.Sequence[bytes], S: int, cdf, static: bool = False, total_range_bits: int = 24,
                  n_sym: tp.Optional[tp.Sequence[int]] = None):
        """-> symbols [B, S] int32; raises EOFError where ArithmeticDecoder.pull would return None (compress.py:148-149).
        n_sym (optional): stream b holds n_sym[b] <= S symbols (ldc_ac_decode_ragged); the symbols behind them come out 0."""
        import numpy as np
        t = self.torch
        B = len(streams)
        width = max(1, max(len(x) for x in streams))
        host = np.zeros((B, width), np.uint8)
        for b, x in enumerate(streams):
            host[b, :len(x)] = np.frombuffer(x, np.uint8)
        data = t.from_numpy(host).to(self.eng.device)
        nbytes = t.tensor([len(x) for x in streams], dtype=t.int64, device=self.eng.device)
        cdf = cdf.to(self.eng.device, t.int32).contiguous()
        symbols = t.zeros(B, S, dtype=t.int32, device=self.eng.device)
        status = t.zeros(B, dtype=t.int32, device=self.eng.device)
        s = self.eng._enter()
        if n_sym is None:
            L.check(self.lib.ldc_ac_decode(self.eng._ctx, data.data_ptr(), data.stride(0), nbytes.data_ptr(), cdf.data_ptr(), B, S,
                                           cdf.shape[-1], cdf.shape[0] if static else 0, total_range_bits, symbols.data_ptr(),
                                           status.data_ptr(), s))
        else:
            cnt = self._counts(n_sym, B, S)
            L.check(self.lib.ldc_ac_decode_ragged(self.eng._ctx, data.data_ptr(), data.stride(0), nbytes.data_ptr(), cnt.data_ptr(),
                                                  cdf.data_ptr(), B, S, cdf.shape[-1], cdf.shape[0] if static else 0, total_range_bits,
                                                  symbols.data_ptr(), status.data_ptr(), s))
        self.eng._exit()
        st = status.cpu().tolist()
        if any(v == 1 for v in st):
            raise EOFError("The stream ended sooner than expected.")
        if any(v == 2 for v in st):
            raise RuntimeError("Binary search failed")               # ac.py:241
        return symbols

    # ---- container: compress.py:28-84 / 87-156 with use_lm = False (plain packing) or a static per-codebook model ----------
    def compress_codes(self, codes, audio_length: int, model_name: str = "ladiffcodec_16khz", bits: int = 10,
                       static_cdf=None, hop_length: int = 320) -> tp.List[bytes]:
        """codes [n_q, B, F] -> one ECDC byte string per utterance (header + payload).

        Header fields as compress.py:47-71 writes them; `lm` keeps the reference's meaning (payload arithmetic-coded with the
        model's LM pdfs, compress.py:118-141), which this library never produces, so it is always false.  A payload coded with
        a caller-supplied static per-codebook table says so in its own field `ac: "static"`; a reference decoder that meets
        it reads `lm: false`, plain-unpacks and finds the stream too short instead of silently mis-decoding.

        audio_length: one length for the batch, or a list of B lengths for items of different lengths (codes right-padded to F =
        the longest item's frames, ZERO behind an item's frames, as Engine.get_cond_ragged returns them).  Either way one device
        call; every container is byte-identical to the one the item gives alone: a plain payload is the first
        packed_bytes(n_q, F_b, bits) bytes of its padded row (zero codes behind F_b leave the last partial byte as the solo pack
        writes it), a static one codes n_q * F_b symbols (ac_encode's n_sym)."""
        n_q, B, F = codes.shape
        ragged = hasattr(audio_length, "__len__")
        als = [int(v) for v in audio_length] if ragged else [int(audio_length)] * B
        frames = [-(-al // int(hop_length)) for al in als]
        if len(als) != B or max(frames) != F or min(frames) < 1:
            raise ValueError(f"audio_length {audio_length} does not give {F} frames at hop {hop_length}")
        if static_cdf is None:
            rows = self.pack_codes(codes, bits).cpu().numpy()
            payloads = [bytes(r[:packed_bytes(n_q, fb, bits)]) for r, fb in zip(rows, frames)]
        else:
            if static_cdf.shape[0] != n_q:
                raise ValueError(f"static_cdf has {static_cdf.shape[0]} tables for {n_q} codebooks (symbol s uses table s % n_q)")
            sym = codes.permute(1, 2, 0).reshape(B, F * n_q)          # push order: t outer, k inner
            payloads = self.ac_encode(sym, static_cdf, static=True, n_sym=[n_q * fb for fb in frames] if ragged else None)
        out = []
        for b in range(B):
            fo = io.BytesIO()
            meta = ecdc_meta(als[b], n_q, model_name, hop_length)
            if static_cdf is not None:
                meta["ac"] = "static"
            write_ecdc_header(fo, meta)
            fo.write(payloads[b])
            out.append(fo.getvalue())
        return out

    def decompress_codes(self, blobs: tp.Sequence[bytes], F: tp.Optional[int] = None, bits: int = 10, static_cdf=None,
                         ragged: bool = False):
        """-> (codes [n_q, B, F] int64, list of metadata).  F is derived from the header (`al`, `hop`) and, when given, must agree.
        ragged: the containers may differ in length -- codes [n_q, B, Fmax], zero behind an item's own frames (its header's), still
        one device call."""
        import numpy as np
        if ragged:
            return self._decompress_ragged(blobs, bits, static_cdf)
        metas, payloads = [], []
        for blob in blobs:
            fo = io.BytesIO(blob)
            metas.append(read_ecdc_header(fo))
            payloads.append(fo.read())
        n_q = metas[0]["nc"]
        if any(m["nc"] != n_q for m in metas):
            raise ValueError("streams of one batch must share the number of codebooks")
        for m in metas:
            if m.get("lm"):
                raise ValueError("stream is coded with a language model (lm: true): not produced nor decodable here")
            mode = m.get("ac", "none")
            if mode not in ("none", "static"):
                raise ValueError(f"unknown entropy-coding mode {mode!r}")
            if (mode == "static") != (static_cdf is not None):
                raise ValueError("stream is static-table arithmetic-coded: pass the table it was coded with" if mode == "static"
                                 else "stream is plainly packed: static_cdf must not be given")
            frames = -(-int(m["al"]) // int(m.get("hop", 320)))
            if F is None:
                F = frames
            if frames != F:
                raise ValueError(f"header says {frames} frames (al {m['al']}), caller expects {F}")
        if static_cdf is None:
            width = max(len(p) for p in payloads)
            host = np.zeros((len(payloads), max(width, 1)), np.uint8)
            for b, p in enumerate(payloads):
                host[b, :len(p)] = np.frombuffer(p, np.uint8)
            if min(len(p) for p in payloads) < int(self.lib.ldc_packed_bytes(n_q, F, bits)):
                raise EOFError("The stream ended sooner than expected.")
            return self.unpack_codes(self.torch.from_numpy(host), n_q, F, bits), metas
        if static_cdf.shape[0] != n_q:
            raise ValueError(f"static_cdf has {static_cdf.shape[0]} tables for {n_q} codebooks")
        sym = self.ac_decode(payloads, F * n_q, static_cdf, static=True)
        return sym.reshape(len(payloads), F, n_q).permute(2, 0, 1).contiguous().to(self.torch.int64), metas

    def _decompress_ragged(self, blobs, bits, static_cdf):
        import numpy as np
        t = self.torch
        metas, payloads = [], []
        for blob in blobs:
            fo = io.BytesIO(blob)
            metas.append(read_ecdc_header(fo))
            payloads.append(fo.read())
        n_q = metas[0]["nc"]
        if any(m["nc"] != n_q for m in metas):
            raise ValueError("streams of one batch must share the number of codebooks")
        for m in metas:
            if m.get("lm"):
                raise ValueError("stream is coded with a language model (lm: true): not produced nor decodable here")
            mode = m.get("ac", "none")
            if mode not in ("none", "static"):
                raise ValueError(f"unknown entropy-coding mode {mode!r}")
            if (mode == "static") != (static_cdf is not None):
                raise ValueError("stream is static-table arithmetic-coded: pass the table it was coded with" if mode == "static"
                                 else "stream is plainly packed: static_cdf must not be given")
        frames = [-(-int(m["al"]) // int(m.get("hop", 320))) for m in metas]
        B, F = len(blobs), max(frames)
        if static_cdf is not None:
            if static_cdf.shape[0] != n_q:
                raise ValueError(f"static_cdf has {static_cdf.shape[0]} tables for {n_q} codebooks")
            sym = self.ac_decode(payloads, F * n_q, static_cdf, static=True, n_sym=[n_q * fb for fb in frames])
            return sym.reshape(B, F, n_q).permute(2, 0, 1).contiguous().to(t.int64), metas
        if any(len(p) < packed_bytes(n_q, fb, bits) for p, fb in zip(payloads, frames)):
            raise EOFError("The stream ended sooner than expected.")
        # rows are zero behind a payload's own bytes; the spare bits of an item's last byte are whatever its writer left there, so the
        # codes behind its frames are cleared explicitly
        host = np.zeros((B, max(packed_bytes(n_q, F, bits), 1)), np.uint8)
        for b, (p, fb) in enumerate(zip(payloads, frames)):
            nb = packed_bytes(n_q, fb, bits)
            host[b, :nb] = np.frombuffer(p[:nb], np.uint8)
        codes = self.unpack_codes(t.from_numpy(host), n_q, F, bits)
        keep = t.arange(F, device=codes.device)[None, :] < t.tensor(frames, device=codes.device)[:, None]
        return codes * keep[None].to(codes.dtype), metas
