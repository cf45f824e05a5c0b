"""`python -m ladiffcodec_amd.compress` -- the sender: every `**/*.wav` under `--input_dir` becomes an ECDC container of its RVQ codes.

Flags: those of `srcs.sample` (the checkpoints included: a context is built with both models, so `--model_path` is needed here
too).  Every file is read at 16 kHz and trimmed to a multiple of 640 samples (sample.py:87); files of equal length are encoded
in batches of `--batch_size` (sample.plan_batches), the codes computed at `--cond_bandwidth` (Engine.get_cond) and packed at
10 bits per code on the GPU (Bitstream.pack_codes).  `<output_dir><rel>.ecdc` holds the reference container
(compress.py:28-84 with use_lm False: keys m, al = trimmed length, nc, lm, hop) and the payload; a file of C > 1 channels
becomes one container with the extra key `ch: C` and its C payloads back to back.  `python -m ladiffcodec_amd.decompress`
turns the containers back into audio.

`--ragged [--ragged_waste W]` packs mono files of DIFFERENT lengths into shared encoder batches (sample.plan_ragged_batches at the
same 640-sample trim -- the sender does not know the receiver's UNet quantum -- and Engine.get_cond_ragged): every container is
byte-identical to the one the run without the flag writes.

`--stream_sec S` (default 0: off) encodes every mono file longer than S seconds through a stream session of the cond encoder
(Engine.open_stream) in chunks of S seconds, rounded down to whole 320-sample hops, the first chunk at least the session's `min_first`
samples: the activations of a call cover one chunk, not the recording.  Chunks of different files share calls as stream items; a file's
codes are joined and packed once, and the container is byte-identical to the one the run without the flag writes wherever the codes
agree.  The streamed encoder output equals the whole-file one to fp32 last bits (a chunk may sum in another order), so a frame whose two
nearest codebook entries are closer than that could take the other code: not seen on the test inputs, not excluded for arbitrary audio.
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import List

from .sample import build_parser

BITS = 10      # log2(bins): compress.py's BitPacker width
TRIM = 640     # sample.py:87


def ragged_options(a):
    """sample.ragged_options for the codec-end CLIs, which refuse a --ragged_waste that nothing would read."""
    from .sample import ragged_options as base
    ragged, waste = base(a)
    if not ragged and hasattr(a, "ragged_waste"):
        raise SystemExit("--ragged_waste needs --ragged")
    if waste < 0:
        raise SystemExit("--ragged_waste must be >= 0")
    return ragged, waste


def stream_options(a) -> float:
    """--stream_sec of a parsed namespace (0: off); a negative value is refused."""
    s = float(getattr(a, "stream_sec", 0.0) or 0.0)
    if s < 0:
        raise SystemExit("--stream_sec must be >= 0")
    return s


def _stream_sec_arg(v: str) -> float:
    s = float(v)
    if s < 0:
        raise argparse.ArgumentTypeError("--stream_sec must be >= 0")
    return s


def stream_codes(eng, wavs, idxs: List[int], ns: List[int], chunk: int, bandwidth: float):
    """RVQ codes [n_q, ns[k] // 320] of mono files idxs[k] through ONE stream session: the files are its items and advance together, by
    the scheduled chunk or by what the shortest unfinished file has left; a finished file's item is fed silence and ignored."""
    import numpy as np
    import torch
    from . import lib as L
    st = eng.open_stream(L.MODEL_COND, L.STREAM_ENCODER, len(idxs))
    try:
        pos, parts = [0] * len(idxs), [[] for _ in idxs]
        while any(p < n for p, n in zip(pos, ns)):
            left = min(n - p for p, n in zip(pos, ns) if p < n)
            t = min(left, max(chunk, st.min_first) if not any(pos) else chunk)
            x = np.zeros((len(idxs), 1, t), np.float32)
            for k, i in enumerate(idxs):
                if pos[k] < ns[k]:
                    x[k, 0] = wavs[i][0, pos[k]:pos[k] + t]
            _, codes = st.get_cond(torch.from_numpy(x).to(eng.device), bandwidth=bandwidth, return_codes=True)
            for k in range(len(idxs)):
                if pos[k] < ns[k]:
                    parts[k].append(codes[:, k])
                    pos[k] += t
        return [torch.cat(p, dim=1) for p in parts]
    finally:
        st.close()


def compress_files(eng, files: List[str], inp_args, rank: int = 0, world: int = 1) -> List[str]:
    """Encode and write this rank's files; -> the container paths written."""
    from .bitstream import Bitstream, ecdc_container
    from .bitstream import packed_bytes
    from .sample import LazyWavs, output_path, plan_batches, plan_ragged_batches

    ragged, waste = ragged_options(inp_args)
    stream_sec = stream_options(inp_args)
    bs = Bitstream(eng)
    wavs = LazyWavs(files, eng)
    keep = [i for i, sh in enumerate(wavs.shapes) if sh[1] // 640 * 640 > 0]                  # sample.py:87-88
    files, wavs = [files[i] for i in keep], wavs.subset(keep)
    lengths, channels = [sh[1] for sh in wavs.shapes], [sh[0] for sh in wavs.shapes]
    dev = eng.device
    written = []

    def write(i, n, payloads, n_q):
        path = output_path(files[i], inp_args.input_dir, inp_args.output_dir, ".wav", ".ecdc")
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "wb") as fo:
            fo.write(ecdc_container(payloads, n, n_q))
        written.append(path)

    if ragged:
        work = plan_ragged_batches(lengths, channels, rank, world, inp_args.batch_size, waste, TRIM)
    else:
        work = plan_batches(lengths, channels, rank, world, inp_args.batch_size)
    for idxs, joint in work:
        if stream_sec > 0 and not joint:      # long mono files: chunk by chunk through a stream session, packed once per file
            from . import lib as L
            chunk = max(320, int(stream_sec * 16000) // 320 * 320)
            floor = max(int(stream_sec * 16000), L.stream_min_first(eng._cfg, L.MODEL_COND, L.STREAM_ENCODER) - 1)
            long_ = [i for i in idxs if lengths[i] // TRIM * TRIM > floor]
            if long_:
                lns = [lengths[i] // TRIM * TRIM for i in long_]
                for i, n, codes in zip(long_, lns, stream_codes(eng, wavs, long_, lns, chunk, float(inp_args.cond_bandwidth))):
                    write(i, n, [bs.pack_codes(codes[:, None, :].contiguous(), BITS).cpu().numpy()[0].tobytes()], int(codes.shape[0]))
                    wavs.drop(i)
                idxs = [i for i in idxs if i not in long_]
                if not idxs:
                    continue
        ns = [lengths[i] // TRIM * TRIM for i in idxs]
        if ragged and not joint and len(set(ns)) > 1:
            # codes are zero behind an item's frames, so the first packed_bytes(n_q, F_b) bytes of its padded row are its solo pack
            _, codes = eng.get_cond_ragged(wavs.padded_batch(idxs, ns).to(dev), ns, bandwidth=float(inp_args.cond_bandwidth), return_codes=True)
        else:
            _, codes = eng.get_cond(wavs.batch(idxs, joint, ns[0]).to(dev), bandwidth=float(inp_args.cond_bandwidth), return_codes=True)
        rows = bs.pack_codes(codes, BITS).cpu().numpy()                                          # [B, packed bytes]
        n_q = int(codes.shape[0])
        if joint:
            groups = [(idxs[0], ns[0], [r.tobytes() for r in rows])]
        else:
            groups = [(i, n, [rows[k][:packed_bytes(n_q, n // 320, BITS)].tobytes()]) for k, (i, n) in enumerate(zip(idxs, ns))]
        for i, n, payloads in groups:
            write(i, n, payloads, n_q)
        for i in idxs:
            wavs.drop(i)
    return written


def compress(inp_args) -> List[str]:
    from . import parallel
    from .sample import _unsupported, build_engines

    _unsupported(inp_args)
    ragged_options(inp_args)                    # (refusals before anything is loaded)
    stream_options(inp_args)
    rank, local_rank, world = parallel.init_process_group("nccl")
    files = sorted(glob.glob(os.path.join(inp_args.input_dir, "**/*.wav"), recursive=True))
    inp_args.in_flight = 1                      # one engine: the encode has nothing to keep in flight
    (eng,) = build_engines(inp_args, files, rank, world, local_rank)
    try:
        return compress_files(eng, files, inp_args, rank, world)
    finally:
        eng.close()


def build_cli_parser():
    p = build_parser()
    p.description = "compress wav files to ECDC containers of their RVQ codes"
    p.add_argument("--stream_sec", type=_stream_sec_arg, default=0.0,
                   help="mono files longer than this many seconds are encoded chunk by chunk through a stream session of the cond encoder "
                        "(chunks of this length, whole 320-sample hops): activation memory of one chunk; the same containers as "
                        "a run without the flag, up to a code whose two nearest codebook entries tie within fp32 rounding; 0 = whole files")
    for act in p._actions:      # the shared flags, described for this CLI
        if act.dest == "ragged":
            act.help = ("encode mono files of DIFFERENT lengths in shared batches (Engine.get_cond_ragged); files are trimmed to 640 "
                        "samples as without the flag and every container is byte-identical to the one written without it")
    return p


def main(argv=None):
    return compress(build_cli_parser().parse_args(argv))


if __name__ == "__main__":
    main()
