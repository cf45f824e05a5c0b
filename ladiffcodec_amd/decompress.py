"""`python -m ladiffcodec_amd.decompress` -- the receiver: every `**/*.ecdc` under `--input_dir` becomes `<output_dir><rel>.wav`.

Flags: those of `srcs.sample` plus `--ddim_steps` (0: the DDPM halfway sampling of `--midway_t` steps, the default) and
`--ddim_eta`, checked as `sample_ddim` checks them, and `--dpm_steps` (0: off, the default; > 0: DPM-Solver++(2M) from `--midway_t`,
checked as `sample_dpm` checks it; refused together with `--ddim_steps` > 0 and, having no ragged decode from codes, with
`--ragged`).  Every container is validated on the host first (magic, version, `m`,
`lm` false, no `ac`, nc <= the codebooks of the model, hop 320, payload exactly ch x packed bytes); a file that fails stops the
run before anything is decoded, with an error naming it.  The payload rows go to the GPU as they are and the decode starts
from them (Engine.decode_codes): the cond encoder does not run.  Batching, per-item / joint normalisation, `--in_flight`,
`--seed`, rank sharding and `--chunk_sec` are those of `srcs.sample` (sample.decode_files over a container source); a long
mono stream under `--chunk_sec` is cut at frame counts that are multiples of chunk_quantum / 320, its chunks decoded as batch
items and their raw decoder outputs joined and normalised over the whole recording.  The codes of such a recording come from
a whole-file encode, so that output is not `srcs.sample --chunk_sec` of the waveform.
`--chunk_sec C --chunk_overlap_sec S` (checked as `srcs.sample` checks them) decodes such a stream on COUPLED windows instead
(Engine.decode_codes_windows, with `--dpm_steps` Engine.decode_codes_dpm_windows: one shared latent, no seams); a stream that needs
more than 32 windows is cut into segments of codes at whole condition frames, decoded one after another and hard-joined.

`--item_seeds` (as in `srcs.sample`): container i of the run's file list draws under seed (`--seed` + i) mod 2^64 as if decoded alone
(Engine.decode_codes_seeded), in equal-length batches and with `--ragged`; its audio depends neither on `--batch_size`, the packing,
`--in_flight` nor the number of ranks.  Not with `--chunk_sec` > 0, `--dpm_steps` or multi-channel containers.

`--ragged [--ragged_waste W]` decodes mono containers of DIFFERENT lengths in shared batches (plan_container_batches,
Engine.decode_codes_ragged): containers are grouped by (nc, bits, mode) and those whose frame count -- from the header -- is a
multiple of chunk_quantum / 320 are packed within the waste bound; the others (a sender trims to 640 samples, not to the receiver's
quantum) and multi-channel files keep the per-length batches, untrimmed.  Every file decodes as it does without the flag.
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Tuple

import numpy as np

from .sample import CodesBatch, build_parser as _base_parser

BITS = 10

_FLAGS = [
    ("--ddim_steps", dict(type=int, default=0, help="DDIM iterations from --midway_t (at most --midway_t); 0 = DDPM halfway sampling")),
    ("--ddim_eta", dict(type=float, default=0.0, help="DDIM eta in [0, 1]")),
    # (absent from the parsed namespace unless given: read with dpm_steps(a))
    ("--dpm_steps", dict(type=int, default=argparse.SUPPRESS,
                         help="DPM-Solver++(2M) iterations from --midway_t (at most --midway_t); 0 or absent = off; not with --ddim_steps > 0")),
]


def build_parser() -> argparse.ArgumentParser:
    p = _base_parser()
    p.description = "decompress ECDC containers of RVQ codes to wav files"
    for flag, kw in _FLAGS:
        p.add_argument(flag, **kw)
    for act in p._actions:      # the shared flag, described for this CLI
        if act.dest == "ragged":
            act.help = ("decode mono containers of DIFFERENT lengths in shared batches (Engine.decode_codes_ragged); only containers "
                        "whose frame count is a multiple of the chunk quantum / 320 (8 frames for --enc_ratios 8 4) are packed, the "
                        "others keep the equal-length batches; nothing is trimmed")
    return p


def plan_container_batches(metas: List[dict], rank: int, world: int, batch_size: int, waste: float, quantum: int,
                           bits: int = BITS) -> List[Tuple[List[int], bool, bool]]:
    """--ragged work list of one rank over container headers: [(indices, joint, ragged)].  The files are dealt to the ranks as
    plan_batches deals them (parallel.shard_utterances over `al`); a batch shares (nc, bits, mode).  Mono containers whose length is
    a positive multiple of `quantum` samples are packed by plan_ragged_batches' rule (longest first, at most batch_size, closed before
    B * Tmax exceeds (1 + waste) x the samples held) -- ragged; every other container falls back to plan_batches' equal-length
    batches (multi-channel ones alone, joint) -- not ragged."""
    from . import parallel
    from .sample import plan_batches, plan_ragged_batches
    lengths = [int(m["al"]) for m in metas]
    mine = parallel.shard_utterances(lengths, rank, world)
    groups: Dict[tuple, List[int]] = {}
    for i in mine:
        groups.setdefault((int(metas[i]["nc"]), int(bits), str(metas[i].get("ac", "none"))), []).append(i)
    work: List[Tuple[List[int], bool, bool]] = []
    for _, idx in sorted(groups.items()):
        is_al = [int(metas[i].get("ch", 1)) == 1 and lengths[i] % quantum == 0 for i in idx]
        aligned = [i for i, ok in zip(idx, is_al) if ok]
        rest = [i for i, ok in zip(idx, is_al) if not ok]
        # (rank 0 of a world of 1: the sub-lists are this rank's already)
        for sub, _ in plan_ragged_batches([lengths[i] for i in aligned], [1] * len(aligned), 0, 1, batch_size, waste, quantum):
            work.append(([aligned[k] for k in sub], False, True))
        for sub, joint in plan_batches([lengths[i] for i in rest], [int(metas[i].get("ch", 1)) for i in rest], 0, 1, batch_size):
            work.append(([rest[k] for k in sub], joint, False))
    return work


def dpm_steps(a) -> int:
    return int(getattr(a, "dpm_steps", 0) or 0)


def sampler_from_args(a):
    from .sample import CodesSampler, DdpmSampler
    from .sample_ddim import sampler_from_args as ddim_sampler
    if dpm_steps(a) < 0:
        raise SystemExit(f"--dpm_steps {a.dpm_steps}: must be >= 0")
    if dpm_steps(a) > 0:
        from .sample_dpm import sampler_from_args as dpm_sampler
        if a.ddim_steps > 0:
            raise SystemExit(f"--dpm_steps {a.dpm_steps} and --ddim_steps {a.ddim_steps}: choose one sampler")
        if getattr(a, "ragged", False):
            raise SystemExit("--dpm_steps has no ragged decode from codes: run without --ragged")
        return CodesSampler(dpm_sampler(a))
    return CodesSampler(ddim_sampler(a) if a.ddim_steps > 0 else DdpmSampler(a.midway_t))


def unpack_rows(rows: np.ndarray, n_q: int, F: int, bits: int = BITS) -> np.ndarray:
    """BitUnpacker on the host: payload rows [B, >= packed bytes] -> codes [n_q, B, F] int64 (push order for t: for k)."""
    B = rows.shape[0]
    b = np.unpackbits(np.ascontiguousarray(rows), axis=1, bitorder="little")[:, :n_q * F * bits].reshape(B, F, n_q, bits)
    vals = (b.astype(np.int64) << np.arange(bits, dtype=np.int64)).sum(-1)
    return np.ascontiguousarray(vals.transpose(2, 0, 1))


class EcdcSource:
    """decode_files' batch source over validated containers: shapes (channels, al); batches of payload rows (CodesBatch)."""

    in_ext = ".ecdc"

    def __init__(self, files: List[str], n_q_layers: int):
        from .bitstream import parse_ecdc
        self.files = files
        self.parsed = []
        for f in files:
            with open(f, "rb") as fo:
                self.parsed.append(parse_ecdc(fo.read(), f, n_q_layers, BITS))
        self.shapes = [(rows.shape[0], int(meta["al"])) for meta, rows, _ in self.parsed]
        self._codes: Dict[int, np.ndarray] = {}

    def subset(self, idx: List[int]) -> "EcdcSource":
        out = EcdcSource.__new__(EcdcSource)
        out.files = [self.files[i] for i in idx]
        out.parsed = [self.parsed[i] for i in idx]
        out.shapes = [self.shapes[i] for i in idx]
        out._codes = {}
        return out

    def __len__(self):
        return len(self.files)

    def n_q(self, i: int) -> int:
        return int(self.parsed[i][0]["nc"])

    def batch(self, idxs: List[int], joint: bool, n: int) -> CodesBatch:
        """payload rows [B, packed bytes] of the files' first n // 320 frames (their full length: al is trimmed by compress)"""
        import torch
        rows = self.parsed[idxs[0]][1] if joint else np.stack([self.parsed[i][1][0] for i in idxs])
        n_q = {self.n_q(i) for i in idxs}
        if len(n_q) != 1:
            raise ValueError(f"one batch mixes numbers of codebooks {sorted(n_q)}")
        return CodesBatch(packed=torch.from_numpy(np.array(rows)), n_q=n_q.pop(), F=n // 320, bits=BITS)

    def plan_ragged(self, rank: int, world: int, batch_size: int, waste: float, quantum: int):
        return plan_container_batches([m for m, _, _ in self.parsed], rank, world, batch_size, waste, quantum)

    def ragged_batch(self, idxs: List[int], quantum: int):
        """-> (RaggedCodesBatch: row b = container idxs[b]'s own payload, zeros behind it; the items' lengths in samples)"""
        import torch
        from .sample import RaggedCodesBatch
        n_q = {self.n_q(i) for i in idxs}
        if len(n_q) != 1:
            raise ValueError(f"one batch mixes numbers of codebooks {sorted(n_q)}")
        rows = [self.parsed[i][1][0] for i in idxs]
        packed = np.zeros((len(idxs), max(len(r) for r in rows)), np.uint8)
        for b, r in enumerate(rows):
            packed[b, :len(r)] = r
        return RaggedCodesBatch(torch.from_numpy(packed), n_q.pop(), [self.parsed[i][2] for i in idxs], BITS), [self.shapes[i][1] for i in idxs]

    def chunk_batch(self, part: List[Tuple[int, int, int]], ln: int) -> CodesBatch:
        """codes [n_q, len(part), ln // 320] of chunks (file, order, start sample) of mono streams"""
        import torch
        out = []
        for i, _, st in part:
            if i not in self._codes:
                meta, rows, F = self.parsed[i]
                self._codes[i] = unpack_rows(rows, self.n_q(i), F)
            out.append(self._codes[i][:, 0, st // 320:(st + ln) // 320])
        return CodesBatch(codes=torch.from_numpy(np.ascontiguousarray(np.stack(out, axis=1))))


def decompress(inp_args) -> List[str]:
    from . import parallel
    from .sample import _unsupported, build_engines, decode_files, windows_options
    from .spec import CodecConfig

    from .compress import ragged_options
    _unsupported(inp_args)
    ragged_options(inp_args)                        # (refusals before anything is loaded)
    windows_options(inp_args)                       # (likewise: --chunk_overlap_sec needs --chunk_sec and is at most half of it)
    sampler = sampler_from_args(inp_args)
    # the codebooks the cond quantizer is built with (as build_engines builds it: ratios [8,5,4,2] at --cond_bandwidth)
    n_q_layers = CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=inp_args.cond_bandwidth).n_q_layers
    files = sorted(glob.glob(os.path.join(inp_args.input_dir, "**/*.ecdc"), recursive=True))
    source = EcdcSource(files, n_q_layers)          # every header is checked before anything is decoded
    rank, local_rank, world = parallel.init_process_group("nccl")
    engines = build_engines(inp_args, files, rank, world, local_rank)
    written = []
    try:
        # a batch shares its number of codebooks: one pass per nc (a run written by one compress call has one)
        for nc in sorted({source.n_q(i) for i in range(len(files))}):
            idx = [i for i in range(len(files)) if source.n_q(i) == nc]
            # (--item_seeds: a container is seeded by its index in the run's file list, not in its pass)
            kw = dict(run_index=idx) if getattr(inp_args, "item_seeds", False) else {}
            written += decode_files(engines if len(engines) > 1 else engines[0], [files[i] for i in idx], inp_args, rank, world,
                                    local_rank, sampler=sampler, source=source.subset(idx), **kw)
    finally:
        for eng in engines:
            eng.close()
    return written


def main(argv=None):
    return decompress(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
