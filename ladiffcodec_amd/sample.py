"""`python -m srcs.sample` -- the synthesis CLI of the reference (srcs/sample.py:50-203) on the MI355X engine.

Same flags, defaults and output naming as the reference.  What differs, by design:
  * mono files are decoded in BATCHES of equal trimmed length (the reference walks them one by one,
    sample.py:73); every utterance is normalised on its own, which is what the reference computes for
    a mono file (its "batch" is the channel axis of one file, sample.py:85,129,133-134).  A
    multi-channel file is decoded as ONE batch of its channels with the reference's joint
    (whole-tensor) normalisation, so its channels keep their relative levels exactly as in the reference;
  * `midway_t` (a literal 100 at sample.py:69) is a flag, `--midway_t`, default 100;
  * `--seed` (default 0) seeds the device noise stream (rank r uses seed + r); every decode call draws fresh noise,
    as torch.randn_like does in the reference (ddpm_loss.py:249);
  * `--ragged` batches mono files of DIFFERENT lengths (plan_ragged_batches, Engine.decode_ragged): every file is still decoded
    as if alone, but trimmed to the chunk quantum (2560 samples for `--enc_ratios 8 4`) instead of the reference's 640;
  * `--chunk_overlap_sec S` (with `--chunk_sec`) decodes a long mono recording on coupled windows that overlap by S seconds
    (Engine.decode_windows: one shared latent, no seams) instead of as independent chunks -- also in `sample_ddim`, `sample_dpm`
    and, from the container's codes, in `decompress`;
  * `--window_group` (with `--chunk_overlap_sec`; `sample`, `sample_ddim`, `sample_dpm`) decodes SEVERAL such recordings per call
    (Engine.decode_windows_group: the windows of a group, at most 32 in all, share one batch; file order, first fit).  Recording i of
    the run's file list draws under seed (`--seed` + i) mod 2^64, whatever group or rank it lands in;
  * `--item_seeds` (`sample`, `sample_ddim`, `decompress`; equal-length batches and `--ragged`) seeds every mono file on its own
    (Engine.decode_seeded / decode_codes_seeded): file i of the run's file list draws under seed (`--seed` + i) mod 2^64 exactly as
    if it were decoded alone, so its audio depends neither on `--batch_size`, the `--ragged` packing, `--in_flight` nor the number
    of ranks.  Refused with `--chunk_sec` > 0 and on multi-channel files;
  * under `torch.distributed.run` the FILE list is sharded over the ranks (one process per GPU; all channels of a
    file stay on one rank, every output file has exactly one writer).
Flags that are inert in the reference stay accepted and inert (`--sampling_timesteps`,
`--cond_enc_ratios`: quirk Q1, the cond codec is always built with ratios [8,5,4,2]).
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

# (flag, kwargs) in the reference's order -- srcs/sample.py:141-198
_FLAGS: List[Tuple[str, dict]] = [
    ("--data_folder_path", dict(type=str, default="/data/hy17/librispeech/librispeech")),
    ("--n_spks", dict(type=int, default=500)),
    ("--seq_len_in_sec", dict(type=float, default=1.8)),
    ("--sample_rate", dict(type=int, default=16000)),
    ("--model_path", dict(type=str, default="")),
    ("--qtzer_path", dict(type=str, default="")),
    ("--note", dict(type=str, default="")),
    ("--rep_dims", dict(type=int, default=128)),
    ("--emb_dims", dict(type=int, default=128)),
    ("--quantization", dict(dest="quantization", action="store_true")),
    ("--bandwidth", dict(type=float, default=3.0)),
    ("--n_filters", dict(type=int, default=32)),
    ("--lstm", dict(type=int, default=2)),
    ("--n_residual_layers", dict(type=int, default=1)),
    ("--enc_ratios", dict(nargs="+", type=int, default=[8])),
    ("--final_activation", dict(type=str, default=None)),
    ("--run_diff", dict(dest="run_diff", action="store_true")),
    ("--run_vae", dict(dest="run_vae", action="store_true")),
    ("--train_time_diff", dict(dest="train_time_diff", action="store_true")),
    ("--diff_dims", dict(type=int, default=256)),
    ("--qtz_condition", dict(dest="qtz_condition", action="store_true")),
    ("--self_condition", dict(dest="self_condition", action="store_true")),
    ("--seq_length", dict(type=int, default=16000)),
    ("--model_type", dict(type=str, default="unet")),
    ("--scaling_frame", dict(dest="scaling_frame", action="store_true")),
    ("--scaling_feature", dict(dest="scaling_feature", action="store_true")),
    ("--scaling_global", dict(dest="scaling_global", action="store_true")),
    ("--scaling_dim", dict(dest="scaling_dim", action="store_true")),
    ("--sampling_timesteps", dict(type=int, default=1000)),
    ("--use_film", dict(dest="use_film", action="store_true")),
    ("--model_for_cond", dict(type=str, default="")),
    ("--upsampling_ratios", dict(nargs="+", type=int, default=[5, 4, 2])),
    ("--cond_enc_ratios", dict(nargs="+", type=int, default=[8, 5, 4, 2])),
    ("--cond_bandwidth", dict(type=float, default=3.0)),
    ("--cond_global", dict(type=float, default=3.0)),
    ("--unet_scale_cond", dict(dest="unet_scale_cond", action="store_true")),
    ("--unet_scale_x", dict(dest="unet_scale_x", action="store_true")),
    ("--input_dir", dict(type=str, default="")),
    ("--output_dir", dict(type=str, default="outputs/")),
]
# additions of this implementation
_EXTRA: List[Tuple[str, dict]] = [
    ("--midway_t", dict(type=int, default=100, help="reverse-diffusion steps (literal 100 in the reference)")),
    ("--dtype", dict(type=str, default="bf16", choices=["bf16", "f32", "fp8"], help="UNet compute dtype on the GPU (fp8: e4m3 conv weights, bf16 math)")),
    ("--batch_size", dict(type=int, default=32, help="utterances decoded per engine call")),
    ("--seed", dict(type=int, default=0, help="seed of the device noise stream (rank r uses seed + r)")),
    ("--in_flight", dict(type=int, default=2, help="engine calls kept in flight when a run has several batches: n engines on n "
                                                    "streams, batches dealt round-robin, every batch decoded as one chain "
                                                    "(+19 %% throughput at 32 x 2.4 s on MI355X); 1 = one batch at a time")),
    ("--chunk_sec", dict(type=float, default=0.0, help="long-form mode (BASELINE config 5): mono recordings longer than this are "
                                                        "decoded as chunks of this length batched together, the chunks' raw decoder "
                                                        "outputs are joined and normalised over the whole recording; 0 = whole files")),
    # (both absent from the namespace unless given -- argparse.SUPPRESS -- so a run without them carries exactly the arguments it carried
    # before they existed; ragged_options() reads them with their defaults: off, 0.25)
    ("--ragged", dict(dest="ragged", action="store_true", default=argparse.SUPPRESS,
                      help="batch mono files of DIFFERENT lengths (Engine.decode_ragged: every file decoded as if alone); files are "
                           "trimmed to the chunk quantum (2560 samples for --enc_ratios 8 4, coarser than the reference's 640)")),
    ("--ragged_waste", dict(type=float, default=argparse.SUPPRESS, help="--ragged: a batch is closed before its padded size B * Tmax "
                                                                        "exceeds (1 + this) x the samples it really holds (default 0.25)")),
    ("--chunk_overlap_sec", dict(type=float, default=argparse.SUPPRESS,
                                 help="--chunk_sec > 0: decode a long mono recording on COUPLED windows of --chunk_sec that overlap by this "
                                      "much (Engine.decode_windows: one shared latent, the windows' predictions are cross-faded at every "
                                      "step, so there are no seams) instead of as independent chunks; at most half of --chunk_sec, 0 allowed")),
    ("--window_group", dict(dest="window_group", action="store_true", default=argparse.SUPPRESS,
                            help="--chunk_overlap_sec: decode SEVERAL long mono recordings per call (Engine.decode_windows_group): their "
                                 "windows, at most 32 in all, share one batch; recording i of the run is seeded (--seed + i) mod 2^64, so its "
                                 "audio depends neither on the grouping nor on the number of ranks")),
    ("--item_seeds", dict(dest="item_seeds", action="store_true", default=argparse.SUPPRESS,
                          help="seed every mono file on its own (Engine.decode_seeded): file i of the run is seeded (--seed + i) mod 2^64 and "
                               "draws as if decoded alone, so its audio depends neither on --batch_size, --ragged packing, --in_flight nor "
                               "the number of ranks; not with --chunk_sec > 0, not on multi-channel files")),
]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Encodec_baseline")
    for flag, kw in _FLAGS + _EXTRA:
        p.add_argument(flag, **kw)
    return p


def ragged_options(a) -> Tuple[bool, float]:
    """(--ragged, --ragged_waste) of a parsed namespace, with their defaults: off, 0.25."""
    return bool(getattr(a, "ragged", False)), float(getattr(a, "ragged_waste", 0.25))


def windows_options(a):
    """--chunk_overlap_sec of a parsed namespace: None without the flag, else the overlap in seconds (it needs --chunk_sec > 0 and is
    at most half of it)."""
    if not hasattr(a, "chunk_overlap_sec"):
        return None
    ov, chunk_sec = float(a.chunk_overlap_sec), float(getattr(a, "chunk_sec", 0.0) or 0.0)
    if chunk_sec <= 0:
        raise SystemExit("--chunk_overlap_sec needs --chunk_sec > 0 (the window length)")
    if not 0.0 <= ov <= chunk_sec / 2:
        raise SystemExit(f"--chunk_overlap_sec {ov}: must be in [0, --chunk_sec / 2 = {chunk_sec / 2}]")
    return ov


def window_group_option(a) -> bool:
    """--window_group of a parsed namespace (off without the flag); it needs --chunk_overlap_sec."""
    if not getattr(a, "window_group", False):
        return False
    if not hasattr(a, "chunk_overlap_sec"):
        raise SystemExit("--window_group needs --chunk_overlap_sec (it groups the recordings that are decoded on coupled windows)")
    return True


def item_seeds_option(a) -> bool:
    """--item_seeds of a parsed namespace (off without the flag); refused with --chunk_sec > 0: independent chunks have no single item
    length, and coupled windows have their own seeds (--window_group)."""
    if not getattr(a, "item_seeds", False):
        return False
    if float(getattr(a, "chunk_sec", 0.0) or 0.0) > 0:
        raise SystemExit("--item_seeds is not available with --chunk_sec > 0 (independent chunks have no single item length; coupled "
                         "windows are seeded per recording by --window_group)")
    return True


def item_seeds_for(seed: int, run_index: List[int]) -> List[int]:
    """--item_seeds: the seeds of a batch whose items are files run_index[k] of the run's file list: (seed + index) mod 2^64."""
    return [(int(seed) + int(i)) % (1 << 64) for i in run_index]


def _unsupported(a) -> None:
    bad = [n for n in ("train_time_diff", "self_condition", "qtz_condition", "use_film", "run_vae") if getattr(a, n)]
    if bad:
        raise SystemExit(f"flags {bad} select paths outside the decode path this implementation covers (SURVEY.md section 8)")
    if a.model_type != "unet":
        raise SystemExit("only --model_type unet is supported")
    if not a.model_for_cond:
        raise SystemExit("--model_for_cond is required: halfway sampling starts from the quantised condition (sample.py:125-130)")
    from .lib import FINAL_ACTIVATIONS
    if a.final_activation not in FINAL_ACTIVATIONS:
        raise SystemExit(f"--final_activation {a.final_activation}: supported are {sorted(k for k in FINAL_ACTIVATIONS if k)}")


def read_wav(path: str):
    """torchaudio.load (sample.py:83): -> (float32 [channels, T] in [-1, 1), sample rate)."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    x = x[None, :] if x.ndim == 1 else x.T
    return np.ascontiguousarray(x), int(sr)


def read_wav_16k(path: str, eng=None) -> np.ndarray:
    """-> float32 [channels, T] at 16 kHz: torchaudio.load + torchaudio.functional.resample(wav, sr, 16000) of the reference
    (sample.py:83-84); the resampling runs on the GPU (ldc_resample, the same windowed-sinc filter bank)."""
    x, sr = read_wav(path)
    if sr != 16000:
        import torch
        if eng is None:
            raise RuntimeError(f"{path}: {sr} Hz input needs the engine's resampler")
        x = eng.resample(torch.from_numpy(x), sr, 16000).cpu().numpy()
    return x


def wav_header(path: str) -> Tuple[int, int, int]:
    """(channels, samples at 16 kHz, sample rate) from the RIFF header alone: the 'fmt ' and 'data' chunk headers are parsed
    directly, no sample is touched and every PCM / float container size works (scipy's memory-mapped read refuses the 3-byte
    samples of 24-bit files: one such file used to abort the whole run on every rank).  The length after resampling is what
    the resampler itself will produce (ldc_resample_out_len = torchaudio's ceil(16000 * T / sr)), so the batch plan and the
    data agree."""
    import struct
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        ch = sr = block = None
        n_bytes = None
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                break
            cid, size = hdr[:4], struct.unpack("<I", hdr[4:])[0]
            if cid == b"fmt ":
                fmt = f.read(size + (size & 1))
                if len(fmt) < 16:
                    raise ValueError(f"{path}: 'fmt ' chunk of {len(fmt)} bytes (16 needed)")
                tag, ch, sr, _, block, _ = struct.unpack("<HHIIHH", fmt[:16])
                if tag == 0xFFFE and len(fmt) >= 26:            # WAVE_FORMAT_EXTENSIBLE: the real tag opens the sub-format GUID
                    tag = struct.unpack("<H", fmt[24:26])[0]
                if tag not in (1, 3):                            # PCM / IEEE float: the only containers whose block count is a sample count
                    raise ValueError(f"{path}: WAVE format tag {tag:#x} is not PCM or IEEE float")
            elif cid == b"data":
                here = f.tell()
                f.seek(0, 2)
                n_bytes = min(size, f.tell() - here) if size not in (0, 0xFFFFFFFF) else f.tell() - here   # streamed files leave the size open
                break
            else:
                f.seek(size + (size & 1), 1)
    if not ch or not sr or not block or n_bytes is None:
        raise ValueError(f"{path}: no 'fmt ' / 'data' chunk")
    n = n_bytes // block
    return int(ch), resample_out_len(n, int(sr), 16000), int(sr)


def resample_out_len(n: int, sr_in: int, sr_out: int) -> int:
    """Samples torchaudio.functional.resample returns for n input samples: ceil(new * n / orig) on the gcd-reduced rates
    (the arithmetic of ldc_resample_out_len, restated in Python so that header planning needs no built library;
    tests/test_cli_and_parallel_cpu.py holds the two to each other)."""
    import math
    g = math.gcd(int(sr_in), int(sr_out))
    o, nw = int(sr_in) // g, int(sr_out) // g
    return int(-(-nw * int(n) // o))


class LazyWavs:
    """The run's recordings at 16 kHz, loaded (and resampled on the GPU) on first use: a rank touches only the files of its own
    shard (through round 2 every rank read and resampled the whole corpus before sharding it: world-times redundant I/O and
    O(corpus) host memory per rank).  `shapes[i]` = (channels, samples) from the header.

    The batch source of decode_files: `batch` / `chunk_batch` build what the sampler decodes (here a waveform tensor; the
    decompress CLI's source hands out code batches), `in_ext` is the input extension output_path replaces."""

    in_ext = ".wav"

    def __init__(self, files: List[str], eng):
        self.files, self.eng = files, eng
        self.shapes = [wav_header(f)[:2] for f in files]
        self._cache: Dict[int, np.ndarray] = {}

    def subset(self, idx: List[int]) -> "LazyWavs":
        out = LazyWavs.__new__(LazyWavs)
        out.files, out.eng = [self.files[i] for i in idx], self.eng
        out.shapes = [self.shapes[i] for i in idx]
        out._cache = {}
        return out

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i: int) -> np.ndarray:
        if i not in self._cache:
            w = read_wav_16k(self.files[i], self.eng if hasattr(self.eng, "resample") else None)
            if w.shape[-1] != self.shapes[i][1]:               # a resampler that rounds differently: trust the data
                self.shapes[i] = (w.shape[0], w.shape[-1])
            self._cache[i] = w
        return self._cache[i]

    def drop(self, i: int) -> None:
        self._cache.pop(i, None)

    def batch(self, idxs: List[int], joint: bool, n: int):
        """[channels, 1, n] of one file (joint, as sample.py:85) or [len(idxs), 1, n] of mono files."""
        import torch
        if joint:
            return torch.from_numpy(np.ascontiguousarray(self[idxs[0]][:, None, :n]))
        return torch.from_numpy(np.stack([self[i][0, :n] for i in idxs])[:, None, :])

    def padded_batch(self, idxs: List[int], lens: List[int]):
        """[len(idxs), 1, max(lens)]: the first lens[k] samples of mono file idxs[k], zero-padded on the right (a ragged batch)."""
        import torch
        out = np.zeros((len(idxs), 1, max(lens)), np.float32)
        for k, (i, n) in enumerate(zip(idxs, lens)):
            out[k, 0, :n] = self[i][0, :n]
        return torch.from_numpy(out)

    def chunk_batch(self, part: List[Tuple[int, int, int]], ln: int):
        """[len(part), 1, ln]: chunk (file, order, start) of mono recordings."""
        import torch
        return torch.from_numpy(np.stack([self[i][0, st:st + ln] for i, _, st in part])[:, None, :])

    def plan_ragged(self, rank: int, world: int, batch_size: int, waste: float, quantum: int) -> List[Tuple[List[int], bool, bool]]:
        """--ragged work list of one rank: [(file indices, joint, ragged)] -- plan_ragged_batches; its sub-quantum files are not ragged."""
        lengths, channels = [sh[1] for sh in self.shapes], [sh[0] for sh in self.shapes]
        return [(idxs, joint, not joint and lengths[idxs[0]] >= quantum)
                for idxs, joint in plan_ragged_batches(lengths, channels, rank, world, batch_size, waste, quantum)]

    def ragged_batch(self, idxs: List[int], quantum: int):
        """-> (RaggedBatch of the files trimmed to whole quanta, their lengths in samples)"""
        lens = [self.shapes[i][1] // quantum * quantum for i in idxs]
        return RaggedBatch(self.padded_batch(idxs, lens), lens), lens


def output_path(wav_file: str, input_dir: str, output_dir: str, in_ext: str = ".wav", out_ext: str = ".wav") -> str:
    """sample.py:75-81,136: save_path = output_dir + wav_file[len(input_dir):][:-4]; file = save_path + '.wav'.
    (in_ext / out_ext: the compress / decompress CLIs name their files the same way, .wav <-> .ecdc)"""
    local_path = wav_file[len(input_dir):][:-len(in_ext)]
    save_path = output_dir + local_path
    return os.path.join(output_dir, f"{save_path}{out_ext}")


class RaggedBatch:
    """Mono files of different lengths as one engine call: wav [B, 1, Tmax] right-padded with zeros, lengths[b] samples of item b
    (multiples of the chunk quantum).  `.to(device)` as a tensor batch (see CodesBatch); the samplers route it to
    Engine.decode_ragged, whose outputs are zero behind an item's length."""

    def __init__(self, wav, lengths):
        self.wav, self.lengths = wav, [int(n) for n in lengths]

    def to(self, device, non_blocking: bool = False):
        return RaggedBatch(self.wav.to(device, non_blocking=non_blocking), self.lengths)


class DdpmSampler:
    """The reference's decode: halfway sampling, `n_steps` ancestral steps (Engine.decode).  `draws`: noise tensors per call."""

    def __init__(self, n_steps: int):
        self.n_steps = self.draws = int(n_steps)

    def __call__(self, eng, batch, noise, per_item: bool, want_stages: bool = False, seeds=None):
        if seeds is not None:   # --item_seeds: every item draws as if alone (no tape, per-item normalisation)
            rag = isinstance(batch, RaggedBatch)
            return eng.decode_seeded(batch.wav if rag else batch, seeds, self.n_steps, lengths=batch.lengths if rag else None,
                                     want_stages=want_stages)
        if isinstance(batch, RaggedBatch):
            return eng.decode_ragged(batch.wav, batch.lengths, self.n_steps, noise=noise, want_stages=want_stages)
        if want_stages:
            return eng.decode(batch, self.n_steps, noise=noise, per_item=per_item, want_stages=True)
        return eng.decode(batch, self.n_steps, noise=noise, per_item=per_item)


class DdimSampler:
    """DDIM decode (Engine.decode_ddim): `n_steps` strided iterations from `t_start` with `eta`."""

    def __init__(self, t_start: int, n_steps: int, eta: float = 0.0):
        self.t_start, self.n_steps, self.eta = int(t_start), int(n_steps), float(eta)
        self.draws = self.n_steps

    def __call__(self, eng, batch, noise, per_item: bool, want_stages: bool = False, seeds=None):
        if seeds is not None:   # --item_seeds, as DdpmSampler's
            rag = isinstance(batch, RaggedBatch)
            return eng.decode_seeded(batch.wav if rag else batch, seeds, self.n_steps, lengths=batch.lengths if rag else None,
                                     sampler="ddim", t_start=self.t_start, eta=self.eta, want_stages=want_stages)
        if isinstance(batch, RaggedBatch):
            return eng.decode_ragged(batch.wav, batch.lengths, self.n_steps, t_start=self.t_start, eta=self.eta, noise=noise,
                                     want_stages=want_stages)
        return eng.decode_ddim(batch, self.t_start, self.n_steps, self.eta, noise=noise, per_item=per_item, want_stages=want_stages)


class DpmSampler:
    """DPM-Solver++(2M) decode (Engine.decode_dpm): `n_steps` second-order multistep iterations from `t_start` on DDIM's timestep
    list.  Deterministic: `draws` is 0, so no noise provider is asked for a tape and none is passed on."""

    draws = 0

    def __init__(self, t_start: int, n_steps: int):
        self.t_start, self.n_steps = int(t_start), int(n_steps)

    def __call__(self, eng, batch, noise, per_item: bool, want_stages: bool = False, seeds=None):
        if seeds is not None:
            raise SystemExit("--item_seeds: DPM-Solver++ draws nothing, there is nothing to seed; drop the flag")
        if isinstance(batch, RaggedBatch):
            return eng.decode_ragged_dpm(batch.wav, batch.lengths, self.t_start, self.n_steps, want_stages=want_stages)
        return eng.decode_dpm(batch, self.t_start, self.n_steps, per_item=per_item, want_stages=want_stages)


class CodesBatch:
    """A batch of RVQ codes for CodesSampler: packed [B, >= packed bytes] uint8 (the container payload rows, `bits` per code) or
    codes [n_q, B, F] int64.  `.to(device)` as a tensor batch, so decode_with_retry and the in-flight retire path take it as is."""

    def __init__(self, packed=None, codes=None, n_q: int = 0, F: int = 0, bits: int = 10):
        self.packed, self.codes, self.bits = packed, codes, int(bits)
        self.n_q = int(codes.shape[0]) if codes is not None else int(n_q)
        self.F = int(codes.shape[2]) if codes is not None else int(F)

    def to(self, device, non_blocking: bool = False):
        mv = lambda t: t.to(device, non_blocking=non_blocking) if t is not None else None
        return CodesBatch(mv(self.packed), mv(self.codes), self.n_q, self.F, self.bits)


class RaggedCodesBatch:
    """Containers of different lengths as one engine call: packed [B, stride] uint8, row b = item b's own payload (zeros behind it),
    frames[b] condition frames of item b (multiples of chunk_quantum // 320).  CodesSampler routes it to Engine.decode_codes_ragged."""

    def __init__(self, packed, n_q: int, frames, bits: int = 10):
        self.packed, self.n_q, self.frames, self.bits = packed, int(n_q), [int(f) for f in frames], int(bits)

    def to(self, device, non_blocking: bool = False):
        return RaggedCodesBatch(self.packed.to(device, non_blocking=non_blocking), self.n_q, self.frames, self.bits)


class CodesSampler:
    """The decode of `inner` (DdpmSampler / DdimSampler / DpmSampler) started from a CodesBatch: Engine.decode_codes /
    decode_codes_ddim / decode_codes_dpm; from a RaggedCodesBatch: Engine.decode_codes_ragged (DDPM and DDIM only)."""

    def __init__(self, inner):
        self.inner = inner
        self.n_steps = self.draws = inner.draws

    def __call__(self, eng, batch, noise, per_item: bool, want_stages: bool = False, seeds=None):
        dpm = isinstance(self.inner, DpmSampler)
        if seeds is not None:   # --item_seeds: Engine.decode_codes_seeded, DDPM and DDIM only
            if dpm:
                raise SystemExit("--item_seeds: DPM-Solver++ draws nothing, there is nothing to seed; drop the flag")
            ddim = isinstance(self.inner, DdimSampler)
            rag = isinstance(batch, RaggedCodesBatch)
            return eng.decode_codes_seeded(seeds, codes=None if rag else batch.codes, packed=batch.packed, lengths=batch.frames if rag else None,
                                           bits=batch.bits, n_q=batch.n_q, F=None if rag else batch.F, n_steps=self.inner.n_steps,
                                           sampler="ddim" if ddim else "ddpm", t_start=self.inner.t_start if ddim else 0,
                                           eta=self.inner.eta if ddim else 0.0, want_stages=want_stages)
        if isinstance(batch, RaggedCodesBatch):
            if dpm:
                raise ValueError("DPM-Solver++ sampling has no ragged decode from codes (Engine.decode_codes_ragged takes DDPM and DDIM "
                                 "only): decode the containers in equal-length batches, without --ragged")
            ddim = isinstance(self.inner, DdimSampler)
            return eng.decode_codes_ragged(packed=batch.packed, frames=batch.frames, bits=batch.bits, n_q=batch.n_q,
                                           n_steps=self.inner.n_steps, t_start=self.inner.t_start if ddim else 0,
                                           eta=self.inner.eta if ddim else 0.0, noise=noise, want_stages=want_stages)
        kw = dict(codes=batch.codes, packed=batch.packed, bits=batch.bits, n_q=batch.n_q, F=batch.F, noise=noise, per_item=per_item,
                  want_stages=want_stages)
        if dpm:
            del kw["noise"]
            return eng.decode_codes_dpm(t_start=self.inner.t_start, n_steps=self.inner.n_steps, **kw)
        if isinstance(self.inner, DdimSampler):
            return eng.decode_codes_ddim(t_start=self.inner.t_start, n_steps=self.inner.n_steps, eta=self.inner.eta, **kw)
        return eng.decode_codes(n_steps=self.inner.n_steps, **kw)


def _sampler_of(n_steps: int, sampler):
    return sampler if sampler is not None else DdpmSampler(n_steps)


def _sampler(inp_args, sampler):
    return sampler if sampler is not None else DdpmSampler(inp_args.midway_t)


def synthesis(inp_args, sampler=None) -> List[str]:
    """`sampler`: DdpmSampler (default, --midway_t steps), DdimSampler or DpmSampler."""
    from . import parallel

    _unsupported(inp_args)
    rank, local_rank, world = parallel.init_process_group("nccl")
    files = sorted(glob.glob(os.path.join(inp_args.input_dir, "**/*.wav"), recursive=True))
    engines = build_engines(inp_args, files, rank, world, local_rank)
    written = decode_files(engines if len(engines) > 1 else engines[0], files, inp_args, rank, world, local_rank, sampler=sampler)
    for eng in engines:
        eng.close()
    return written


def build_engines(inp_args, files: List[str], rank: int, world: int, local_rank: int):
    """The run's engines (both models loaded from --model_path / --model_for_cond): --in_flight of them when the rank has several
    batches, else one."""
    from . import checkpoint, lib as L
    from .model import Engine
    from .spec import CodecConfig, UnetConfig

    main_codec = CodecConfig(rep_dims=inp_args.rep_dims, n_filters=inp_args.n_filters,
                             n_residual_layers=inp_args.n_residual_layers, lstm=inp_args.lstm,
                             enc_ratios=tuple(inp_args.enc_ratios), quantization=False,
                             final_activation=inp_args.final_activation)
    cond_codec = CodecConfig(rep_dims=inp_args.rep_dims, n_filters=inp_args.n_filters,
                             n_residual_layers=inp_args.n_residual_layers, lstm=inp_args.lstm,
                             enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=inp_args.cond_bandwidth,
                             final_activation=inp_args.final_activation)   # quirk Q1: ratios are always [8,5,4,2]
    unet = UnetConfig(dim=inp_args.diff_dims, inp_channels=inp_args.rep_dims, upsampling_ratios=tuple(inp_args.upsampling_ratios),
                      unet_scale_cond=inp_args.unet_scale_cond, unet_scale_x=inp_args.unet_scale_x)
    n_eng = max(1, int(getattr(inp_args, "in_flight", 1)))
    if len(files) <= inp_args.batch_size * world:        # a single batch per rank: nothing to pipeline
        n_eng = 1
    sd_main, sd_cond = checkpoint.read_amlt(inp_args.model_path), checkpoint.read_amlt(inp_args.model_for_cond)
    engines = []
    for k in range(n_eng):
        eng = Engine(main_codec, unet, cond_codec, dtype=inp_args.dtype, device=local_rank, noise_seed=inp_args.seed + rank + 7919 * k)
        if n_eng > 1:
            eng.set_option("split", 1)                   # with batches in flight each batch is one chain (a per-context option,
        eng.load_state_dict(L.MODEL_MAIN, sd_main)       # not an environment variable: other engines of the process keep theirs)
        eng.load_state_dict(L.MODEL_COND, sd_cond)       # load_model(model, path, strict=True)
        eng.finalize(strict=True)
        engines.append(eng)
    return engines


def apply_device_fallback(eng, err) -> bool:
    """A kernel whose bounded in-launch wait gave up poisons its output with NaN and raises the context's device-side failure
    flag; the call that sees the flag fails with LDC_E_HIP and a tagged message (ldc_api.cpp: check_dev_flag).  Switch the engine
    to the form that needs no co-residency: "[coop_lstm]" -> the streamed LSTM kernel, "[gn_wait]" -> separate conv + gn_apply
    launches.  "[ctx_range]" is raised the same way by the LinearAttention context fold when a k is outside the range its unshifted
    exponentials are valid for -> fold_ctx 0 (column maximum + context launch).  Returns False for any other error."""
    from . import lib as L
    if getattr(err, "code", None) != L.E_HIP or "device-side failure" not in str(err):
        return False
    if "[gn_wait]" in str(err):
        eng.set_option("fuse_gn_epi", 0)
    elif "[ctx_range]" in str(err):
        eng.set_option("fold_ctx", 0)
    else:
        eng.set_option("lstm_stream", 1)
    return True


def decode_with_retry(eng, batch, n_steps: int, noise, per_item: bool, sampler=None, seeds=None):
    """One engine call; a batch hit by a device-side failure (or by the report of an earlier call's) is decoded again after
    the matching fallback (apply_device_fallback), twice at most: the LSTM and the GroupNorm exchange can each give up once.
    `sampler` (optional) replaces the DDPM decode of n_steps; `seeds` (--item_seeds): one seed per item, through the sampler."""
    from . import lib as L
    for attempt in range(3):
        try:
            if seeds is not None:
                return _sampler_of(n_steps, sampler)(eng, batch, None, per_item, seeds=seeds)
            if sampler is not None:
                return sampler(eng, batch, noise, per_item)
            return eng.decode(batch, n_steps, noise=noise, per_item=per_item)
        except L.LdcError as e:
            if attempt == 2 or not apply_device_fallback(eng, e):
                raise


def plan_batches(lengths: List[int], channels: List[int], rank: int, world: int, batch_size: int) -> List[Tuple[List[int], bool]]:
    """Work list of one rank: [(file indices, joint)].  Files are dealt to ranks whole (parallel.shard_utterances over
    FILES), so a file has one writer.  Mono files of equal trimmed length share batches (`joint` False: per-utterance
    normalisation = the reference's result for a mono file); a multi-channel file is its own batch, normalised jointly
    over its channels as sample.py:129,133-134 do."""
    from . import parallel
    mine = parallel.shard_utterances(lengths, rank, world)
    work: List[Tuple[List[int], bool]] = []
    by_len: Dict[int, List[int]] = {}
    for i in mine:
        if channels[i] > 1:
            work.append(([i], True))
        else:
            by_len.setdefault(lengths[i] // 640 * 640, []).append(i)
    for _, idxs in sorted(by_len.items(), reverse=True):
        for s in range(0, len(idxs), batch_size):
            work.append((idxs[s:s + batch_size], False))
    return work


def plan_ragged_batches(lengths: List[int], channels: List[int], rank: int, world: int, batch_size: int, waste: float,
                        quantum: int) -> List[Tuple[List[int], bool]]:
    """plan_batches for --ragged: the rank's mono files, trimmed to whole quanta and sorted by that length (longest first), are packed
    greedily into batches of at most batch_size files; a batch is closed before its padded size B * Tmax would exceed (1 + waste) x
    the samples it holds.  Multi-channel files keep their joint single-file batches; mono files shorter than one quantum (nothing of
    them survives the trim) keep plan_batches' equal-length batches and the reference's 640-sample trim."""
    from . import parallel
    mine = parallel.shard_utterances(lengths, rank, world)
    work: List[Tuple[List[int], bool]] = []
    short: Dict[int, List[int]] = {}
    mono: List[Tuple[int, int]] = []
    for i in mine:
        if channels[i] > 1:
            work.append(([i], True))
        elif lengths[i] // quantum == 0:
            short.setdefault(lengths[i] // 640 * 640, []).append(i)
        else:
            mono.append((lengths[i] // quantum * quantum, i))
    mono.sort(key=lambda t: (-t[0], t[1]))
    cur: List[int] = []
    tmax = held = 0
    for n, i in mono:
        if cur and (len(cur) == batch_size or (len(cur) + 1) * tmax > (1.0 + waste) * (held + n)):
            work.append((cur, False))
            cur = []
        if not cur:
            tmax = held = 0
        cur.append(i)
        tmax = max(tmax, n)
        held += n
    if cur:
        work.append((cur, False))
    for _, idxs in sorted(short.items(), reverse=True):
        for s in range(0, len(idxs), batch_size):
            work.append((idxs[s:s + batch_size], False))
    return work


_CHUNK_QUANTUM = 2560     # default quantum (enc_ratios 8 4): see chunk_quantum


def chunk_quantum(enc_ratios, unet_levels: int = 5) -> int:
    """Samples a chunk must be a multiple of: whole condition frames (320 samples, cond codec hop 8*5*4*2) AND a latent length that
    survives the UNet's unet_levels - 1 halvings (unet.py:336-349): lcm(320, hop * 2^(levels-1)) -- 2560 for enc_ratios 8 4 (hop
    32), 640 for enc_ratios 8.  (Through round 2 this was a fixed 1280, which let a 1.2 s tail -- the tail of a 30 s recording cut
    into 2.4 s chunks -- reach the UNet with L = 600.)"""
    import math
    hop = int(np.prod(list(enc_ratios)))
    return math.lcm(320, hop * (1 << (unet_levels - 1)))


def plan_chunks(n_samples: int, chunk: int, quantum: int = _CHUNK_QUANTUM) -> List[Tuple[int, int]]:
    """[(start, length)] of a recording cut into `chunk`-sample pieces; the tail keeps whole quanta (a shorter last chunk),
    what is left of it (less than one quantum) is dropped as the reference drops the sub-frame tail (sample.py:87-88)."""
    out, pos = [], 0
    while n_samples - pos >= chunk:
        out.append((pos, chunk)); pos += chunk
    tail = (n_samples - pos) // quantum * quantum
    if tail > 0:
        out.append((pos, tail))
    return out


def decode_long_files(eng, files: List[str], wavs, inp_args, rank: int, world: int, local_rank: int, sampler=None) -> List[str]:
    """Long-form mode: every chunk of every recording of this rank is one batch item (equal-length chunks share engine calls
    across recordings); the chunks' latents go through the decoder, the raw waveforms are joined per recording and the
    reference's output normalisation (sample.py:133-134) runs once over the whole recording."""
    import torch
    from scipy.io import wavfile
    from . import lib as L, parallel
    sampler = _sampler(inp_args, sampler)
    quantum = chunk_quantum(getattr(inp_args, "enc_ratios", [8, 4]))
    chunk = max(quantum, int(round(inp_args.chunk_sec * 16000)) // quantum * quantum)
    mine = parallel.shard_utterances([sh[1] for sh in wavs.shapes], rank, world)
    pieces: Dict[int, List[Tuple[int, int, int]]] = {}            # chunk length -> [(file, order, start)]
    nchunks = {}
    for i in mine:
        plan = plan_chunks(wavs.shapes[i][1], chunk, quantum)
        nchunks[i] = len(plan)
        for k, (st, ln) in enumerate(plan):
            pieces.setdefault(ln, []).append((i, k, st))
    dev = torch.device("cuda", local_rank)
    raw: Dict[int, List] = {i: [None] * nchunks[i] for i in mine}
    for ln, items in sorted(pieces.items(), reverse=True):
        for s in range(0, len(items), inp_args.batch_size):
            part = items[s:s + inp_args.batch_size]
            batch = wavs.chunk_batch(part, ln)
            # test seam (see decode_files): keys are (file index, chunk number)
            provider = getattr(inp_args, "noise_provider", None)
            hop = int(np.prod(getattr(inp_args, "enc_ratios", [8])))
            # (a sampler that draws nothing -- DpmSampler -- never asks for a tape)
            noise = provider([(i, k) for i, k, _ in part], sampler.draws, ln // hop).to(dev) if provider is not None and sampler.draws > 0 else None
            stages = sampler(eng, batch.to(dev), noise, True, want_stages=True)
            wav_raw = eng.decode_latents(L.MODEL_MAIN, stages["latents"])          # un-normalised decoder output
            for j, (i, k, _) in enumerate(part):
                raw[i][k] = wav_raw[j:j + 1]
    written = []
    for i in mine:
        if not raw[i]:
            continue
        whole = eng.output_normalise(torch.cat(raw[i], dim=-1), per_item=False)
        if not bool(torch.isfinite(whole).all()):
            raise RuntimeError(f"non-finite audio decoded for {files[i]}")
        path = output_path(files[i], inp_args.input_dir, inp_args.output_dir, wavs.in_ext)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        wavfile.write(path, 16000, np.ascontiguousarray(whole.cpu().numpy()[0, 0]))
        written.append(path)
    return written


MAX_WINDOWS = 32          # windows of one Engine.decode_windows call (ldc_window_layout)


def window_grid(chunk_sec: float, overlap_sec: float, enc_ratios, upsampling_ratios) -> Tuple[int, int]:
    """(Lw, overlap) in latent frames for --chunk_sec / --chunk_overlap_sec: the window on the chunk quantum (as --chunk_sec cuts its
    chunks), the overlap rounded down to whole condition frames (multiples of prod(upsampling_ratios)) and to at most Lw / 2."""
    quantum, hop = chunk_quantum(enc_ratios), int(np.prod(list(enc_ratios)))
    up = int(np.prod(list(upsampling_ratios)))
    Lw = max(quantum, int(round(chunk_sec * 16000)) // quantum * quantum) // hop
    ov = min(int(round(overlap_sec * 16000)) // hop, Lw // 2) // up * up
    return Lw, ov


def plan_window_segments(Ltot: int, Lw: int, overlap: int, up: int, max_windows: int = MAX_WINDOWS) -> List[Tuple[int, int]]:
    """[(first frame, frames)] of a recording of Ltot latent frames cut into segments of at most max_windows coupled windows each
    (Lw + (max_windows - 1)(Lw - overlap) frames).  A last segment shorter than one window takes the frames it lacks from its
    predecessor (whole condition frames), so every segment holds at least Lw frames."""
    seg = Lw + (max_windows - 1) * (Lw - overlap)
    if Ltot <= seg:
        return [(0, Ltot)]
    cuts = list(range(0, Ltot, seg))
    if Ltot - cuts[-1] < Lw:
        cuts[-1] -= -(-(Lw - (Ltot - cuts[-1])) // up) * up
    return [(a, b - a) for a, b in zip(cuts, cuts[1:] + [Ltot])]


def window_decoder(eng, sampler, Lw: int, ov: int):
    """The coupled-windows call of `sampler` on `eng` as (piece, noise, want_stages) -> result.  DdpmSampler / DdimSampler / DpmSampler:
    piece is the waveform [1, 1, T] (Engine.decode_windows / decode_ddim_windows / decode_dpm_windows); a CodesSampler around one of
    them: piece is the codes [n_q, 1, F] (Engine.decode_codes_windows / decode_codes_dpm_windows).  A DPM route is never handed noise."""
    from_codes = isinstance(sampler, CodesSampler)
    inner = sampler.inner if from_codes else sampler
    if not isinstance(inner, (DdpmSampler, DdimSampler, DpmSampler)):
        raise SystemExit("--chunk_overlap_sec: coupled windows decode with DDPM, DDIM or DPM-Solver++ sampling only")
    ddim = isinstance(inner, DdimSampler)

    def one(wav, noise, stages):
        if isinstance(inner, DpmSampler):
            return eng.decode_dpm_windows(wav, inner.t_start, inner.n_steps, Lw, ov, want_stages=stages)
        if ddim:
            return eng.decode_ddim_windows(wav, inner.t_start, inner.n_steps, Lw, ov, eta=inner.eta, noise=noise, want_stages=stages)
        return eng.decode_windows(wav, inner.n_steps, Lw, ov, noise=noise, want_stages=stages)

    def one_codes(codes, noise, stages):
        if isinstance(inner, DpmSampler):
            return eng.decode_codes_dpm_windows(codes=codes, t_start=inner.t_start, n_steps=inner.n_steps, Lw=Lw, overlap=ov, want_stages=stages)
        return eng.decode_codes_windows(codes=codes, n_steps=inner.n_steps, Lw=Lw, overlap=ov, t_start=inner.t_start if ddim else 0,
                                        eta=inner.eta if ddim else 0.0, noise=noise, want_stages=stages)

    return one_codes if from_codes else one


def plan_window_groups(windows: List[int], max_windows: int = MAX_WINDOWS) -> List[List[int]]:
    """--window_group: recordings of windows[k] windows each packed into groups of at most max_windows windows in all -- in order, first
    fit; -> the groups as lists of positions (ascending inside a group).  Every group is one Engine.decode_windows_group call."""
    groups, room = [], []
    for k, w in enumerate(windows):
        if not 1 <= w <= max_windows:
            raise ValueError(f"recording {k}: {w} windows do not fit a group of {max_windows}")
        g = next((j for j, r in enumerate(room) if w <= r), None)
        if g is None:
            groups.append([])
            room.append(max_windows)
            g = len(groups) - 1
        groups[g].append(k)
        room[g] -= w
    return groups


def decode_window_group(eng, wavs_dev, sampler, Lw: int, ov: int, noise=None, seeds=None):
    """One Engine.decode_windows_group call of `sampler` (DdpmSampler / DdimSampler / DpmSampler) -> the list of waveforms."""
    if isinstance(sampler, DpmSampler):
        return eng.decode_windows_group(wavs_dev, sampler.n_steps, Lw, ov, sampler="dpm", t_start=sampler.t_start)
    if isinstance(sampler, DdimSampler):
        return eng.decode_windows_group(wavs_dev, sampler.n_steps, Lw, ov, sampler="ddim", t_start=sampler.t_start, eta=sampler.eta,
                                        noise=noise, seeds=seeds)
    return eng.decode_windows_group(wavs_dev, sampler.n_steps, Lw, ov, noise=noise, seeds=seeds)


def decode_window_files(eng, files: List[str], wavs, inp_args, overlap_sec: float, rank: int, world: int, local_rank: int, sampler=None,
                        run_index: Optional[List[int]] = None) -> List[str]:
    """--chunk_overlap_sec: every long mono recording of this rank through Engine.decode_windows / decode_ddim_windows /
    decode_dpm_windows, trimmed to whole 640-sample frames as the whole-file path trims.  With a CodesSampler (decompress) `wavs` is a
    container source and the recording's codes go through Engine.decode_codes_windows / decode_codes_dpm_windows instead.  A recording
    that needs more than MAX_WINDOWS windows is cut into segments (of the waveform, or of the codes: cuts fall at whole condition
    frames) that are decoded one after another and hard-joined (raw decoder outputs, normalised once over the recording).
    --window_group (waveforms only): the rank's recordings that fit one call are packed into groups of at most MAX_WINDOWS windows
    (plan_window_groups: file order, first fit), every group one Engine.decode_windows_group call.  Without a noise provider recording i
    is seeded (--seed + run_index[i]) mod 2^64 -- run_index[i]: its index in the run's file list (default: i) --, so its audio depends
    neither on the grouping nor on the number of ranks; the provider is asked per recording as without the flag, key (i, 0)."""
    import sys
    import torch
    from scipy.io import wavfile
    from . import lib as L, parallel
    sampler = _sampler(inp_args, sampler)
    from_codes = isinstance(sampler, CodesSampler)
    enc_ratios = getattr(inp_args, "enc_ratios", [8, 4])
    hop, up = int(np.prod(list(enc_ratios))), int(np.prod(list(inp_args.upsampling_ratios)))
    Lw, ov = window_grid(float(inp_args.chunk_sec), overlap_sec, enc_ratios, inp_args.upsampling_ratios)
    dev = torch.device("cuda", local_rank)
    provider = getattr(inp_args, "noise_provider", None)
    one = window_decoder(eng, sampler, Lw, ov)   # (refuses a sampler without a windows route before anything is loaded)
    written = []
    mine = list(parallel.shard_utterances([sh[1] for sh in wavs.shapes], rank, world))
    grouped = set()
    if window_group_option(inp_args):
        if from_codes:
            raise SystemExit("--window_group: decoding from codes has no group call (Engine.decode_windows_group takes waveforms); drop the flag")

        def n_windows(i):   # 0: the recording keeps the route below (more than MAX_WINDOWS windows: segments)
            Ltot = wavs.shapes[i][1] // 640 * 640 // hop
            if Ltot < Lw or len(plan_window_segments(Ltot, Lw, ov, up)) > 1:
                return 0
            return 1 + -(-(Ltot - Lw) // (Lw - ov))
        cand = [i for i in mine if n_windows(i)]
        inner_draws = sampler.draws
        for g in plan_window_groups([n_windows(i) for i in cand]):
            idx = [cand[k] for k in g]
            ns = [wavs.shapes[i][1] // 640 * 640 for i in idx]
            xs = [torch.from_numpy(np.ascontiguousarray(wavs[i][:1, None, :n])).to(dev) for i, n in zip(idx, ns)]
            noise = seeds = None
            if inner_draws > 0 and provider is not None:   # test seam (see decode_files): asked per recording, key (file index, 0)
                noise = [provider([(i, 0)], inner_draws, n // hop).to(dev) for i, n in zip(idx, ns)]
            elif inner_draws > 0:
                seeds = [(int(inp_args.seed) + (run_index[i] if run_index is not None else i)) % (1 << 64) for i in idx]
            outs = decode_window_group(eng, xs, sampler, Lw, ov, noise=noise, seeds=seeds)
            for i, whole in zip(idx, outs):
                if not bool(torch.isfinite(whole).all()):
                    raise RuntimeError(f"non-finite audio decoded for {files[i]}")
                path = output_path(files[i], inp_args.input_dir, inp_args.output_dir, wavs.in_ext)
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                wavfile.write(path, 16000, np.ascontiguousarray(whole.cpu().numpy()[0, 0]))
                written.append(path)
                wavs.drop(i)
        grouped = set(cand)
    for i in mine:
        if i in grouped:
            continue
        n = wavs.shapes[i][1] // 640 * 640
        x = None if from_codes else torch.from_numpy(np.ascontiguousarray(wavs[i][:1, None, :n]))
        segs = plan_window_segments(n // hop, Lw, ov, up)
        if len(segs) > 1:
            print(f"[windows] {files[i]}: {n // hop} latent frames need more than {MAX_WINDOWS} windows; decoded as {len(segs)} "
                  f"segments, hard-joined", file=sys.stderr)
        raw = []
        for k, (f0, fl) in enumerate(segs):
            # test seam (see decode_files): keys are (file index, segment number)
            noise = provider([(i, k)], sampler.draws, fl).to(dev) if provider is not None and sampler.draws > 0 else None
            if from_codes:   # the segment's codes [n_q, 1, fl / up] (a cut at latent frame f0 is condition frame f0 / up)
                piece = wavs.chunk_batch([(i, k, f0 * hop)], fl * hop).codes
            else:
                piece = x[:, :, f0 * hop:(f0 + fl) * hop].contiguous()
            got = one(piece.to(dev), noise, len(segs) > 1)
            raw.append(got if len(segs) == 1 else eng.decode_latents(L.MODEL_MAIN, got["latents"]))
        whole = raw[0] if len(segs) == 1 else eng.output_normalise(torch.cat(raw, dim=-1), per_item=False)
        if not bool(torch.isfinite(whole).all()):
            raise RuntimeError(f"non-finite audio decoded for {files[i]}")
        path = output_path(files[i], inp_args.input_dir, inp_args.output_dir, wavs.in_ext)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        wavfile.write(path, 16000, np.ascontiguousarray(whole.cpu().numpy()[0, 0]))
        written.append(path)
        if not from_codes:
            wavs.drop(i)
    return written


def decode_files(eng, files: List[str], inp_args, rank: int, world: int, local_rank: int, sampler=None, source=None,
                 run_index: Optional[List[int]] = None) -> List[str]:
    """`eng`: one engine, or a list of engines (one batch in flight per engine, each on its own stream); `sampler`: as synthesis;
    `source`: the batch source over `files` (default LazyWavs; see there).
    --item_seeds: file i draws under (--seed + run_index[i]) mod 2^64 -- run_index[i]: its index in the run's file list (default: i) --
    as if decoded alone (item_seeds_for; Engine.decode_seeded / decode_codes_seeded through the sampler), whatever batch, engine or rank
    it lands on; a noise provider is not asked."""
    import torch
    from scipy.io import wavfile
    engines = list(eng) if isinstance(eng, (list, tuple)) else [eng]
    eng = engines[0]
    sampler = _sampler(inp_args, sampler)
    steps = sampler.draws
    wavs = source if source is not None else LazyWavs(files, eng)   # headers only: (channels, samples at 16 kHz); data is loaded per shard
    keep = [i for i, sh in enumerate(wavs.shapes) if sh[1] // 640 * 640 > 0]                  # sample.py:87-88
    files, wavs = [files[i] for i in keep], wavs.subset(keep)
    item_seeds = item_seeds_option(inp_args)   # (refused with --chunk_sec > 0 before anything is decoded)
    if item_seeds:
        multi = [f for f, sh in zip(files, wavs.shapes) if sh[0] > 1]
        if multi:
            raise SystemExit(f"--item_seeds: {multi[0]} has more than one channel (a multi-channel file keeps the joint normalisation "
                             f"over its channels, so its channels are not items that decode as if alone)")
        run_of = [run_index[i] if run_index is not None else i for i in keep]
    chunk_sec = float(getattr(inp_args, "chunk_sec", 0.0) or 0.0)
    overlap_sec = windows_options(inp_args)
    window_group_option(inp_args)   # (--window_group without --chunk_overlap_sec is refused before anything is decoded)
    if overlap_sec is not None and source is not None and not isinstance(sampler, CodesSampler):
        raise SystemExit("--chunk_overlap_sec: a batch source other than waveforms needs a CodesSampler (decompress)")
    if chunk_sec > 0:
        # recordings longer than a chunk (mono) take the long-form path, everything else the reference's whole-file path
        is_long = [sh[0] == 1 and sh[1] > int(round(chunk_sec * 16000)) for sh in wavs.shapes]
        long_i = [i for i, m in enumerate(is_long) if m]
        short_i = [i for i, m in enumerate(is_long) if not m]
        long_f, long_w = [files[i] for i in long_i], wavs.subset(long_i)
        files, wavs = [files[i] for i in short_i], wavs.subset(short_i)
        if overlap_sec is not None:
            written_long = decode_window_files(eng, long_f, long_w, inp_args, overlap_sec, rank, world, local_rank, sampler=sampler,
                                               run_index=[keep[i] for i in long_i]) if long_f else []
        else:
            written_long = decode_long_files(eng, long_f, long_w, inp_args, rank, world, local_rank, sampler=sampler) if long_f else []
    else:
        written_long = []
    lengths = [sh[1] for sh in wavs.shapes]
    channels = [sh[0] for sh in wavs.shapes]
    written = []
    dev = torch.device("cuda", local_rank)
    streams = [torch.cuda.Stream(device=dev) for _ in engines] if len(engines) > 1 else [None]
    pending: List[tuple] = []                 # (output tensor on the device, file indices, joint, stream, redo, lengths | None), oldest first
    ragged, ragged_waste = ragged_options(inp_args)
    quantum = chunk_quantum(getattr(inp_args, "enc_ratios", [8, 4]))
    hop = int(np.prod(getattr(inp_args, "enc_ratios", [8])))   # samples per latent frame of the main codec (noise seam only)

    def retire(item):
        out, idxs, joint, stream, redo, lens = item
        if stream is not None:
            stream.synchronize()               # the producer stream, not the current one: waits for that engine's batch only
        out = out.cpu()
        if not bool(torch.isfinite(out).all()):
            # the device-side failure of this batch (cooperative LSTM timed out: its output is poisoned with NaN) is reported by
            # the engine's NEXT call; decode the batch again on the streamed LSTM instead of losing the run
            # (that report -- LDC_E_HIP with the failure's tag -- may well arrive in the redo itself: decode_with_retry applies the
            # matching fallback and decodes again; without a report the cooperative LSTM is the one that poisons silently)
            eng_k, batch_k, per_item_k, noise_k = redo[:4]
            kw_k = dict(seeds=redo[4]) if len(redo) > 4 else {}   # (--item_seeds: the same seeds, so the same audio)
            out = decode_with_retry(eng_k, batch_k.to(dev), steps, noise_k, per_item_k, sampler, **kw_k).cpu()
            if not bool(torch.isfinite(out).all()):
                eng_k.set_option("lstm_stream", 1)
                eng_k.set_option("fuse_gn_epi", 0)
                out = decode_with_retry(eng_k, batch_k.to(dev), steps, noise_k, per_item_k, sampler, **kw_k).cpu()
            if not bool(torch.isfinite(out).all()):
                raise RuntimeError(f"non-finite audio decoded for {[files[i] for i in idxs]}")
        out = out.numpy()
        for k, i in enumerate(idxs):
            path = output_path(files[i], inp_args.input_dir, inp_args.output_dir, wavs.in_ext)
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            data = out[:, 0, :].T if joint else out[k, 0]                                     # [T, channels] | [T]
            if lens is not None:
                data = data[:lens[k]]                                                          # ragged batch: the item's own samples
            wavfile.write(path, 16000, np.ascontiguousarray(data))
            written.append(path)

    if ragged:     # the source's own plan: (indices, joint, ragged) -- files it keeps out of ragged batches take the equal-length path
        work = wavs.plan_ragged(rank, world, inp_args.batch_size, ragged_waste, quantum)
    else:
        work = [(idxs, joint, False) for idxs, joint in plan_batches(lengths, channels, rank, world, inp_args.batch_size)]
    for j, (idxs, joint, is_ragged) in enumerate(work):
        lens = None
        if is_ragged:
            batch, lens = wavs.ragged_batch(idxs, quantum)
            n = max(lens)
        else:
            n = lengths[idxs[0]] // 640 * 640
            batch = wavs.batch(idxs, joint, n)
        slot = j % len(engines)
        if len(pending) >= len(engines):
            retire(pending.pop(0))             # the batch this engine decoded last: its output is read before the slot is reused
        # test seam: a callable (file indices, steps, latent length) -> noise [steps, B, 128, L] replaces the device-drawn noise
        provider = getattr(inp_args, "noise_provider", None)
        noise = provider(idxs, steps, n // hop).to(dev) if provider is not None and steps > 0 and not item_seeds else None
        kw = dict(seeds=item_seeds_for(inp_args.seed, [run_of[i] for i in idxs])) if item_seeds else {}
        if streams[slot] is not None:
            with torch.cuda.stream(streams[slot]):
                out = decode_with_retry(engines[slot], batch.to(dev, non_blocking=True), steps, noise, not joint, sampler, **kw)
        else:
            out = decode_with_retry(engines[slot], batch.to(dev), steps, noise, not joint, sampler, **kw)
        redo = (engines[slot], batch, not joint, noise) + ((kw["seeds"],) if item_seeds else ())
        pending.append((out, idxs, joint, streams[slot], redo, lens))
    while pending:
        retire(pending.pop(0))
    return written_long + written


def main(argv=None):
    synthesis(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
