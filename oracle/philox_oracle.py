"""The device-drawn noise of the samplers, from its definition: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
as easy as 1, 2, 3", SC'11) in exact integer arithmetic, Box-Muller in float64, and the layout that says which block and which of
its four outputs an element of a latent tensor receives ("the noise contract").  Plain numpy, no GPU.

Everything here is written from the specification -- a counter, a key, an index formula -- and vectorised over whole tensors; it does
not walk tiles or threads.  `tests/test_noise_cpu.py` pins it against the published known-answer vectors and checks its statistics;
`tests/test_gpu_noise.py` compares every engine entry that draws with the tapes built here.

Layers, bottom up:
  philox4x32        the block function, any number of rounds (10 is the generator; other counts exist for the tests' mutants)
  block_words       (key, block index g, step word j, stream word) -> the four 32-bit words of the block
  box_muller4 / uniform01   words -> four normals / one uniform
  step_layout       (B, C, L, elem_base) -> block index and output number of every element of a batch part
  call_key / NoiseClock     the key of a call: seed ^ epoch * golden ratio, and which calls advance the epoch
  step_normals / item_normals / start_normal / start_uniform      one tensor of draws
  tape_*            float64 arrays shaped like the `noise` argument of each entry
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl increments of the key
GOLDEN64 = 0x9E3779B97F4A7C15              # the epoch's multiplier in the call key
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

STREAM_START_NORMAL = 0x4C444321           # fourth counter word: one normal per block (start images)
STREAM_START_UNIFORM = 0x4C444322          # one uniform per block (infilling's start image)
STREAM_STEP = 0x4C444323                   # four normals per block (the per-step draws)
STEP_WORD_LOOP, STEP_WORD_INFILL, STEP_WORD_DDIM = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD   # third counter word of a start image

TILE_C, GROUP_C = 32, 8                    # channels c, c+8, c+16, c+24 of a 32-channel tile share a block
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))  # u1 >= 2^-24, so |z| <= sqrt(-2 ln 2^-24) = 5.7681


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """counter [..., 4], key [..., 2] (broadcast over the leading axes) -> uint32 [..., 4].  Round: (hi, lo) of M0 * c0 and M1 * c2;
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key moves on by (W0, W1) between rounds."""
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    c = np.asarray(counter, dtype=np.uint64) & m32
    k = np.asarray(key, dtype=np.uint64) & m32
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c = np.broadcast_to(c, lead + (4,))
    k = np.broadcast_to(k, lead + (2,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(int(rounds)):
        p0 = np.uint64(M0) * c0             # both factors below 2^32: the product fits 64 bits
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & m32, p1 & m32, ((p0 >> s32) ^ c3 ^ k1) & m32, p0 & m32
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def block_words(key: int, g, step_word: int, stream: int, rounds: int = 10) -> np.ndarray:
    """The block of counter (lo(g), hi(g), step_word, stream) under key (lo(key), hi(key)); g any integer array -> uint32 [..., 4]."""
    g = np.asarray(g, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(MASK32), g >> np.uint64(32), np.full(g.shape, step_word & MASK32, np.uint64),
                    np.full(g.shape, stream & MASK32, np.uint64)], axis=-1)
    key = int(key) & MASK64
    return philox4x32(ctr, np.array([key & MASK32, key >> 32], dtype=np.uint64), rounds)


def _u1(w):
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0      # (0, 1]


def _u2(w):
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0              # [0, 1)


def box_muller4(words) -> np.ndarray:
    """words [..., 4] -> float64 [..., 4]: (r0 cos, r0 sin, r1 cos, r1 sin); (u1, u2) of pair h from words (2h, 2h + 1), the top 24
    bits of each; r = sqrt(-2 ln u1), angle 2 pi u2."""
    w = np.asarray(words, np.uint32)
    out = np.empty(w.shape[:-1] + (4,), np.float64)
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(_u1(w[..., 2 * h])))
        a = 2.0 * np.pi * _u2(w[..., 2 * h + 1])
        out[..., 2 * h] = r * np.cos(a)
        out[..., 2 * h + 1] = r * np.sin(a)
    return out


def uniform01(words) -> np.ndarray:
    """the uniform of a start-image block: the top 24 bits of word 0, in [0, 1)"""
    return _u2(np.asarray(words, np.uint32)[..., 0])


# ---- layout ---------------------------------------------------------------------------------------------------------------------
def output_number(C: int) -> np.ndarray:
    """[C]: which of its block's four outputs channel c takes: (c mod 32) div 8"""
    return (np.arange(C) % TILE_C) // GROUP_C


def first_channel(C: int) -> np.ndarray:
    """[C]: the channel whose position names the block of channel c: c - 8 * ((c mod 32) div 8)"""
    return np.arange(C) - GROUP_C * output_number(C)


def step_layout(B: int, C: int, L: int, elem_base: int = 0):
    """-> (g uint64 [B, C, L], out int [C]): element (b, c, l) of a batch part of B items padded to L positions takes output out[c] of
    block g[b, c, l] = elem_base + (b * C + c_first(c)) * L + l.  elem_base is the flat offset of the part in the whole batch."""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    cf = first_channel(C).astype(np.uint64)[None, :, None]
    l = np.arange(L, dtype=np.uint64)[None, None, :]
    g = np.uint64(elem_base) + (b * np.uint64(C) + cf) * np.uint64(L) + l
    return g, output_number(C)


def normals_at(key: int, j: int, g, out, stream: int = STREAM_STEP, rounds: int = 10) -> np.ndarray:
    """output out[c] of block g[b, c, l] at step word j -> float64 [B, C, L]"""
    z4 = box_muller4(block_words(key, g, j, stream, rounds))
    idx = np.broadcast_to(np.asarray(out)[None, :, None, None], g.shape + (1,))
    return np.take_along_axis(z4, idx, axis=-1)[..., 0]


def parts_of(B: int, split: int = 2):
    """[(first item, items)] of a batch decoded as min(split, B) parts: part k holds items [B k / n, B (k + 1) / n)"""
    n = max(1, min(int(split), B))
    return [(B * k // n, B * (k + 1) // n - B * k // n) for k in range(n)]


# ---- keys -----------------------------------------------------------------------------------------------------------------------
def call_key(seed: int, epoch: int) -> int:
    return (int(seed) ^ ((int(epoch) * GOLDEN64) & MASK64)) & MASK64


class NoiseClock:
    """The context's call counter.  `reseed` sets the seed and rewinds the epoch; every sampler entry takes the key of the current
    epoch and, if the call could draw, moves the epoch on.  The conditions, entry by entry:

      p_sample(t, noise)                   noise is None and t > 0      (t = 0 adds no noise: the epoch stays)
      denoise(n_steps, noise)              noise is None                (also for n_steps = 1, whose only step is t = 0)
      p_sample_loop / infilling            noise is None or the start image is drawn on the device
      ddim_sample                          (noise is None and some iteration has sigma > 0) or the start image is drawn on the device
      decode, decode_codes, decode_ragged at t_start 0            noise is None
      decode_ddim, decode_codes_ddim, decode_ragged at t_start > 0     noise is None and some iteration has sigma > 0
      unet_forward*, get_cond, pool calls  never (a pool item's key is its own seed, not the context's)"""

    def __init__(self, seed: int = 0):
        self.reseed(seed)

    def reseed(self, seed: int) -> None:
        self.seed, self.epoch = int(seed) & MASK64, 0

    def key(self, draws: bool = True) -> int:
        k = call_key(self.seed, self.epoch)
        if draws:
            self.epoch += 1
        return k

    def p_sample(self, t: int, noise_given: bool = False) -> int:
        return self.key(not noise_given and t > 0)

    def denoise(self, noise_given: bool = False) -> int:
        return self.key(not noise_given)

    def loop(self, noise_given: bool = False, fill_start: bool = False) -> int:
        """p_sample_loop and infilling"""
        return self.key(not noise_given or fill_start)

    def ddim(self, eta: float, n_steps: int, noise_given: bool = False, fill_start: bool = False) -> int:
        some_sigma = eta > 0.0 and n_steps > 1      # (the last iteration never draws; sigma = eta * (...) > 0 on every other one)
        return self.key((not noise_given and some_sigma) or fill_start)


# ---- one tensor of draws ---------------------------------------------------------------------------------------------------------
def step_normals(key: int, j: int, B: int, C: int, L: int, split: Optional[int] = None, lens: Optional[Sequence[int]] = None) -> np.ndarray:
    """The draws of step word j for a batch [B, C, L] (L the padded length), float64.  split: build the batch part by part as the engine
    decodes it (each part with its own elem_base); None: the whole batch as one part.  The two agree (split independence,
    tests/test_noise_cpu.py).  lens: positions behind lens[b] receive no noise (0 here)."""
    z = np.empty((B, C, L), np.float64)
    for b0, nb in (parts_of(B, split) if split else [(0, B)]):
        g, out = step_layout(nb, C, L, elem_base=b0 * C * L)
        z[b0:b0 + nb] = normals_at(key, j, g, out)
    if lens is not None:
        for b, n in enumerate(lens):
            z[b, :, int(n):] = 0.0
    return z


def item_normals(seed: int, j: int, C: int, length: int) -> np.ndarray:
    """The draws of a pool item at its own step j: the item alone, g = c_first * length + l, key = the item's seed -> [1, C, length]"""
    return step_normals(int(seed) & MASK64, j, 1, C, int(length))


def start_normal(key: int, step_word: int, shape) -> np.ndarray:
    """A device-drawn N(0,1) start image: one element per block at g = flat index, output 0 (r cos) of word pair (0, 1)"""
    g = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return box_muller4(block_words(key, g, step_word, STREAM_START_NORMAL))[..., 0]


def start_uniform(key: int, step_word: int, shape) -> np.ndarray:
    g = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return uniform01(block_words(key, g, step_word, STREAM_START_UNIFORM))


# ---- tapes: float64, shaped like the `noise` argument -------------------------------------------------------------------------------
def tape_p_sample(key: int, B: int, C: int, L: int, split: Optional[int] = None) -> np.ndarray:
    """p_sample(x, t > 0, cond, noise): [B, C, L], step word 0"""
    return step_normals(key, 0, B, C, L, split)


def tape_steps(key: int, n_steps: int, B: int, C: int, L: int, split: Optional[int] = None, lens: Optional[Sequence[int]] = None) -> np.ndarray:
    """denoise, decode, decode_codes, p_sample_loop, ddim_sample, decode_ddim, decode_ragged: [n_steps, B, C, L], entry j = step word j
    (the entry of a step that adds no noise -- t = 0, DDIM's last iteration -- is drawn all the same; the engine does not read it)"""
    return np.stack([step_normals(key, j, B, C, L, split, lens) for j in range(n_steps)])


def tape_infilling(key: int, midway_t: int, B: int, C: int, L: int, split: Optional[int] = None) -> np.ndarray:
    """infilling: [2 * midway_t, B, C, L]; iteration i draws entry 2 i for `img` and 2 i + 1 for `infill`, all under one key"""
    return tape_steps(key, 2 * midway_t, B, C, L, split)


def tape_item(seed: int, n_steps: int, C: int, length: int) -> np.ndarray:
    """a pool item's tape: [n_steps, 1, C, length] on the item's OWN length; seed = submit's `seed`, or the ticket number"""
    return np.stack([item_normals(seed, j, C, length) for j in range(n_steps)])
