"""DPM-Solver++(2M) items of decode pools: the schedules of tests/test_gpu_pool_dpm.py, the items' start images and conditions on the
CPU oracle without their DDPM decodes (the CPU test needs nothing else of tests/test_gpu_pool.py's `setup`), and the two mutants of the
restatement (tests/dpm_restatement.py) that a pool could compute by mistake: the update without its `b1` term, and the update fed the
x0 history another item left in the slot."""
import torch

from ladiffcodec_amd import sample, synth
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np
from oracle import ldc_oracle as O
import dpm_restatement as R

# name: (item of tests/test_gpu_pool.py whose waveform it is, t_start, n_steps)
DPM = {"three": ("B", 40, 3),        # the smallest schedule on which b1 acts: iteration 1 has a predecessor and is not the last
       "C": ("C", 40, 8),
       "D": ("D", 25, 4),
       "one": ("B", 40, 1),          # the only iteration is the last: the history is neither read nor written
       "two": ("E", 40, 2),          # the history is written once and never read
       "dense": ("D", 6, 6)}         # stride 1
_FRONT = {}


def fronts(tag):
    """-> (sdm, u, {item: (img0, cond)}): the oracle's start image and condition of the five items of tests/test_gpu_pool.py, cut from
    the same waveforms as its `setup` cuts them (whose `ref` holds the same two tensors next to the item's DDPM decode)"""
    if tag not in _FRONT:
        from test_gpu_pool import QUANTA
        mc, u, _ = CASES[tag]
        q = sample.chunk_quantum(mc.enc_ratios)
        lens = [k * q for k in QUANTA[tag]] + [5120]
        src = torch.from_numpy(synth.synthetic_wav(4, max(lens), seed=71)) * 0.5
        sdc, sdm = synth.to_torch(cond_sd_np()), synth.to_torch(main_sd_np(tag))
        items = {}
        for k, (name, n) in enumerate(zip("ABCDE", lens)):
            cond = O.get_cond(sdc, COND_CFG, src[k % 4:k % 4 + 1, :, :n].contiguous())[0]
            items[name] = (O.start_image(sdm, u, cond, True), cond)
        _FRONT[tag] = (sdm, u, items)
    return _FRONT[tag]


def dpm_variant(sd, u, img, cond, t_start, S, drop_b1=False, foreign=None):
    """`dpm_restatement.dpm_sample` (float32 state) with a switch for each mutant -> (latents, [x0_0, x0_1, ...]).
    drop_b1: the history term is left out.  foreign [1, C, L]: iteration 1 reads it in place of the item's own x0_0.
    With neither, the result is dpm_sample's bit for bit (the CPU test asserts it)."""
    ts, coef = R.sd_table(sd, t_start, S)
    coef = torch.from_numpy(coef).to(torch.float32)
    prefix = "diffusion.model" if "diffusion.model.init_conv.weight" in sd else "diff_model"
    Rt, Mt = sd["diffusion.sqrt_recip_alphas_cumprod"], sd["diffusion.sqrt_recipm1_alphas_cumprod"]
    x, prev, hist = img.float(), None, []
    for j in range(S):
        t = int(ts[j])
        eps = O.unet_forward(sd, u, x, torch.full((x.shape[0],), t, dtype=torch.long), cond, prefix=prefix)
        x0 = (Rt[t] * x - Mt[t] * eps).clamp(-1.0, 1.0)
        a, b0, b1 = coef[j]
        if j == 1 and foreign is not None:
            prev = foreign
        if j == S - 1:
            x = x0
        elif prev is None or drop_b1:
            x = a * x + b0 * x0
        else:
            x = a * x + b0 * x0 + b1 * prev
        prev = x0
        hist.append(x0)
    return x, hist


def stale_block(x0_other, L):
    """what an item of L frames would load from a slot's history block that holds another item's x0 [1, C, L']: the block is flat
    memory, the new item reads its first C * L floats as [C][L] (repeated here where the other item was the shorter one)"""
    C = x0_other.shape[1]
    flat = x0_other.reshape(-1)
    flat = flat.repeat(-(-C * L // flat.numel()))[:C * L]
    return flat.reshape(1, C, L).clone()
