"""Coupled windows restated in Python from DESIGN.md section 5g (not from the library): the layout, the weights and the coupled loop on
the CPU oracle's Unet1D.forward (`oracle.unet_forward`), `oracle.p_sample_update` and the DDIM arithmetic the ragged tests restate
(ddpm_loss.py:268-303 with clip_denoised, on the timestep list of ldc_ddim_times).

A window is an ordinary batch item: x_k = X[:, s_k : s_k + Lw], cond_k the matching slice of the RAW condition; the eps of the recording
is ebar(g) = sum_k w_k(g) eps_k(g - s_k), accumulated in float32 in window order, and X moves by the sampler's own update at B = 1,
L = Ltot with the noise of that call.  `mode` selects the mutants the tests tell the scheme from: "end" decodes every window on its own
and blends once at the end, "hard" replaces the cross-fade by a hard switch to the heaviest window."""
import math

import numpy as np
import torch

from oracle import ldc_oracle as O

MAX_WINDOWS = 32


def layout(Ltot, Lw, overlap, up=1, quantum=None):
    """-> (starts, Lw used).  Raises ValueError for everything section 5g refuses."""
    if up < 1:
        raise ValueError("up")
    if Ltot <= 0 or Ltot % up:
        raise ValueError("Ltot")
    if Lw <= 0 or Lw % up or (quantum and Ltot > Lw and Lw % quantum):
        raise ValueError("Lw")
    if overlap < 0 or overlap % up or 2 * overlap > Lw:
        raise ValueError("overlap")
    if Ltot <= Lw:
        return [0], Ltot
    H = Lw - overlap
    W = 1 + math.ceil((Ltot - Lw) / H)
    if W > MAX_WINDOWS:
        raise ValueError("windows")
    return [min(k * H, Ltot - Lw) for k in range(W)], Lw


def weights(Ltot, Lw, overlap, up=1):
    """-> (starts, w [W, Lw] float32, cover: per global frame the list of covering windows)"""
    starts, Lw = layout(Ltot, Lw, overlap, up)
    W = len(starts)
    u = np.ones((W, Lw), np.float64)
    l = np.arange(Lw, dtype=np.float64)
    for k, s in enumerate(starts):
        Rl = starts[k - 1] + Lw - s if k > 0 else 0
        Rr = s + Lw - starts[k + 1] if k + 1 < W else 0
        if Rl > 0:
            u[k] = np.minimum(u[k], (l + 0.5) / Rl)
        if Rr > 0:
            u[k] = np.minimum(u[k], (Lw - l - 0.5) / Rr)
    total = np.zeros(Ltot, np.float64)
    cover = [[] for _ in range(Ltot)]
    for k, s in enumerate(starts):
        total[s:s + Lw] += u[k]
        for g in range(s, s + Lw):
            cover[g].append(k)
    w = np.stack([u[k] / total[s:s + Lw] for k, s in enumerate(starts)]).astype(np.float32)
    return starts, w, cover


def hard_weights(starts, w, Ltot):
    """the argmax mutant: the heaviest covering window takes the whole frame (the first of equals)"""
    Lw = w.shape[1]
    full = np.full((len(starts), Ltot), -1.0, np.float32)
    for k, s in enumerate(starts):
        full[k, s:s + Lw] = w[k]
    best = full.argmax(axis=0)
    out = np.zeros_like(w)
    for g in range(Ltot):
        out[best[g], g - starts[best[g]]] = 1.0
    return out


def blend(per_window, starts, w, Ltot):
    """[W, C, Lw] -> [1, C, Ltot]: sum_k w_k * per_window_k in float32, in window order"""
    Lw = w.shape[1]
    out = torch.zeros(1, per_window.shape[1], Ltot, dtype=torch.float32)
    seen = torch.zeros(Ltot, dtype=torch.bool)
    wt = torch.from_numpy(w)
    for k, s in enumerate(starts):
        term = wt[k] * per_window[k]
        first = ~seen[s:s + Lw]
        out[0, :, s:s + Lw] = torch.where(first, term, out[0, :, s:s + Lw] + term)
        seen[s:s + Lw] = True
    return out


def _prefix(sd):
    return "diffusion.model" if "diffusion.model.init_conv.weight" in sd else "diff_model"


def window_eps(sd, u, X, t, cond, starts, Lw, up):
    """eps of every window as a batch item: [W, C, Lw]"""
    xs = torch.cat([X[:, :, s:s + Lw] for s in starts]).contiguous()
    cs = torch.cat([cond[:, :, s // up:(s + Lw) // up] for s in starts]).contiguous()
    return O.unet_forward(sd, u, xs, torch.full((len(starts),), t, dtype=torch.long), cs, prefix=_prefix(sd))


def unet_forward_windows(sd, u, X, t, cond, Lw, overlap, up):
    starts, w, _ = weights(X.shape[2], Lw, overlap, up)
    return blend(window_eps(sd, u, X, t, cond, starts, w.shape[1], up), starts, w, X.shape[2])


def denoise_windows(sd, u, X, cond, n_steps, noise, Lw, overlap, up, mode="coupled"):
    """halfway sampling of one recording X [1, C, Ltot] on coupled windows; noise [n_steps, 1, C, Ltot]"""
    Ltot = X.shape[2]
    starts, w, _ = weights(Ltot, Lw, overlap, up)
    Lw = w.shape[1]
    if mode == "end":
        outs = [O.halfway_sampling(sd, u, X[:, :, s:s + Lw].contiguous(), cond[:, :, s // up:(s + Lw) // up].contiguous(), n_steps,
                                   noise[:, :, :, s:s + Lw]) for s in starts]
        return blend(torch.cat(outs), starts, w, Ltot), outs
    if mode == "hard":
        w = hard_weights(starts, w, Ltot)
    X = X.clone()
    for j, t in enumerate(reversed(range(n_steps))):
        ebar = blend(window_eps(sd, u, X, t, cond, starts, Lw, up), starts, w, Ltot)
        X = O.p_sample_update(sd, X, ebar, t, None if t == 0 else noise[j])
    return X


def ddim_windows(sd, u, X, cond, times, eta, noise, Lw, overlap, up):
    """DDIM (clip_denoised) of one recording on coupled windows over `times` (n_steps + 1 entries, the last -1)"""
    Ltot = X.shape[2]
    starts, w, _ = weights(Ltot, Lw, overlap, up)
    Lw = w.shape[1]
    ac = sd["diffusion.alphas_cumprod"]
    X = X.clone()
    for j, (t, tn) in enumerate(zip(times[:-1], times[1:])):
        ebar = blend(window_eps(sd, u, X, t, cond, starts, Lw, up), starts, w, Ltot)
        x0 = (sd["diffusion.sqrt_recip_alphas_cumprod"][t] * X - sd["diffusion.sqrt_recipm1_alphas_cumprod"][t] * ebar).clamp(-1.0, 1.0)
        if tn < 0:
            X = x0
            continue
        a, an = ac[t], ac[tn]
        sigma = eta * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
        c = (1 - an - sigma ** 2).clamp(min=0).sqrt()
        X = x0 * an.sqrt() + c * ebar + sigma * noise[j]
    return X


_INPUTS = {}


def inputs(tag, Ltot, n_steps=40, seed=31):
    """One recording for the checks on checkpoint `tag`: raw cond [1, C, Ftot], the normalised start image [1, C, Ltot] it upsamples to
    and a seeded noise tape [n_steps, 1, C, Ltot] (cached: the tests share them, nothing writes to them)."""
    from helpers import CASES, main_sd_np
    from ladiffcodec_amd import synth
    key = (tag, Ltot, n_steps, seed)
    if key not in _INPUTS:
        _, u, _ = CASES[tag]
        up = int(np.prod(u.upsampling_ratios))
        sd = synth.to_torch(main_sd_np(tag))
        g = torch.Generator().manual_seed(seed)
        cond = torch.randn(1, 128, Ltot // up, generator=g)
        img = O.start_image(sd, u, cond)
        noise = torch.randn(n_steps, 1, 128, Ltot, generator=g)
        _INPUTS[key] = dict(sd=sd, u=u, up=up, cond=cond, img=img, noise=noise)
    return _INPUTS[key]


_REFS = {}


def reference(tag, Ltot, Lw, overlap, n_steps=40, mode="coupled"):
    """denoise_windows on inputs(tag, Ltot, n_steps), computed once per process"""
    key = (tag, Ltot, Lw, overlap, n_steps, mode)
    if key not in _REFS:
        s = inputs(tag, Ltot, n_steps)
        _REFS[key] = denoise_windows(s["sd"], s["u"], s["img"], s["cond"], n_steps, s["noise"], Lw, overlap, s["up"], mode=mode)
    return _REFS[key]
