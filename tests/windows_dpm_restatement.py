"""DPM-Solver++(2M) on coupled windows, restated in Python from DESIGN.md sections 5f and 5g (not from the library): the coupled loop of
`windows_restatement` with the update of `dpm_restatement`, on the CPU oracle's Unet1D.forward.

    times, (a, b0, b1)  = dpm_restatement.sd_table(sd, t_start, S)        float64, rounded once to float32
    iteration j:  ebar  = blend(window_eps(X, t_j))                       float32, window order, the first term assigned
                  x0_j  = clamp(R_t X - M_t ebar, -1, 1)
                  X    <- last ? x0_j : a X + b0 x0_j + (j >= 1 ? b1 x0_{j-1} : 0)

on the ONE state X [1, C, Ltot] with the ONE history x0_{j-1} [1, C, Ltot].  Consequences the tests assert: a W = 1 call is
`dpm_restatement.dpm_sample` at B = 1 (bit for bit on the CPU), an overlap-0 call is the batch of independent chunks.

`mode` selects the mutants the tests tell the scheme from: "end" solves every window on its own (a history per window) and blends once
at the end; "first" is the first-order solver (b1 folded into b0: the history is never used).  The third mutant is
`windows_restatement.ddim_windows` at eta 0 on the same timesteps.

Code-driven windows decode has no arithmetic of its own; its contract is "decode_codes_windows(get_cond(wav).codes) is
decode_windows(wav)"."""
import numpy as np
import torch

from oracle import ldc_oracle as O
import dpm_restatement as D
import windows_restatement as R


def dpm_windows(sd, u, X, cond, t_start, S, Lw, overlap, up, mode="coupled"):
    """S iterations from X [1, C, Ltot] on coupled windows; `sd` a torch state dict.  mode "end": -> (blend, [solo results])"""
    Ltot = X.shape[2]
    starts, w, _ = R.weights(Ltot, Lw, overlap, up)
    Lw = w.shape[1]
    if mode == "end":
        outs = [D.dpm_sample(sd, u, X[:, :, s:s + Lw].contiguous(), cond[:, :, s // up:(s + Lw) // up].contiguous(), t_start, S) for s in starts]
        return R.blend(torch.cat(outs), starts, w, Ltot), outs
    ts, coef = D.sd_table(sd, t_start, S)
    coef = torch.from_numpy(coef).to(torch.float32)          # the one rounding of the table
    Rt, Mt = sd["diffusion.sqrt_recip_alphas_cumprod"], sd["diffusion.sqrt_recipm1_alphas_cumprod"]
    X, prev = X.clone(), None
    for j in range(S):
        t = int(ts[j])
        ebar = R.blend(R.window_eps(sd, u, X, t, cond, starts, Lw, up), starts, w, Ltot)
        x0 = (Rt[t] * X - Mt[t] * ebar).clamp(-1.0, 1.0)
        a, b0, b1 = coef[j]
        if j == S - 1:
            X = x0
        elif prev is None:
            X = a * X + b0 * x0
        elif mode == "first":
            X = a * X + (b0 + b1) * x0
        else:
            X = a * X + b0 * x0 + b1 * prev
        prev = x0
    return X


_REFS = {}


def reference(tag, Ltot, Lw, overlap, t_start, S, mode="coupled"):
    """dpm_windows (mode "ddim": windows_restatement.ddim_windows at eta 0 on the same timesteps) on windows_restatement.inputs(tag,
    Ltot), computed once per process; nothing writes to the results"""
    key = (tag, Ltot, Lw, overlap, t_start, S, mode)
    if key not in _REFS:
        s = R.inputs(tag, Ltot)
        if mode == "ddim":
            _REFS[key] = R.ddim_windows(s["sd"], s["u"], s["img"], s["cond"], D.dpm_times(t_start, S), 0.0, torch.zeros_like(s["noise"][:S]),
                                        Lw, overlap, s["up"])
        else:
            _REFS[key] = dpm_windows(s["sd"], s["u"], s["img"], s["cond"], t_start, S, Lw, overlap, s["up"], mode=mode)
    return _REFS[key]


def decode_dpm_windows(sdc, cond_cfg, sdm, mc, u, wav, t_start, S, Lw, overlap):
    """the decode: get_cond and the normalised start image over the whole recording, the coupled DPM loop, the decoder over the whole
    latent, output normalisation.  -> dict(codes, margins, cond, latents, out)"""
    cond, codes, margins, _ = O.get_cond(sdc, cond_cfg, wav, None)
    img0 = O.start_image(sdm, u, cond)
    lat = dpm_windows(sdm, u, img0, cond, t_start, S, Lw, overlap, int(np.prod(u.upsampling_ratios)))
    return dict(codes=codes, margins=margins, cond=cond, latents=lat, out=O.output_normalise(O.seanet_decode(sdm, mc, lat)))
