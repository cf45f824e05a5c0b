"""DPM-Solver++(2M), data-prediction form, restated in Python on the CPU oracle's Unet1D.forward: the reference of the DPM tests.

The reference project has no such sampler, so this file plays the role `oracle_ddim` (tests/test_gpu_ragged.py) plays for DDIM.  It is
written from the published update (Lu et al., "DPM-Solver++", 2022, algorithm 2 with the multistep ratio r = h_prev / h), not from
the library's code:

    R_t = sqrt_recip_alphas_cumprod[t] = 1 / alpha_t,   M_t = sqrt_recipm1_alphas_cumprod[t] = sigma_t / alpha_t,   lambda_t = -ln M_t
    x0_j = clamp(R_t x - M_t eps(x, t, cond), -1, 1)
    last iteration (t_next < 0):  x <- x0_j
    else h = lambda_next - lambda_t,  phi = -alpha_next expm1(-h),  a = sigma_next / sigma_t
         j = 0:  x <- a x + phi x0_0
         j > 0:  r = (lambda_t - lambda_prev) / h,  x <- a x + phi (1 + 1/(2r)) x0_j - (phi / (2r)) x0_{j-1}

The table is float64 arithmetic on the checkpoint's two float32 tables, rounded once to float32; the state update is float32
(`state=torch.float64` keeps the table's doubles and a double state: the figure quoted for the float32 state's own error).
The timestep list is the reference's reversed(torch.linspace(-1, t_start - 1, S + 1).int())."""
import numpy as np
import torch

from oracle import ldc_oracle as O


def _f64(v):
    return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)


def dpm_times(t_start, S):
    return list(reversed(torch.linspace(-1, t_start - 1, steps=S + 1).int().tolist()))


def dpm_table(sqrt_recip, sqrt_recipm1, t_start, S):
    """-> (t [S] int, coef [S, 3] float64 rows (a, b0, b1)): x <- a x + b0 x0_j + b1 x0_{j-1}; the final row is (0, 1, 0)"""
    R, M = _f64(sqrt_recip), _f64(sqrt_recipm1)
    alpha, sigma, lam = 1.0 / R, M / R, -np.log(M)
    times = dpm_times(t_start, S)
    ts, coef = [], np.zeros((S, 3), np.float64)
    for j in range(S):
        t, tn = times[j], times[j + 1]
        ts.append(t)
        if tn < 0:
            coef[j] = (0.0, 1.0, 0.0)
            continue
        h = lam[tn] - lam[t]
        phi = -alpha[tn] * np.expm1(-h)
        a = sigma[tn] / sigma[t]
        if j == 0:
            coef[j] = (a, phi, 0.0)
        else:
            r = (lam[t] - lam[times[j - 1]]) / h
            coef[j] = (a, phi * (1.0 + 0.5 / r), -phi * 0.5 / r)
    return np.asarray(ts, np.int64), coef


def sd_table(sd, t_start, S):
    return dpm_table(sd["diffusion.sqrt_recip_alphas_cumprod"], sd["diffusion.sqrt_recipm1_alphas_cumprod"], t_start, S)


def dpm_sample(sd, u, img, cond, t_start, S, state=torch.float32):
    """S iterations from `img` [B, C, L] on the oracle's UNet; `sd` a torch state dict (synth.to_torch)"""
    ts, coef = sd_table(sd, t_start, S)
    coef = torch.from_numpy(coef).to(state)          # (float32: the one rounding of the table)
    prefix = "diffusion.model" if "diffusion.model.init_conv.weight" in sd else "diff_model"
    R, M = sd["diffusion.sqrt_recip_alphas_cumprod"], sd["diffusion.sqrt_recipm1_alphas_cumprod"]
    x, prev = img.to(state), None
    for j in range(S):
        t = int(ts[j])
        eps = O.unet_forward(sd, u, x.float(), torch.full((x.shape[0],), t, dtype=torch.long), cond, prefix=prefix)
        x0 = (R[t].to(state) * x - M[t].to(state) * eps.to(state)).clamp(-1.0, 1.0)
        a, b0, b1 = coef[j]
        if j == S - 1:
            x = x0
        elif prev is None:
            x = a * x + b0 * x0
        else:
            x = a * x + b0 * x0 + b1 * prev
        prev = x0
    return x.float()
