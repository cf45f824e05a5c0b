"""Generate tests/golden/ddim_r84.npz: the reference's GaussianDiffusion1D.ddim_sample (ddpm_loss.py:268-303) on the synthetic
r84 checkpoint (the weights of tools/gen_golden.py's drivers_case), with injected start images and noise draws.

Run in the build container only:   python tools/gen_golden_ddim.py [OUT.npz]
The start images and noise tapes are regenerated at test time from the recorded seeds (tests/test_gpu_ddim.py: ddim_inputs), so
the fixture holds the condition, the halfway start image and the four results.  The archive is written with fixed zip
timestamps: two runs give byte-identical files.

Cases (B = 2, T = 2560, L = 80):
  a  t_start 1000, S 10, eta 0.0, N(0,1) start image
  b  t_start 1000, S 25, eta 0.7, N(0,1) start image, noise tape
  c  t_start 20,   S 6,  eta 0.0, the upsampled, per-item max-normalised condition (the DDIM form of halfway_sampling:
     num_timesteps set to 20, torch.randn patched to return the start image)
  d  t_start 8,    S 8,  eta 1.0, N(0,1) start image, noise tape
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from gen_golden import build_cond_model, build_main_model, np32  # noqa: E402
from ref_import import import_reference  # noqa: E402
from ladiffcodec_amd import synth  # noqa: E402
from ladiffcodec_amd.spec import CodecConfig, UnetConfig  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ddim_r84.npz")
# (name, t_start, S, eta, seed of the start image, seed of the noise tape); must match tests/test_gpu_ddim.py
CASES = [("a", 1000, 10, 0.0, 301, 302), ("b", 1000, 25, 0.7, 303, 304), ("c", 20, 6, 0.0, None, 306), ("d", 8, 8, 1.0, 307, 308)]
B, T, SEED_W, SEED_WAV = 2, 2560, 21, 777


def save_npz(path, arrays):
    """np.savez layout with a fixed timestamp per member (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


class NoiseTape:
    """torch.randn_like inside the reference's ddpm_loss returns the recorded draws in order."""

    def __init__(self, noises):
        self.noises, self.i = noises, 0

    def __call__(self, x):
        n = self.noises[self.i]
        self.i += 1
        assert n.shape == x.shape
        return n


def main():
    torch.set_num_threads(8)
    ref = import_reference()
    import srcs.losses.ddpm_loss as ref_ddpm
    mc = CodecConfig(enc_ratios=(8, 4), quantization=False)
    u = UnetConfig(dim=32, upsampling_ratios=(5, 2), unet_scale_cond=True)
    cond_model = build_cond_model(ref, CodecConfig(enc_ratios=(8, 5, 4, 2), quantization=True, bandwidth=3.0), seed=11)
    main_model = build_main_model(ref, mc, u, seed=SEED_W)
    diff = main_model.diffusion
    L = T // mc.hop_length
    wav = torch.from_numpy(synth.synthetic_wav(B, T, seed=SEED_WAV)) * 0.5
    out = {"wav": np32(wav), "meta": np.array([SEED_W, T, SEED_WAV, B], np.int64),
           "cases": np.array([[t0, S, int(round(eta * 1000)), -1 if si is None else si, sn] for _, t0, S, eta, si, sn in CASES], np.int64)}
    with torch.no_grad():
        cond = cond_model.get_cond(wav)
        out["cond"] = np32(cond)
        up = cond
        for layer in main_model.diff_model.upsampling_layers:
            up = layer(up)
        start_c = up / (up.abs().amax(dim=(1, 2), keepdim=True) + 1e-8)   # per item, as the decode normalises a batch of mono files
        out["start_c"] = np32(start_c)
        saved_randn, saved_like, saved_tqdm = ref_ddpm.torch.randn, ref_ddpm.torch.randn_like, ref_ddpm.tqdm
        try:
            ref_ddpm.tqdm = lambda it, **k: it
            for name, t_start, S, eta, seed_img, seed_noise in CASES:
                img0 = start_c if seed_img is None else torch.randn(B, 128, L, generator=torch.Generator().manual_seed(seed_img))
                g = torch.Generator().manual_seed(seed_noise)
                tape = NoiseTape([torch.randn(B, 128, L, generator=g) for _ in range(S)])
                diff.num_timesteps, diff.sampling_timesteps, diff.ddim_sampling_eta = t_start, S, eta
                ref_ddpm.torch.randn = lambda *a, **k: img0.clone()
                ref_ddpm.torch.randn_like = tape
                res = diff.ddim_sample((B, 128, L), condition=cond, clip_denoised=True)
                ref_ddpm.torch.randn, ref_ddpm.torch.randn_like = saved_randn, saved_like
                assert tape.i == S - 1, (name, tape.i)
                out["out_" + name] = np32(res)
                print(f"ddim {name}: t_start {t_start} S {S} eta {eta}: absmax {float(res.abs().max()):.4f}")
        finally:
            ref_ddpm.torch.randn, ref_ddpm.torch.randn_like, ref_ddpm.tqdm = saved_randn, saved_like, saved_tqdm
            diff.num_timesteps = 1000
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
