"""`python -m ladiffcodec_amd.sample_dpm` -- the synthesis CLI (`python -m srcs.sample`) with DPM-Solver++(2M) sampling.

Every flag of `srcs.sample` plus `--dpm_steps` (default 10).  The decode starts at `--midway_t` from the upsampled, normalised
condition, as the DDPM and DDIM decodes do, and runs `--dpm_steps` iterations of the second-order multistep solver in its
data-prediction form (Lu et al. 2022) over the timesteps of `sample_ddim`,
reversed(linspace(-1, midway_t - 1, steps + 1)), with the same clipped x0.  The sampler is deterministic: `--seed` changes nothing.
Output naming, batching, `--in_flight`, `--chunk_sec`, `--chunk_overlap_sec` (Engine.decode_dpm_windows), `--ragged` and rank sharding
are those of `srcs.sample`;
`--sampling_timesteps` stays inert, as it is there.
"""
from __future__ import annotations

import argparse

from .sample import DpmSampler, build_parser as _base_parser, synthesis

_DPM_FLAGS = [
    ("--dpm_steps", dict(type=int, default=10, help="DPM-Solver++(2M) iterations from --midway_t (at most --midway_t)")),
]


def build_parser() -> argparse.ArgumentParser:
    p = _base_parser()
    for flag, kw in _DPM_FLAGS:
        p.add_argument(flag, **kw)
    return p


def sampler_from_args(a) -> DpmSampler:
    if not 1 <= a.dpm_steps <= a.midway_t:
        raise SystemExit(f"--dpm_steps {a.dpm_steps}: must be in [1, --midway_t = {a.midway_t}]")
    return DpmSampler(a.midway_t, a.dpm_steps)


def main(argv=None):
    a = build_parser().parse_args(argv)
    return synthesis(a, sampler=sampler_from_args(a))


if __name__ == "__main__":
    main()
