"""`python -m ladiffcodec_amd.sample_ddim` -- the synthesis CLI (`python -m srcs.sample`) with DDIM sampling.

Every flag of `srcs.sample` plus `--ddim_steps` (default 10) and `--ddim_eta` (default 0.0).  The decode starts at
`--midway_t` from the upsampled, normalised condition, as the DDPM decode does, and runs `--ddim_steps` iterations of
the reference's ddim_sample (ddpm_loss.py:268-303) over the timesteps reversed(linspace(-1, midway_t - 1, steps + 1)).
Output naming, batching, `--in_flight`, `--chunk_sec`, `--item_seeds` and rank sharding are those of `srcs.sample`;
`--sampling_timesteps` stays inert, as it is there.
"""
from __future__ import annotations

import argparse

from .sample import DdimSampler, build_parser as _base_parser, synthesis

_DDIM_FLAGS = [
    ("--ddim_steps", dict(type=int, default=10, help="DDIM iterations from --midway_t (at most --midway_t)")),
    ("--ddim_eta", dict(type=float, default=0.0, help="DDIM eta in [0, 1]: 0 deterministic, 1 the DDPM posterior variance")),
]


def build_parser() -> argparse.ArgumentParser:
    p = _base_parser()
    for flag, kw in _DDIM_FLAGS:
        p.add_argument(flag, **kw)
    return p


def sampler_from_args(a) -> DdimSampler:
    if not 1 <= a.ddim_steps <= a.midway_t:
        raise SystemExit(f"--ddim_steps {a.ddim_steps}: must be in [1, --midway_t = {a.midway_t}]")
    if not 0.0 <= a.ddim_eta <= 1.0:
        raise SystemExit(f"--ddim_eta {a.ddim_eta}: must be in [0, 1]")
    return DdimSampler(a.midway_t, a.ddim_steps, a.ddim_eta)


def main(argv=None):
    a = build_parser().parse_args(argv)
    return synthesis(a, sampler=sampler_from_args(a))


if __name__ == "__main__":
    main()
