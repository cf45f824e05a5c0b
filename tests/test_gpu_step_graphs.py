"""Step graphs on the GPU: the graph launches a sampler loop issues (ldc_host_stats) are the ones the graph-length rule predicts
(ldc_graph_schedule, host-only), for per-part graphs and the fork / join graph, cold, warm and across a change of the "graph_steps"
option; warm loops never wait for the device; every arrangement computes what the eager steps (serial_parts) compute.

An engine of its own: the counts of device synchronisations are exact, so nothing else may have captured on this context."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladiffcodec_amd import lib as L, synth  # noqa: E402
from ladiffcodec_amd.model import Engine  # noqa: E402
from helpers import CASES, COND_CFG, cond_sd_np, main_sd_np  # noqa: E402
from gpu_common import rel  # noqa: E402
from drift_tolerances import TOL  # noqa: E402
import step_graphs_restatement as R  # noqa: E402

SAME = TOL["f32"]["repeat"]
B, LAT, N_STEPS, PARTS = 2, 80, 7, 2          # two parts of one item each at the default split; L = 80: 2560 samples, 8 condition frames


@pytest.fixture(scope="module")
def eng():
    mc, u, _ = CASES["r84"]
    e = Engine(mc, u, COND_CFG, dtype="f32")
    e.load_state_dict(L.MODEL_MAIN, main_sd_np("r84"))
    e.load_state_dict(L.MODEL_COND, cond_sd_np())
    e.finalize(strict=True)
    yield e
    e.close()


def predicted(strided, option, per_part, captures):
    """launches of one loop of N_STEPS from ldc_graph_schedule; the restatement must agree"""
    K, nb, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.check(L.load().ldc_graph_schedule(N_STEPS, PARTS, strided, option, ctypes.byref(K), ctypes.byref(nb), ctypes.byref(ns)))
    n_big, n_single = divmod(N_STEPS - 1, K.value) if captures else (nb.value, ns.value)
    n = (PARTS if per_part else 1) * (n_big + n_single)
    assert n == R.launches(N_STEPS, PARTS, strided, option, per_part, captures)
    return K.value, n


def syncs():
    return L.load().ldc_debug_sync_count()


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_launch_counts_follow_the_graph_schedule(eng, sampler):
    e = eng
    g = torch.Generator().manual_seed(41)
    img = torch.randn(B, 128, LAT, generator=g).cuda()
    cond = torch.randn(B, 128, LAT // 10, generator=g).cuda()
    noise = torch.randn(N_STEPS, B, 128, LAT, generator=g).cuda()          # one tape for every call: its address is part of what a capture binds
    strided = int(sampler == "ddim")

    def run():
        e.host_stats(reset=True)
        if strided:
            out = e.ddim_sample(cond, 40, N_STEPS, 0.6, img=img, noise=noise)
        else:
            out = e.denoise(img, cond, N_STEPS, noise=noise)
        torch.cuda.synchronize()
        return out.cpu().numpy(), e.host_stats(reset=True)[2]

    def check(what, option, per_part, captures, extra_syncs):
        before = syncs()
        out, n = run()
        K, want = predicted(strided, option, per_part, captures)
        err = rel(out, ref)
        print(f"{sampler} {what}: K {K}, {n} launches (predicted {want}), {syncs() - before} device syncs (expected {extra_syncs}), "
              f"against eager {err:.3e} (bar {SAME:.3e})")
        assert n == want, (what, n, want)
        assert syncs() - before == extra_syncs, (what, syncs() - before)
        assert err < SAME, (what, err)
        return K

    try:
        e.set_option("serial_parts", 1)
        ref, n = run()
        assert n == 0 and np.isfinite(ref).all()
        e.set_option("serial_parts", 0)
        # per-part graphs.  K: DDPM 6 (7 divides 7, clamped to n_steps - 1: 1 + 1 replays per part), DDIM 5 (1 + 2)
        out, n = run()                                                      # captures: the first step eagerly, the rest replayed
        K, want = predicted(strided, 0, True, True)
        print(f"{sampler} first call: K {K}, {n} launches (predicted {want})")
        assert K == (5 if strided else 6) and n == want and rel(out, ref) < SAME
        for rep in range(2):
            check(f"warm {rep}", 0, True, False, 0)
        # the option changes K: the binding differs, the built entry is drained (one sync) and captured again
        e.set_option("graph_steps", 3)
        assert check("graph_steps 3, first", 3, True, True, 1) == 3
        check("graph_steps 3, warm", 3, True, False, 0)
        e.set_option("graph_steps", 0)
        check("graph_steps 0 again, first", 0, True, True, 1)
        check("graph_steps 0 again, warm", 0, True, False, 0)
        # one fork / join graph: one launch per replay
        e.set_option("part_graphs", 0)
        check("fork / join, first", 0, False, True, 1)
        for rep in range(2):
            check(f"fork / join, warm {rep}", 0, False, False, 0)
    finally:
        e.set_option("serial_parts", 0)
        e.set_option("graph_steps", 0)
        e.set_option("part_graphs", 1)


def test_pool_launch_counts(eng):
    """a pool steps on per-part graphs of 5 steps and 1 step: 7 steps are 1 + 2 replays per part once the graphs exist"""
    e = eng
    wav = torch.from_numpy(synth.synthetic_wav(1, LAT * 32, seed=43)).cuda() * 0.5
    pool = e.open_pool(2, LAT * 32)
    try:
        pool.submit(wav=wav, n_steps=3 * N_STEPS, seed=7)
        e.host_stats(reset=True)
        pool.step(N_STEPS)                                                  # the first step eagerly, the capture, 1 + 1 replays per part
        torch.cuda.synchronize()
        cold = e.host_stats(reset=True)[2]
        before = syncs()
        pool.step(N_STEPS)
        torch.cuda.synchronize()
        warm = e.host_stats(reset=True)[2]
        print(f"pool of 2 slots, {N_STEPS} steps: {cold} launches capturing, {warm} warm")
        assert cold == PARTS * (1 + 1) and warm == PARTS * (1 + 2)
        assert syncs() == before
    finally:
        pool.close()
