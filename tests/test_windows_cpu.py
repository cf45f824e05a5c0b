"""Coupled windows without a GPU: ldc_window_layout (host-only) against the Python restatement, every refusal of
the layout, the identities of the scheme on the CPU oracle (W = 1 is halfway sampling, overlap 0 is the batch of independent chunks),
the discrimination conditions the GPU tests rely on -- asserted here on the reference alone -- and the CLI flag."""
import numpy as np
import pytest
import torch

from ladiffcodec_amd import lib as L, sample, sample_ddim
from drift_tolerances import TOL
from oracle import ldc_oracle as O
import windows_restatement as R

TRIPLES = [(200, 80, 20), (180, 80, 40), (240, 80, 0), (81, 80, 40), (100, 80, 10), (60, 80, 20), (80, 80, 40), (2560, 80, 0), (1320, 80, 40)]


@pytest.mark.parametrize("triple", TRIPLES)
def test_layout_and_weights_against_the_restatement(triple):
    Ltot, Lw, O_ = triple
    starts, w = L.window_layout(Ltot, Lw, O_, 1)
    rs, rw, cover = R.weights(Ltot, Lw, O_)
    lw = min(Lw, Ltot)
    assert starts == rs and len(starts) == (1 if Ltot <= Lw else 1 + -(-(Ltot - Lw) // (Lw - O_)))
    assert starts[-1] == Ltot - lw                                   # the last window is right-aligned
    assert w.shape == (len(starts), lw) and w.dtype == np.float32
    assert np.array_equal(w, rw)                                     # double arithmetic, rounded once: bit for bit
    total = np.zeros(Ltot, np.float64)
    count = np.zeros(Ltot, np.int64)
    for k, s in enumerate(starts):
        total[s:s + lw] += w[k].astype(np.float64)
        count[s:s + lw] += 1
    assert count.min() >= 1 and count.max() <= 3
    assert [len(c) for c in cover] == list(count)
    for c in cover:
        assert c == list(range(c[0], c[0] + len(c)))                 # consecutive windows
    print(triple, "max |sum w - 1| =", np.abs(total - 1).max())
    assert np.abs(total - 1).max() <= 1.2e-7
    for k, s in enumerate(starts):
        assert np.all(w[k][count[s:s + lw] == 1] == np.float32(1.0))
        assert np.all(w[k] > 0)


def test_the_issues_worked_examples():
    assert L.window_layout(200, 80, 20, 10)[0] == [0, 60, 120]
    assert L.window_layout(180, 80, 40, 10)[0] == [0, 40, 80, 100]
    _, _, cover = R.weights(180, 80, 40)
    assert [g for g, c in enumerate(cover) if len(c) == 3] == list(range(100, 120))
    starts, w = L.window_layout(240, 80, 0, 10)
    assert starts == [0, 80, 160] and np.all(w == 1.0)
    # a plain overlap is a linear cross-fade: (l + 0.5) / R rising, its mirror image falling
    starts, w = L.window_layout(200, 80, 20, 10)
    ramp = (np.arange(20) + 0.5) / 20
    assert np.allclose(w[1][:20], ramp, atol=1e-7) and np.allclose(w[0][60:], 1 - ramp, atol=1e-7)


@pytest.mark.parametrize("bad,word", [
    ((185, 80, 40, 10), "Ltot 185"), ((0, 80, 40, 10), "Ltot 0"), ((-10, 80, 40, 10), "Ltot -10"),
    ((180, 85, 40, 10), "Lw 85"), ((180, 0, 0, 10), "Lw 0"),
    ((180, 80, 45, 10), "overlap 45"), ((180, 80, 50, 10), "overlap 50"), ((180, 80, -10, 10), "overlap -10"),
    ((80 + 32 * 40, 80, 40, 10), "33 windows"), ((180, 80, 40, 0), "up 0"),
])
def test_layout_refusals_name_the_value(bad, word):
    with pytest.raises(L.LdcError) as ei:
        L.window_layout(*bad)
    assert ei.value.code == L.E_INVALID and word in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        R.layout(*bad)


def test_thirty_two_windows_are_accepted():
    starts, _ = L.window_layout(80 + 31 * 40, 80, 40, 10)
    assert len(starts) == 32


def test_one_window_is_halfway_sampling():
    s = R.inputs("r84", 80, 6)
    got = R.denoise_windows(s["sd"], s["u"], s["img"], s["cond"], 6, s["noise"], 160, 40, s["up"])
    ref = O.halfway_sampling(s["sd"], s["u"], s["img"], s["cond"], 6, s["noise"])
    assert torch.equal(got, ref)


def test_overlap_zero_is_the_batch_of_independent_chunks():
    s = R.inputs("r84", 240, 6)
    got = R.denoise_windows(s["sd"], s["u"], s["img"], s["cond"], 6, s["noise"], 80, 0, s["up"])
    cut = lambda x, n: torch.cat([x[..., k * n:(k + 1) * n] for k in range(3)], dim=-3)      # noqa: E731  [.., 1, C, 3 n] -> [.., 3, C, n]
    ref = O.halfway_sampling(s["sd"], s["u"], cut(s["img"], 80), cut(s["cond"], 8), 6, cut(s["noise"], 80))
    assert torch.equal(got, torch.cat(list(ref[:, None]), dim=-1))


def test_discrimination_conditions_on_the_reference():
    """What the GPU comparisons can tell apart, on the oracle alone: r84, Ltot 180, Lw 80, overlap 40, 40 steps, seeded tape."""
    bar = TOL["f32"]["chain_small"]
    ref = R.reference("r84", 180, 80, 40)
    end, solo = R.reference("r84", 180, 80, 40, mode="end")
    hard = R.reference("r84", 180, 80, 40, mode="hard")
    m = float(ref.abs().max())
    d_end, d_hard = float((ref - end).abs().max()) / m, float((ref - hard).abs().max()) / m
    seam = float((solo[0][:, :, 40:] - solo[1][:, :, :40]).abs().max()) / m
    print(f"coupled vs blended at the end {d_end:.3e}, vs hard switch {d_hard:.3e}, independent windows on their overlap {seam:.3e} (bar {bar:.1e})")
    assert d_end >= 10 * bar
    assert d_hard >= 10 * bar
    assert seam > 1e-2


def test_cli_flag_parsing_and_refusals():
    for mod in (sample, sample_ddim):
        p = mod.build_parser()
        assert "chunk_overlap_sec" not in vars(p.parse_args([]))              # absent unless given: a run without it is what it was
        assert sample.windows_options(p.parse_args(["--chunk_sec", "2.4"])) is None
        assert sample.windows_options(p.parse_args(["--chunk_sec", "2.4", "--chunk_overlap_sec", "0.4"])) == 0.4
        assert sample.windows_options(p.parse_args(["--chunk_sec", "2.4", "--chunk_overlap_sec", "0"])) == 0.0
        for bad in (["--chunk_overlap_sec", "0.4"], ["--chunk_sec", "2.4", "--chunk_overlap_sec", "1.3"],
                    ["--chunk_sec", "2.4", "--chunk_overlap_sec", "-0.1"]):
            with pytest.raises(SystemExit):
                sample.windows_options(p.parse_args(bad))
        assert "coupled" in p.format_help().lower()
    # 2.4 s windows overlapping by 0.4 s: 1200 and 200 latent frames for enc_ratios 8 4 (hop 32, up 10), as the timing tool uses
    assert sample.window_grid(2.4, 0.4, [8, 4], [5, 2]) == (1200, 200)
    assert sample.window_grid(2.4, 0.4, [8], [5, 4, 2]) == (4800, 800)
    assert sample.window_grid(0.16, 0.09, [8, 4], [5, 2]) == (80, 40)          # rounded down to condition frames, capped at Lw / 2
    assert sample.window_grid(0.01, 0.0, [8, 4], [5, 2]) == (80, 0)            # at least one quantum


def test_segments_of_at_most_32_windows():
    assert sample.plan_window_segments(180, 80, 40, 10) == [(0, 180)]
    seg = 80 + 31 * 40
    assert sample.plan_window_segments(seg, 80, 40, 10) == [(0, seg)]
    assert sample.plan_window_segments(seg + 200, 80, 40, 10) == [(0, seg), (seg, 200)]
    assert sample.plan_window_segments(seg + 30, 80, 40, 10) == [(0, seg - 50), (seg - 50, 80)]   # the tail borrows whole condition frames
    for Ltot in (seg + 10, 2 * seg + 70, 3 * seg):
        plan = sample.plan_window_segments(Ltot, 80, 40, 10)
        assert plan[0][0] == 0 and sum(n for _, n in plan) == Ltot
        assert all(a + n == b for (a, n), (b, _) in zip(plan, plan[1:]))
        assert all(n >= 80 and n % 10 == 0 and len(L.window_layout(n, 80, 40, 10)[0]) <= 32 for _, n in plan)
