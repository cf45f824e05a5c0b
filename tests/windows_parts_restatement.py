"""Coupled windows in batch parts ("Windows in parts"), restated in Python: the partition of the windows
(ldc_window_parts) and the PART-BOUNDARY MUTANT a test of a call in parts has to tell the scheme from.  The scheme itself has no
restatement of its own -- a call in parts must compute what `windows_restatement` computes, whatever P is.

The mutant is what an implementation in parts gets wrong when its update sees one part's eps only: every part blends ITS windows with the
layout's weights (which no longer sum to 1 on a frame that windows of another part cover too) and updates the frames its windows cover,
part after part, so the later part's value wins on the frames both cover."""
import torch

from oracle import ldc_oracle as O
import windows_restatement as R


def partition(W, P):
    """the range starts of W windows in min(P, W) parts: part p holds [floor(p W / P_eff), floor((p + 1) W / P_eff))"""
    if W < 1 or P < 1:
        raise ValueError("W, P")
    pe = min(P, W)
    return [p * W // pe for p in range(pe + 1)]


def blend_by_part(per_window, starts, w, Ltot, first):
    """the mutant's eps: every part's own blend over the frames its windows cover, the later part's value winning"""
    Lw = w.shape[1]
    out = torch.zeros(1, per_window.shape[1], Ltot, dtype=torch.float32)
    for a, b in zip(first[:-1], first[1:]):
        lo, hi = starts[a], starts[b - 1] + Lw
        out[:, :, lo:hi] = R.blend(per_window[a:b], starts[a:b], w[a:b], Ltot)[:, :, lo:hi]
    return out


def denoise_part_mutant(sd, u, X, cond, n_steps, noise, Lw, overlap, up, P):
    """windows_restatement.denoise_windows with blend_by_part in place of the blend"""
    Ltot = X.shape[2]
    starts, w, _ = R.weights(Ltot, Lw, overlap, up)
    Lw = w.shape[1]
    first = partition(len(starts), P)
    X = X.clone()
    for j, t in enumerate(reversed(range(n_steps))):
        ebar = blend_by_part(R.window_eps(sd, u, X, t, cond, starts, Lw, up), starts, w, Ltot, first)
        X = O.p_sample_update(sd, X, ebar, t, None if t == 0 else noise[j])
    return X


_REFS = {}


def mutant_reference(tag, Ltot, Lw, overlap, P, n_steps=40):
    """denoise_part_mutant on windows_restatement.inputs(tag, Ltot, n_steps), computed once per process; nothing writes to it"""
    key = (tag, Ltot, Lw, overlap, P, n_steps)
    if key not in _REFS:
        s = R.inputs(tag, Ltot, n_steps)
        _REFS[key] = denoise_part_mutant(s["sd"], s["u"], s["img"], s["cond"], n_steps, s["noise"], Lw, overlap, s["up"], P)
    return _REFS[key]
