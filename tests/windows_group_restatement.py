"""Window groups restated in Python from DESIGN.md section 5g, "Several recordings per call" (not from the library), on top of
`windows_restatement` / `windows_dpm_restatement`.  The contract is one sentence: EVERY RECORDING OF A GROUP CALL COMES OUT AS THE
SINGLE-RECORDING WINDOWS CALL GIVES IT ALONE -- its own layout, its own state, its own noise (a tape block, or Philox under its own seed
at epoch 0), its own x0 history; only the timestep and the schedule are shared.  So the reference of a group is the list of the
single-recording references.

Layout: recording r has the windows of `windows_restatement.layout(Ltot_r, Lw, overlap)`, they take the batch items w0_r .. w0_r + W_r - 1
with w0_r = sum_{q<r} W_q, every Ltot_r >= Lw, at most 32 recordings and 32 windows in all.  Packed tensors: recording r's [C][Ltot_r]
block at float offset C * off_r, off_r = sum_{q<r} Ltot_q (`pack` / `unpack`).

`joint_denoise` runs the group as the library does -- ONE batch of all windows per step -- so that the two mutants the tests tell the
scheme from can be expressed: "cover" reads a recording's cover entry without adding w0_r, so its frames blend the batch items 0, 1, ...
(recording 0's windows); "noise" indexes the tape on the packed axis, c * Lsum + off_r + l, instead of the recording's own c * Ltot_r + l.
Without a mutant it is the contract again (the CPU test asserts that)."""
import numpy as np
import torch

from oracle import ldc_oracle as O
import dpm_restatement as D
import windows_dpm_restatement as WD
import windows_restatement as R

MAX_WINDOWS = 32


def layout(Ltots, Lw, overlap, up=1, quantum=None):
    """-> (w0 [R + 1], starts [W_sum] in each recording's own frames).  Raises ValueError for everything the group calls refuse."""
    if not 1 <= len(Ltots) <= MAX_WINDOWS:
        raise ValueError("R")
    w0, starts = [0], []
    for Ltot in Ltots:
        s, _ = R.layout(Ltot, Lw, overlap, up, quantum)
        if Ltot < Lw:
            raise ValueError("Ltot")
        starts += s
        w0.append(len(starts))
    if len(starts) > MAX_WINDOWS:
        raise ValueError("windows")
    return w0, starts


def pack(xs):
    """[1, C, n_r] tensors -> one flat tensor of [C][n_r] blocks"""
    return torch.cat([x.reshape(-1) for x in xs])


def pack_tapes(tapes):
    """[n, 1, C, Ltot_r] tapes -> [n, C * Lsum]: step j of the packed tape is the packed step j of the recordings"""
    return torch.cat([t.reshape(t.shape[0], -1) for t in tapes], dim=1)


def unet_forward_windows_group(sd, u, Xs, t, conds, Lw, overlap, up):
    return [R.unet_forward_windows(sd, u, X, t, c, Lw, overlap, up) for X, c in zip(Xs, conds)]


def denoise_windows_group(sd, u, Xs, conds, n_steps, noises, Lw, overlap, up):
    return [R.denoise_windows(sd, u, X, c, n_steps, nz, Lw, overlap, up) for X, c, nz in zip(Xs, conds, noises)]


def ddim_windows_group(sd, u, Xs, conds, times, eta, noises, Lw, overlap, up):
    return [R.ddim_windows(sd, u, X, c, times, eta, nz, Lw, overlap, up) for X, c, nz in zip(Xs, conds, noises)]


def dpm_windows_group(sd, u, Xs, conds, t_start, S, Lw, overlap, up):
    return [WD.dpm_windows(sd, u, X, c, t_start, S, Lw, overlap, up) for X, c in zip(Xs, conds)]


def mutant_tapes(noises):
    """mutant "noise": recording r reads element (c, l) of step j at c * Lsum + off_r + l of the PACKED step instead of its own block"""
    C = noises[0].shape[2]
    lens = [int(t.shape[3]) for t in noises]
    Lsum, packed = sum(lens), pack_tapes(noises)
    out, off = [], 0
    for n in lens:
        idx = (torch.arange(C)[:, None] * Lsum + off + torch.arange(n)[None, :]).reshape(-1)
        out.append(packed[:, idx].reshape(-1, 1, C, n).contiguous())
        off += n
    return out


def joint_denoise(sd, u, Xs, conds, n_steps, noises, Lw, overlap, up, mutant=None):
    """halfway sampling of the group with ONE batch of all windows per step.  mutant None | "cover" | "noise"."""
    lens = [int(X.shape[2]) for X in Xs]
    w0, _ = layout(lens, Lw, overlap, up)
    lay = [R.weights(n, Lw, overlap, up) for n in lens]                  # (starts, w, cover) of every recording alone
    starts_b = [s for st, _, _ in lay for s in st]                        # per batch item, in its recording's own frames
    w_b = np.concatenate([w for _, w, _ in lay])
    if mutant == "noise":
        noises = mutant_tapes(noises)
    Xs = [X.clone() for X in Xs]
    for j, t in enumerate(reversed(range(n_steps))):
        xs = torch.cat([X[:, :, s:s + Lw] for X, (st, _, _) in zip(Xs, lay) for s in st]).contiguous()
        cs = torch.cat([c[:, :, s // up:(s + Lw) // up] for c, (st, _, _) in zip(conds, lay) for s in st]).contiguous()
        eps = O.unet_forward(sd, u, xs, torch.full((xs.shape[0],), t, dtype=torch.long), cs, prefix=R._prefix(sd))
        for r, (st, w, cover) in enumerate(lay):
            if mutant == "cover" and r > 0:
                # the cover entry's first window is counted within the recording; without w0_r it names the batch items 0, 1, ...: their
                # eps, weights and starts (a row outside the window wraps: the library would read outside the buffer there)
                ebar = torch.zeros_like(Xs[r])
                for g in range(lens[r]):
                    for i, k in enumerate(cover[g]):
                        l = (g - starts_b[k]) % Lw
                        term = float(w_b[k, l]) * eps[k, :, l]
                        ebar[0, :, g] = term if i == 0 else ebar[0, :, g] + term
            else:
                ebar = R.blend(eps[w0[r]:w0[r + 1]], st, w, lens[r])
            Xs[r] = O.p_sample_update(sd, Xs[r], ebar, t, None if t == 0 else noises[r][j])
    return Xs


# ---- the inputs of the GPU tests' groups: windows_restatement.inputs per recording, a seed each (cached there; nothing writes to them)
GROUPS = {"r84": (80, 40, (180, 80, 240)), "r8": (160, 40, (400, 160))}


def seed_of(r):
    return 31 + 7 * r


def inputs(tag, n_steps=40, lens=None):
    lens = lens or GROUPS[tag][2]
    return [R.inputs(tag, Ltot, n_steps, seed=seed_of(r)) for r, Ltot in enumerate(lens)]


_REFS = {}


def reference(tag, n_steps=40, mode=None):
    """denoise of the group GROUPS[tag] on inputs(tag): the contract (mode None: every recording alone) or a mutant of joint_denoise,
    computed once per process"""
    key = (tag, n_steps, mode)
    if key not in _REFS:
        Lw, O_, _ = GROUPS[tag]
        s = inputs(tag, n_steps)
        a = (s[0]["sd"], s[0]["u"], [i["img"] for i in s], [i["cond"] for i in s], n_steps, [i["noise"] for i in s], Lw, O_, s[0]["up"])
        _REFS[key] = denoise_windows_group(*a) if mode is None else joint_denoise(*a, mutant=mode)
    return _REFS[key]


def rel_group(got, ref):
    """the worst recording: max |got_r - ref_r| / max |ref_r|"""
    return max(float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(np.asarray(b, np.float64)).max() + 1e-30))
               for a, b in zip(got, ref))
