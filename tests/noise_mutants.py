"""Tapes of the device-drawn noise with ONE thing wrong each, built from the pieces of oracle/philox_oracle.py.  tests/test_noise_cpu.py
asserts that each moves the tape by more than 0.5 in rms; tests/test_gpu_noise.py runs two of them through the engine to show that its
chain bars see a wrong tape."""
import numpy as np

from oracle import philox_oracle as P


def mutant_tapes(seed, epoch, n_steps, Bn, Cn, L):
    """name -> a tape [n_steps, B, C, L] built with ONE thing wrong (shared with tests/test_gpu_noise.py's sensitivity checks)"""
    key = P.call_key(seed, epoch)
    g, out = P.step_layout(Bn, Cn, L)

    def steps(fn):
        return np.stack([fn(j) for j in range(n_steps)])

    def second_part_without_elem_base(j):
        z = np.empty((Bn, Cn, L))
        for b0, nb in P.parts_of(Bn):
            gp, _ = P.step_layout(nb, Cn, L, elem_base=0)
            z[b0:b0 + nb] = P.normals_at(key, j, gp, out)
        return z

    def c_first_is_c(j):
        b = np.arange(Bn, dtype=np.uint64)[:, None, None]
        c = np.arange(Cn, dtype=np.uint64)[None, :, None]
        l = np.arange(L, dtype=np.uint64)[None, None, :]
        return P.normals_at(key, j, (b * np.uint64(Cn) + c) * np.uint64(L) + l, out)

    def from_words(j, pick):
        z4 = pick(P.block_words(key, g, j, P.STREAM_STEP))
        idx = np.broadcast_to(out[None, :, None, None], g.shape + (1,))
        return np.take_along_axis(z4, idx, axis=-1)[..., 0]

    return {
        "j off by one": steps(lambda j: P.normals_at(key, j + 1, g, out)),
        "epoch off by one": steps(lambda j: P.normals_at(P.call_key(seed, epoch + 1), j, g, out)),
        "elem_base dropped for the second part": steps(second_part_without_elem_base),
        "outputs 1 and 2 swapped": steps(lambda j: from_words(j, lambda w: P.box_muller4(w)[..., [0, 2, 1, 3]])),
        "c_first taken as c": steps(c_first_is_c),
        "the start images' stream word": steps(lambda j: P.normals_at(key, j, g, out, stream=P.STREAM_START_NORMAL)),
        "nine rounds": steps(lambda j: P.normals_at(key, j, g, out, rounds=9)),
        "u1 and u2 exchanged": steps(lambda j: from_words(j, lambda w: P.box_muller4(w[..., [1, 0, 3, 2]]))),
    }
