"""The reference of the device-drawn noise (oracle/philox_oracle.py) by itself, no GPU: the published known-answer vectors of
Philox4x32-10, the statistics of the normals, the disjointness of the counter ranges by construction, and eight mutants of the layout that
each move the tape by more than 0.5 in rms -- so any bar below that in tests/test_gpu_noise.py separates the true layout from them.

Bounds.  Moments and correlations are asserted within 4 standard errors of a sample of n independent standard normals: 1 / sqrt(n) for
the mean and for a sample correlation, 1 / sqrt(2 n) for the standard deviation, sqrt(96 / n) for the fourth moment (Var z^4 = 105 - 9).
The inputs are fixed, so a check that passes once passes always.  Two independent N(0,1) tapes differ by sqrt(2) in rms; a mutant that
leaves a fraction f of the elements in place differs by sqrt(2 (1 - f)) (outputs 1 and 2 swapped: f = 1/2, 1.0; c_first taken as c:
f = 1/4, 1.22; elem_base dropped for the second part of B = 3: f = 1/3, 1.15)."""
import numpy as np
import pytest

from oracle import philox_oracle as P
from noise_mutants import mutant_tapes

N_BLOCKS = 1 << 20
KEY = P.call_key(0x0123456789ABCDEF, 0)
B, C = 3, 128                                  # the GPU tests' batch; C = 128 by the model


def h(*words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64)


@pytest.mark.parametrize("counter,key,expect", [
    (("00000000",) * 4, ("00000000",) * 2, ("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8")),
    (("ffffffff",) * 4, ("ffffffff",) * 2, ("408f276d", "41c83b0e", "a20bc7c6", "6d5451fd")),
    (("243f6a88", "85a308d3", "13198a2e", "03707344"), ("a4093822", "299f31d0"), ("d16cfe09", "94fdcceb", "5001e420", "24126ea1")),
])
def test_known_answer_vectors(counter, key, expect):
    got = P.philox4x32(h(*counter), h(*key))
    assert got.dtype == np.uint32 and [f"{int(v):08x}" for v in got] == list(expect)


def test_vectorised_over_leading_axes():
    ctr = np.stack([h(*("00000000",) * 4), h(*("ffffffff",) * 4)]).reshape(2, 1, 4)
    key = np.stack([h(*("00000000",) * 2), h(*("ffffffff",) * 2)]).reshape(2, 1, 2)
    got = P.philox4x32(np.broadcast_to(ctr, (2, 3, 4)), key)
    assert got.shape == (2, 3, 4)
    assert [f"{int(v):08x}" for v in got[0, 2]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    assert [f"{int(v):08x}" for v in got[1, 1]] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    # block_words splits a 64-bit block index and a 64-bit key into the counter / key words
    g = np.array([0x85A308D3243F6A88], dtype=np.uint64)
    w = P.block_words(0x299F31D0A4093822, g, 0x13198A2E, 0x03707344)
    assert [f"{int(v):08x}" for v in w[0]] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_call_key_and_epochs():
    assert P.call_key(5, 0) == 5
    assert P.call_key(5, 1) == 5 ^ 0x9E3779B97F4A7C15
    assert P.call_key(0, 3) == (3 * 0x9E3779B97F4A7C15) % 2 ** 64          # the product wraps at 64 bits
    clk = P.NoiseClock(7)
    assert clk.p_sample(0) == P.call_key(7, 0) and clk.epoch == 0          # t = 0 adds no noise: the epoch stays
    assert clk.p_sample(5, noise_given=True) == P.call_key(7, 0) and clk.epoch == 0
    assert clk.p_sample(5) == P.call_key(7, 0) and clk.epoch == 1
    assert clk.denoise() == P.call_key(7, 1) and clk.epoch == 2
    assert clk.loop(noise_given=True, fill_start=True) == P.call_key(7, 2) and clk.epoch == 3
    assert clk.ddim(0.0, 6) == P.call_key(7, 3) and clk.epoch == 3         # eta 0 draws nothing
    assert clk.ddim(1.0, 6) == P.call_key(7, 3) and clk.epoch == 4
    clk.reseed(9)
    assert clk.key(False) == 9 and clk.epoch == 0


# ------------------------------------------------------------------------------------------------------------------- statistics
@pytest.fixture(scope="module")
def blocks():
    g = np.arange(N_BLOCKS, dtype=np.uint64)
    w = P.block_words(KEY, g, 0, P.STREAM_STEP)
    return g, w, P.box_muller4(w)


def corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1])


def assert_uncorrelated(a, b, what):
    n = np.asarray(a).size
    r = corr(a, b)
    print(f"correlation {what}: {r:+.2e} (4 standard errors {4 / np.sqrt(n):.2e})")
    assert abs(r) < 4.0 / np.sqrt(n), (what, r)


def test_moments_of_the_normals(blocks):
    z = blocks[2].ravel()
    n = z.size
    mean, std, m4 = float(z.mean()), float(z.std()), float((z ** 4).mean())
    print(f"{n} normals: mean {mean:+.4f}, standard deviation {std:.4f}, fourth moment {m4:.3f}")
    assert abs(mean) < 4.0 / np.sqrt(n)
    assert abs(std - 1.0) < 4.0 / np.sqrt(2.0 * n)
    assert abs(m4 - 3.0) < 4.0 * np.sqrt(96.0 / n)


def test_u1_is_never_zero_and_the_normals_are_truncated(blocks):
    _, w, z = blocks
    assert P._u1(w).min() > 0.0 and P._u1(w).max() <= 1.0
    assert P._u2(w).min() >= 0.0 and P._u2(w).max() < 1.0
    # the extreme words: u1 = 2^-24 gives the largest radius, u1 = 1 gives 0
    ext = P.box_muller4(np.array([[0x000000FF, 0, 0xFFFFFFFF, 0]], dtype=np.uint32))[0]
    assert ext[0] == pytest.approx(P.Z_MAX, rel=1e-15) and ext[2] == 0.0
    assert P.Z_MAX == pytest.approx(5.7681, abs=5e-5)
    assert np.abs(z).max() <= P.Z_MAX


def test_the_four_outputs_of_a_block_are_uncorrelated(blocks):
    z = blocks[2]
    for a in range(4):
        for b in range(a + 1, 4):
            assert_uncorrelated(z[:, a], z[:, b], f"outputs {a} and {b}")


def test_items_steps_epochs_and_start_images_are_uncorrelated():
    L = 2048                                                         # 3 x 128 x 2048 = 786 432 elements per tensor
    a = P.step_normals(KEY, 0, B, C, L)
    assert_uncorrelated(a[0], a[1], "items 0 and 1")
    assert_uncorrelated(a[1], a[2], "items 1 and 2")
    assert_uncorrelated(a, P.step_normals(KEY, 1, B, C, L), "steps 0 and 1")
    assert_uncorrelated(a, P.step_normals(P.call_key(0x0123456789ABCDEF, 1), 0, B, C, L), "epochs 0 and 1")
    for word, name in ((P.STEP_WORD_LOOP, "p_sample_loop"), (P.STEP_WORD_DDIM, "ddim")):
        assert_uncorrelated(a, P.start_normal(KEY, word, (B, C, L)), f"the {name} start image and step 0")
    assert_uncorrelated(a, P.start_uniform(KEY, P.STEP_WORD_INFILL, (B, C, L)), "the infilling start image and step 0")
    # a pool item keyed like the call draws item 0's noise only where the two layouts coincide: at equal length they do
    assert np.array_equal(P.item_normals(KEY, 0, C, L)[0], a[0])
    # recorded, not promised: at another length under the SAME key only the rows of c_first = 0 (channels 0, 8, 16, 24 of item 0) keep
    # their blocks; every other row moves with the length
    half = P.item_normals(KEY, 0, C, L // 2)[0]
    assert np.array_equal(half[[0, 8, 16, 24]], a[0, [0, 8, 16, 24], :L // 2])
    rest = np.setdiff1d(np.arange(C), [0, 8, 16, 24])
    assert_uncorrelated(half[rest], a[0, rest, :L // 2], "an item alone at half the length and in the batch, rows of c_first > 0")


def test_split_independence_and_uncorrelated_parts():
    """Promised (the comment at elem_base): the draws do not depend on how the batch is split into parts."""
    Bn, L = 6, 352                                                   # 352 = 11 tiles of 32; 6 items split in 2 and in 3
    whole = P.step_normals(KEY, 2, Bn, C, L)
    for split in (1, 2, 3, 6):
        assert np.array_equal(P.step_normals(KEY, 2, Bn, C, L, split=split), whole), split
    assert P.parts_of(3) == [(0, 1), (1, 2)] and P.parts_of(6, 3) == [(0, 2), (2, 2), (4, 2)] and P.parts_of(1) == [(0, 1)]
    for split in (2, 3):
        parts = P.parts_of(Bn, split)
        for i in range(len(parts)):
            for k in range(i + 1, len(parts)):
                (a0, an), (b0, bn) = parts[i], parts[k]
                assert_uncorrelated(whole[a0:a0 + an], whole[b0:b0 + bn], f"split {split}: parts {i} and {k}")


# ----------------------------------------------------------------------------------------------------------------- disjointness
def counters(g, step_word, stream):
    g = np.asarray(g, dtype=np.uint64).ravel()
    return np.stack([g & np.uint64(P.MASK32), g >> np.uint64(32), np.full(g.shape, step_word, np.uint64), np.full(g.shape, stream, np.uint64)], axis=1)


def test_step_draws_and_start_images_never_share_a_counter():
    """By construction, not by sampling: under one key, the counters of the step draws (every step of a 1000-step loop has its own
    third word), of the three normal start images and of the uniform one are pairwise distinct -- the fourth word separates the
    kinds, the third the steps and the samplers."""
    assert len({P.STREAM_STEP, P.STREAM_START_NORMAL, P.STREAM_START_UNIFORM}) == 3
    assert min(P.STEP_WORD_LOOP, P.STEP_WORD_INFILL, P.STEP_WORD_DDIM) > 2 * 1000   # no step word of any loop reaches a start image's
    L = 80
    g, _ = P.step_layout(B, C, L)
    used = np.unique(g)                                               # the blocks one step consumes
    flat = np.arange(B * C * L, dtype=np.uint64)
    rows = [counters(used, j, P.STREAM_STEP) for j in (0, 1, 2, 999, 1999)]
    rows += [counters(flat, w, P.STREAM_START_NORMAL) for w in (P.STEP_WORD_LOOP, P.STEP_WORD_INFILL, P.STEP_WORD_DDIM)]
    rows += [counters(flat, w, P.STREAM_START_UNIFORM) for w in (P.STEP_WORD_LOOP, P.STEP_WORD_INFILL, P.STEP_WORD_DDIM)]
    # the mutant of the GPU mutation check: step draws on the start images' stream word would collide with nothing either (its third
    # word is a step index), which is why that mutant must be caught by value (test_mutants_of_the_layout), not by this count
    allc = np.concatenate(rows)
    assert len(np.unique(allc, axis=0)) == len(allc)


@pytest.mark.parametrize("Bn,Cn,L", [(3, 128, 160), (3, 128, 80), (2, 128, 33), (2, 40, 7), (1, 128, 1)])
def test_block_indices_within_one_call(Bn, Cn, L):
    """Every valid element (b, c, l) consumes its own (block, output number) pair, and the pairs of the whole batch are those of its
    parts.  L not a multiple of 32: in the last tile the lanes behind L compute block indices g = (b C + c_first) L + l with l >= L,
    which are the indices of positions l - L of the NEXT channel row.  Such a lane owns no element and consumes nothing; the element
    that does own the block, (b, c_first + 1, l - L), is reached from its own row.  If the lanes behind L consumed their blocks the
    pairs would repeat: asserted below, so that the property is not vacuous."""
    g, out = P.step_layout(Bn, Cn, L)
    pairs = (g * np.uint64(4) + out.astype(np.uint64)[None, :, None]).ravel()
    assert len(np.unique(pairs)) == Bn * Cn * L
    # four elements per block, channels c_first + {0, 8, 16, 24} of one position (fewer where C is not a multiple of 32)
    _, counts = np.unique(g, return_counts=True)
    assert counts.max() == min(4, -(-Cn // 8)) and (Cn % 32 != 0 or counts.min() == 4)
    # the parts of a split batch, each laid out from its own elem_base, cover the same pairs
    got = np.concatenate([P.step_layout(nb, Cn, L, elem_base=b0 * Cn * L)[0] for b0, nb in P.parts_of(Bn)])
    assert np.array_equal(got, g)
    if L % 32:
        l_behind = np.arange(L, -(-L // 32) * 32, dtype=np.uint64)     # lanes of the last tile behind L
        cf = np.unique(P.first_channel(Cn)).astype(np.uint64)
        phantom = ((np.arange(Bn, dtype=np.uint64)[:, None, None] * np.uint64(Cn) + cf[None, :, None]) * np.uint64(L) + l_behind[None, None, :]).ravel()
        shared = phantom[np.isin(phantom, g)]
        assert len(shared), "lanes behind L do compute indices that valid elements of the next channel row use"
        # no valid element takes its block from a lane behind L: its index is that of its own row at its own l < L ...
        l = np.arange(L, dtype=np.uint64)[None, None, :]
        assert np.array_equal((g - l) % np.uint64(L), np.zeros_like(g)) and np.array_equal((g - l) // np.uint64(L), np.broadcast_to(g[:, :, :1] // np.uint64(L), g.shape))
        # ... and if those lanes consumed what they compute, (block, output) pairs would be used twice
        ph_pairs = np.concatenate([shared * np.uint64(4) + np.uint64(o) for o in range(4)])
        assert np.isin(ph_pairs, pairs).any()


# ---------------------------------------------------------------------------------------------------------------------- mutants
def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize("L", [160, 80])
def test_mutants_of_the_layout(L):
    seed, n = 0x51ED270B0BADC0DE, 2
    true = P.tape_steps(P.call_key(seed, 0), n, B, C, L, split=2)
    assert true.shape == (n, B, C, L) and true.dtype == np.float64
    muts = mutant_tapes(seed, 0, n, B, C, L)
    assert len(muts) == 8
    for name, tape in muts.items():
        d = rms(tape, true)
        print(f"mutant '{name}' at L = {L}: rms {d:.3f}")
        assert d > 0.5, (name, d)
        assert np.isfinite(tape).all() and abs(float(tape.std()) - 1.0) < 0.02, name      # each still looks like N(0,1)


# ------------------------------------------------------------------------------------------------------------------------ tapes
def test_tape_builders_shapes_and_relations():
    L, key = 80, P.call_key(11, 0)
    t = P.tape_steps(key, 3, B, C, L)
    assert np.array_equal(P.tape_p_sample(key, B, C, L), t[0])
    f = P.tape_infilling(key, 2, B, C, L)
    assert f.shape == (4, B, C, L) and np.array_equal(f[:3], t)       # img and infill alternate along ONE sequence of step words
    item = P.tape_item(1234, 3, C, L)
    assert item.shape == (3, 1, C, L)
    # promised: a pool item draws what a B = 1 denoise draws after reseed(seed), i.e. at epoch 0
    assert np.array_equal(item, P.tape_steps(P.call_key(1234, 0), 3, 1, C, L))
    # not promised, recorded: an item of a ragged batch draws by its position in the PADDED batch, so not what it draws alone
    lens = (80, 160, 240)
    rag = P.tape_steps(key, 2, B, C, 240, split=2, lens=lens)
    for b, n in enumerate(lens):
        assert not rag[:, b, :, n:].any() and rag[:, b, :, :n].all()
    alone = P.tape_steps(key, 2, 1, C, 80)
    assert rms(rag[:, 0:1, :, :80], alone) > 0.5                      # item 0 (length 80) inside Lmax = 240: other blocks
    assert np.array_equal(P.tape_steps(key, 2, B, C, 240, lens=lens), rag)
    s = P.start_normal(key, P.STEP_WORD_DDIM, (B, C, L))
    u = P.start_uniform(key, P.STEP_WORD_INFILL, (B, C, L))
    assert s.shape == u.shape == (B, C, L) and u.min() >= 0.0 and u.max() < 1.0 and abs(float(u.mean()) - 0.5) < 4 / np.sqrt(12 * u.size)
    assert np.array_equal((u * 16777216.0), np.floor(u * 16777216.0))  # 24-bit uniforms: exact in float32
    assert rms(s, P.start_normal(key, P.STEP_WORD_LOOP, (B, C, L))) > 0.5
