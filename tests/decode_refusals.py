"""The fixed list of bad calls behind tests/test_decode_refusals_cpu.py and tests/test_gpu_decode_refusals.py, and the recorder of
tests/golden/decode_refusals.json.

Which refusal an entry gives, in which order and with which text is behaviour: the entries do not agree with each other (ldc_decode looks
at the context before the tensors, ldc_decode_dpm the other way round; some messages say `n_steps must be ...`, others `n_steps %d: must
be ...`).  The table pins every (return code, ldc_last_error()) pair so that a change of the decode plumbing cannot move one unnoticed.
A change of that plumbing leaves the table alone; a change that means to move a refusal records it again, from its parent commit's library
for every row it does not mean to move:

    python tests/decode_refusals.py cpu        # no GPU: the NULL-context list
    python tests/decode_refusals.py gpu        # one MI355X: the live-context list

Each writes its half of the table and leaves the other half as it is.  Set LDC_LIB_PATH to record from another build of the library.

An entry is described by its good arguments (a dict), a function that makes the C call from such a dict, and the checks it makes BEFORE
it looks at the context, in its own order, each as the overrides that make that one check fail.  From these the list takes one call per
check, one call per adjacent pair of checks with both bad (the earlier one must win) and one call with everything good, which stops at
`null ctx`.  An entry that looks at the context first has no such checks: it gets the good call and one with every tensor NULL, both of
which must stop at `null ctx`."""
import ctypes as C
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:       # (run as a script: tests/ is on the path, the package's parent is not)
    sys.path.insert(0, _ROOT)

from ladiffcodec_amd import lib as L  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_refusals.json")

# never dereferenced by a refused call
P = C.c_void_p(4096)
NB = 150           # ldc_packed_bytes(6, 20, 10)


def _i32(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def _int(v):
    return None if v is None else (C.c_int * len(v))(*v)


def _u64(v):
    return None if v is None else (C.c_uint64 * len(v))(*v)


# ---- the calls: one function per entry, from a dict of named arguments -------------------------------------------------------------
def _decode(lib, c, a):
    return lib.ldc_decode(c, a["wav"], a["B"], a["T"], a["n_steps"], None, 1, a["out"], None, None, None, None)


def _decode_ddim(lib, c, a):
    return lib.ldc_decode_ddim(c, a["wav"], a["B"], a["T"], a["t_start"], a["n_steps"], a["eta"], None, 1, a["out"], None, None, None, None)


def _decode_ragged(lib, c, a):
    return lib.ldc_decode_ragged(c, a["wav"], _i32(a["lens"]), a["B"], a["T"], a["t_start"], a["n_steps"], a["eta"], None, a["out"], None, None,
                                 None, None)


def _get_cond_ragged(lib, c, a):
    return lib.ldc_get_cond_ragged(c, a["wav"], _i32(a["lens"]), a["B"], a["T"], 0.0, a["out"], None, None)


def _decode_codes(lib, c, a):
    return lib.ldc_decode_codes(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["B"], a["F"], a["n_steps"], None, 1, a["out"],
                                None, None, None)


def _decode_codes_ddim(lib, c, a):
    return lib.ldc_decode_codes_ddim(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["B"], a["F"], a["t_start"], a["n_steps"],
                                     a["eta"], None, 1, a["out"], None, None, None)


def _decode_codes_ragged(lib, c, a):
    return lib.ldc_decode_codes_ragged(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["B"], a["F"], _i32(a["frames"]),
                                       a["t_start"], a["n_steps"], a["eta"], None, a["out"], None, None, None)


def _decode_seeded(lib, c, a):
    return lib.ldc_decode_seeded(c, a["wav"], _i32(a["lens"]), a["B"], a["T"], a["sampler"], a["t_start"], a["n_steps"], a["eta"],
                                 _u64(a["seeds"]), a["out"], None, None, None, None)


def _decode_codes_seeded(lib, c, a):
    return lib.ldc_decode_codes_seeded(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["B"], a["F"], _i32(a["frames"]),
                                       a["sampler"], a["t_start"], a["n_steps"], a["eta"], _u64(a["seeds"]), a["out"], None, None, None)


def _decode_dpm(lib, c, a):
    return lib.ldc_decode_dpm(c, a["wav"], a["B"], a["T"], a["t_start"], a["n_steps"], 1, a["out"], None, None, None, None)


def _decode_ragged_dpm(lib, c, a):
    return lib.ldc_decode_ragged_dpm(c, a["wav"], _i32(a["lens"]), a["B"], a["T"], a["t_start"], a["n_steps"], a["out"], None, None, None, None)


def _decode_codes_dpm(lib, c, a):
    return lib.ldc_decode_codes_dpm(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["B"], a["F"], a["t_start"], a["n_steps"], 1,
                                    a["out"], None, None, None)


def _decode_windows(lib, c, a):
    return lib.ldc_decode_windows(c, a["wav"], a["T"], a["n_steps"], None, a["Lw"], a["overlap"], a["out"], None, None, None, None)


def _decode_ddim_windows(lib, c, a):
    return lib.ldc_decode_ddim_windows(c, a["wav"], a["T"], a["t_start"], a["n_steps"], a["eta"], None, a["Lw"], a["overlap"], a["out"], None,
                                       None, None, None)


def _decode_dpm_windows(lib, c, a):
    return lib.ldc_decode_dpm_windows(c, a["wav"], a["T"], a["t_start"], a["n_steps"], a["Lw"], a["overlap"], a["out"], None, None, None, None)


def _decode_codes_windows(lib, c, a):
    return lib.ldc_decode_codes_windows(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["F"], a["t_start"], a["n_steps"],
                                        a["eta"], None, a["Lw"], a["overlap"], a["out"], None, None, None)


def _decode_codes_dpm_windows(lib, c, a):
    return lib.ldc_decode_codes_dpm_windows(c, a["codes"], a["packed"], a["stride"], a["bits"], a["n_q"], a["F"], a["t_start"], a["n_steps"],
                                            a["Lw"], a["overlap"], a["out"], None, None, None)


def _decode_windows_group(lib, c, a):
    return lib.ldc_decode_windows_group(c, a["wav"], a["R"], _int(a["Ts"]), a["sampler"], a["t_start"], a["n_steps"], a["eta"], a["noise"],
                                        _u64(a["seeds"]), a["Lw"], a["overlap"], a["out"], None, None, None, None)


def _sample_windows_group(lib, c, a):
    return lib.ldc_sample_windows_group(c, a["img"], a["cond"], a["sampler"], a["t_start"], a["n_steps"], a["eta"], a["noise"],
                                        _u64(a["seeds"]), a["R"], _int(a["Ls"]), _int(a["Fs"]), a["Lw"], a["overlap"], None)


def _denoise_windows(lib, c, a):
    return lib.ldc_denoise_windows(c, a["img"], a["cond"], None, a["n_steps"], a["L"], a["F"], a["Lw"], a["overlap"], None)


def _ddim_sample_windows(lib, c, a):
    return lib.ldc_ddim_sample_windows(c, a["img"], a["cond"], None, a["t_start"], a["n_steps"], a["eta"], a["L"], a["F"], a["Lw"], a["overlap"],
                                       None)


def _dpm_sample_windows(lib, c, a):
    return lib.ldc_dpm_sample_windows(c, a["img"], a["cond"], a["t_start"], a["n_steps"], a["L"], a["F"], a["Lw"], a["overlap"], None)


def _denoise(lib, c, a):
    return lib.ldc_denoise(c, a["img"], a["cond"], None, a["n_steps"], a["B"], a["L"], a["F"], None)


def _ddim_sample(lib, c, a):
    return lib.ldc_ddim_sample(c, a["img"], a["cond"], None, 0, a["t_start"], a["n_steps"], a["eta"], a["B"], a["L"], a["F"], None)


def _dpm_sample(lib, c, a):
    return lib.ldc_dpm_sample(c, a["img"], a["cond"], a["t_start"], a["n_steps"], a["B"], a["L"], a["F"], None)


def _sample_seeded(lib, c, a):
    return lib.ldc_sample_seeded(c, a["img"], a["cond"], a["sampler"], a["t_start"], a["n_steps"], a["eta"], _u64(a["seeds"]), a["B"], a["L"],
                                 a["F"], None)


# ---- the NULL-context list ---------------------------------------------------------------------------------------------------------
WAV = dict(wav=P, out=P, B=2, T=6400, n_steps=4, t_start=30, eta=0.0, lens=[6400, 3200], sampler=0, seeds=[1, 2], Lw=80, overlap=20,
           R=2, Ts=[6400, 3200], noise=None)
CODES = dict(codes=P, packed=None, stride=NB, bits=10, n_q=6, B=2, F=20, n_steps=4, t_start=30, eta=0.0, out=P, frames=[20, 10], sampler=0,
             seeds=[1, 2], Lw=80, overlap=20)
IMG = dict(img=P, cond=P, B=2, L=200, F=20, n_steps=4, t_start=30, eta=0.0, sampler=0, seeds=[1, 2], Lw=80, overlap=20, R=2, Ls=[200, 100],
           Fs=[20, 10], noise=None)

# the context-free checks of codes_args, in its order
# (a check that looks at several arguments lists the other ways to fail it behind the first: each gets a call of its own)
_CODES_ARGS = [("one_of", dict(codes=None, packed=None), dict(packed=P)), ("bad_args", dict(F=0), dict(B=0), dict(out=None)),
               ("n_q", dict(n_q=0)), ("bits", dict(codes=None, packed=P, bits=17), dict(codes=None, packed=P, bits=0)),
               ("stride", dict(codes=None, packed=P, stride=NB - 1))]
_CODES_ARGS_W = [ch if ch[0] != "bad_args" else ("bad_args", dict(F=0), dict(out=None)) for ch in _CODES_ARGS]   # (one recording: no B)
_DPM_ARGS = [("t_start", dict(t_start=0)), ("n_steps", dict(n_steps=31), dict(n_steps=0))]
_ALL_NULL_WAV = dict(wav=None, out=None, B=0, T=0, n_steps=0, t_start=-1, eta=2.0, lens=None)
_ALL_NULL_IMG = dict(img=None, cond=None, B=0, L=0, F=0, n_steps=0, t_start=-1, eta=2.0)

# (id, call, good arguments, [(check, overrides, more overrides ...)] in the entry's order, or the overrides of the all-bad call of a
# context-first entry)
CPU_ENTRIES = [
    ("decode", _decode, WAV, _ALL_NULL_WAV),
    ("decode_ddim", _decode_ddim, WAV, _ALL_NULL_WAV),
    ("decode_ragged", _decode_ragged, WAV, _ALL_NULL_WAV),
    ("get_cond_ragged", _get_cond_ragged, WAV, _ALL_NULL_WAV),
    ("decode_windows", _decode_windows, WAV, _ALL_NULL_WAV),
    ("decode_ddim_windows", _decode_ddim_windows, WAV, _ALL_NULL_WAV),
    ("denoise_windows", _denoise_windows, IMG, _ALL_NULL_IMG),
    ("ddim_sample_windows", _ddim_sample_windows, IMG, _ALL_NULL_IMG),
    ("denoise", _denoise, IMG, _ALL_NULL_IMG),
    ("ddim_sample", _ddim_sample, IMG, _ALL_NULL_IMG),
    ("decode_codes", _decode_codes, CODES, _CODES_ARGS + [("n_steps", dict(n_steps=0))]),
    ("decode_codes_ddim", _decode_codes_ddim, CODES,
     _CODES_ARGS + [("eta", dict(eta=1.5), dict(eta=-0.1), dict(eta=float("nan"))), ("t_start", dict(t_start=0)),
                    ("n_steps", dict(n_steps=31), dict(n_steps=0))]),
    ("decode_codes_ragged", _decode_codes_ragged, CODES,
     # (decode_codes_ragged_impl spells its context-free checks out itself: they are not codes_args, and it has no stride check there)
     [("one_of", dict(codes=None, packed=None), dict(packed=P)), ("bad_args", dict(F=0), dict(B=0), dict(out=None)),
      ("lengths", dict(frames=None)), ("n_q", dict(n_q=0)), ("bits", dict(codes=None, packed=P, bits=0), dict(codes=None, packed=P, bits=17)),
      ("t_start", dict(t_start=-1)), ("n_steps", dict(n_steps=0))]),
    ("decode_seeded", _decode_seeded, dict(WAV, sampler=1),
     [("sampler", dict(sampler=2)), ("seeds", dict(seeds=None)), ("t_start", dict(t_start=0))]),
    ("decode_seeded_alone", _decode_seeded, dict(WAV, sampler=1, lens=None),
     [("sampler", dict(sampler=-1)), ("seeds", dict(seeds=None)), ("t_start", dict(t_start=0))]),
    ("decode_codes_seeded_ragged", _decode_codes_seeded, dict(CODES, sampler=1),
     [("sampler", dict(sampler=2)), ("seeds", dict(seeds=None)), ("t_start", dict(t_start=0)),
      ("one_of", dict(codes=None, packed=None), dict(packed=P)), ("bad_args", dict(B=0), dict(F=0), dict(out=None)), ("n_q", dict(n_q=0)),
      ("bits", dict(codes=None, packed=P, bits=17), dict(codes=None, packed=P, bits=0)), ("n_steps", dict(n_steps=0))]),
    ("decode_codes_seeded_ddim", _decode_codes_seeded, dict(CODES, sampler=1, frames=None),
     [("sampler", dict(sampler=3)), ("seeds", dict(seeds=None)), ("t_start", dict(t_start=0))] + _CODES_ARGS
     + [("eta", dict(eta=float("nan"))), ("n_steps", dict(n_steps=31))]),
    ("decode_codes_seeded_ddpm", _decode_codes_seeded, dict(CODES, sampler=0, frames=None, t_start=0),
     [("sampler", dict(sampler=2)), ("seeds", dict(seeds=None))] + _CODES_ARGS + [("n_steps", dict(n_steps=0))]),
    ("decode_dpm", _decode_dpm, WAV, _DPM_ARGS + [("bad_args", dict(wav=None), dict(out=None), dict(B=0), dict(T=0))]),
    ("decode_ragged_dpm", _decode_ragged_dpm, WAV,
     _DPM_ARGS + [("bad_args", dict(T=0), dict(wav=None), dict(out=None), dict(B=0)), ("lengths", dict(lens=None))]),
    ("decode_codes_dpm", _decode_codes_dpm, CODES, _CODES_ARGS + _DPM_ARGS),
    ("decode_dpm_windows", _decode_dpm_windows, WAV, _DPM_ARGS + [("bad_args", dict(out=None), dict(wav=None), dict(T=0))]),
    ("decode_codes_windows", _decode_codes_windows, CODES,
     _CODES_ARGS_W + [("eta", dict(eta=-0.5)), ("t_start", dict(t_start=-1)), ("n_steps", dict(n_steps=0)), ("n_steps_gt", dict(n_steps=31))]),
    ("decode_codes_dpm_windows", _decode_codes_dpm_windows, CODES, _CODES_ARGS_W + _DPM_ARGS),
    ("decode_windows_group_dpm", _decode_windows_group, dict(WAV, sampler=2),
     [("sampler", dict(sampler=3)), ("t_start", dict(t_start=0)), ("n_steps", dict(n_steps=31)),
      ("bad_args", dict(R=0), dict(wav=None), dict(out=None), dict(Ts=None))]),
    ("decode_windows_group_ddpm", _decode_windows_group, WAV, [("sampler", dict(sampler=-1))]),
    ("sample_windows_group_dpm", _sample_windows_group, dict(IMG, sampler=2),
     [("sampler", dict(sampler=3)), ("t_start", dict(t_start=0)), ("n_steps", dict(n_steps=31)), ("tensors", dict(cond=None), dict(img=None))]),
    ("sample_windows_group_ddim", _sample_windows_group, dict(IMG, sampler=1), [("sampler", dict(sampler=7))]),
    ("dpm_sample_windows", _dpm_sample_windows, IMG, _DPM_ARGS + [("tensors", dict(img=None), dict(cond=None))]),
    ("dpm_sample", _dpm_sample, IMG, _DPM_ARGS + [("tensors", dict(cond=None), dict(img=None))]),
    ("sample_seeded", _sample_seeded, IMG, [("sampler", dict(sampler=2)), ("seeds", dict(seeds=None))]),
]


def _merged(a, b):
    """both checks bad: the overrides of the two, except that the later check's may not mend what the earlier one broke"""
    out = dict(b)
    out.update(a)
    return out


def cpu_calls():
    """[(id, thunk(lib) -> return code)]: every call of the NULL-context list"""
    calls = []
    for name, fn, good, checks in CPU_ENTRIES:
        def add(tag, over, fn=fn, good=good):
            calls.append((f"{name}:{tag}", lambda lib: fn(lib, None, dict(good, **over))))
        add("good", {})
        if isinstance(checks, dict):
            add("all_bad", checks)
            continue
        for tag, *overs in checks:
            for i, over in enumerate(overs):
                add(tag if i == 0 else f"{tag}#{i + 1}", over)
        for (ta, oa, *_), (tb, ob, *_) in zip(checks, checks[1:]):
            add(f"{ta}+{tb}", _merged(oa, ob))
    return calls


# ---- the live-context list: CASES["r84"] with COND_CFG at B = 1, T = one ragged quantum -----------------------------------------------
# cond hop 320, main hop 32, four halvings: the quantum is lcm(320, 32 << 4) = 2560 samples = 8 condition frames = 80 latent frames;
# 1000 timesteps; 6 RVQ layers of 1024 bins (10 bits)
GT, GF, GL, GSTEPS = 2560, 8, 80, 1000
GNB = 60           # ldc_packed_bytes(6, 8, 10)


def gpu_calls(bufs):
    """[(id, thunk(lib, ctx) -> return code)].  bufs: real device buffers (wav, out, codes, packed, img, cond), each large enough for
    the good call at B = 2, so that a call that is NOT refused decodes instead of reading a made-up address."""
    W = dict(WAV, wav=bufs["wav"], out=bufs["out"], B=1, T=GT, lens=[GT], seeds=[1], R=1, Ts=[GT], Lw=GL, overlap=0)
    K = dict(CODES, codes=bufs["codes"], out=bufs["out"], stride=GNB, B=1, F=GF, frames=[GF], seeds=[1], Lw=GL, overlap=0)
    KP = dict(K, codes=None, packed=bufs["packed"])
    I = dict(IMG, img=bufs["img"], cond=bufs["cond"], B=1, L=GL, F=GF, seeds=[1], R=1, Ls=[GL], Fs=[GF], Lw=GL, overlap=0)
    big = GSTEPS + 1
    rows = [
        # n_steps above timesteps
        ("decode:n_steps", _decode, dict(W, n_steps=big)),
        ("decode_ragged:n_steps", _decode_ragged, dict(W, t_start=0, n_steps=big)),
        ("decode_seeded_alone:n_steps", _decode_seeded, dict(W, lens=None, n_steps=big)),
        ("decode_codes:n_steps", _decode_codes, dict(K, n_steps=big)),
        ("decode_codes_ragged:n_steps", _decode_codes_ragged, dict(K, t_start=0, n_steps=big)),
        ("decode_codes_seeded_ddpm:n_steps", _decode_codes_seeded, dict(K, frames=None, t_start=0, n_steps=big)),
        ("decode_windows:n_steps", _decode_windows, dict(W, n_steps=big)),
        ("decode_codes_windows:n_steps", _decode_codes_windows, dict(K, t_start=0, n_steps=big)),
        ("decode_windows_group_ddpm:n_steps", _decode_windows_group, dict(W, n_steps=big)),
        ("sample_windows_group_ddpm:n_steps", _sample_windows_group, dict(I, n_steps=big)),
        ("denoise_windows:n_steps", _denoise_windows, dict(I, n_steps=big)),
        ("denoise:n_steps", _denoise, dict(I, n_steps=big)),
        ("sample_seeded:n_steps", _sample_seeded, dict(I, n_steps=big)),
        # t_start above timesteps
        ("decode_ddim:t_start", _decode_ddim, dict(W, t_start=big)),
        ("decode_ragged:t_start", _decode_ragged, dict(W, t_start=big)),
        ("decode_seeded:t_start", _decode_seeded, dict(W, sampler=1, t_start=big)),
        ("decode_codes_ddim:t_start", _decode_codes_ddim, dict(K, t_start=big)),
        ("decode_codes_ragged:t_start", _decode_codes_ragged, dict(K, t_start=big)),
        ("decode_dpm:t_start", _decode_dpm, dict(W, t_start=big)),
        ("decode_ragged_dpm:t_start", _decode_ragged_dpm, dict(W, t_start=big)),
        ("decode_codes_dpm:t_start", _decode_codes_dpm, dict(K, t_start=big)),
        ("decode_ddim_windows:t_start", _decode_ddim_windows, dict(W, t_start=big)),
        ("decode_dpm_windows:t_start", _decode_dpm_windows, dict(W, t_start=big)),
        ("decode_codes_windows:t_start", _decode_codes_windows, dict(K, t_start=big)),
        ("decode_codes_dpm_windows:t_start", _decode_codes_dpm_windows, dict(K, t_start=big)),
        ("decode_windows_group_dpm:t_start", _decode_windows_group, dict(W, sampler=2, t_start=big)),
        ("sample_windows_group_ddim:t_start", _sample_windows_group, dict(I, sampler=1, t_start=big, seeds=[1])),
        ("ddim_sample_windows:t_start", _ddim_sample_windows, dict(I, t_start=big)),
        ("dpm_sample_windows:t_start", _dpm_sample_windows, dict(I, t_start=big)),
        ("ddim_sample:t_start", _ddim_sample, dict(I, t_start=big)),
        ("dpm_sample:t_start", _dpm_sample, dict(I, t_start=big)),
        ("sample_seeded_ddim:t_start", _sample_seeded, dict(I, sampler=1, t_start=big)),
        # n_q above the codec's layers, bits below the bins' need
        ("decode_codes:n_q", _decode_codes, dict(K, n_q=7)),
        ("decode_codes_ddim:n_q", _decode_codes_ddim, dict(K, n_q=7)),
        ("decode_codes_ragged:n_q", _decode_codes_ragged, dict(K, n_q=7)),
        ("decode_codes_seeded_ddpm:n_q", _decode_codes_seeded, dict(K, frames=None, t_start=0, n_q=7)),
        ("decode_codes_dpm:n_q", _decode_codes_dpm, dict(K, n_q=7)),
        ("decode_codes_windows:n_q", _decode_codes_windows, dict(K, n_q=7)),
        ("decode_codes_dpm_windows:n_q", _decode_codes_dpm_windows, dict(K, n_q=7)),
        ("decode_codes:bits", _decode_codes, dict(KP, bits=9)),
        ("decode_codes_ragged:bits", _decode_codes_ragged, dict(KP, bits=9)),
        ("decode_codes_dpm:bits", _decode_codes_dpm, dict(KP, bits=9)),
        ("decode_codes_windows:bits", _decode_codes_windows, dict(KP, bits=9)),
        # T not a multiple of the hops
        ("decode:T", _decode, dict(W, T=GT + 32)),
        ("decode_ddim:T", _decode_ddim, dict(W, T=GT + 320 // 2)),
        ("decode_dpm:T", _decode_dpm, dict(W, T=GT + 1)),
        ("decode_seeded_alone:T", _decode_seeded, dict(W, lens=None, T=GT + 32)),
        ("decode_windows:T", _decode_windows, dict(W, T=GT + 32)),
        ("decode_dpm_windows:T", _decode_dpm_windows, dict(W, T=GT + 32)),
        ("decode_windows_group_dpm:T", _decode_windows_group, dict(W, sampler=2, Ts=[GT + 32])),
        # a ragged length off the quantum or above Tmax
        ("decode_ragged:len_off", _decode_ragged, dict(W, lens=[GT - 320])),
        ("decode_ragged:len_above", _decode_ragged, dict(W, lens=[2 * GT])),
        ("decode_ragged:Tmax_off", _decode_ragged, dict(W, T=GT + 320, lens=[GT])),
        ("decode_seeded:len_off", _decode_seeded, dict(W, lens=[GT - 320])),
        ("decode_ragged_dpm:len_off", _decode_ragged_dpm, dict(W, lens=[GT - 320])),
        ("decode_ragged_dpm:len_above", _decode_ragged_dpm, dict(W, lens=[2 * GT])),
        ("decode_codes_ragged:len_off", _decode_codes_ragged, dict(K, frames=[GF - 1])),
        ("decode_codes_ragged:len_above", _decode_codes_ragged, dict(K, frames=[2 * GF])),
        ("decode_codes_seeded_ragged:len_off", _decode_codes_seeded, dict(K, t_start=0, frames=[GF - 1])),
        ("get_cond_ragged:len_off", _get_cond_ragged, dict(W, lens=[GT - 1])),
        ("get_cond_ragged:len_above", _get_cond_ragged, dict(W, lens=[GT + 320])),
        # packed_stride below the longest item
        ("decode_codes_ragged:stride", _decode_codes_ragged, dict(KP, stride=GNB - 1)),
        ("decode_codes_seeded_ragged:stride", _decode_codes_seeded, dict(KP, t_start=0, stride=GNB - 1)),
        # R above kWinPerPart; a group call that draws with neither tape nor seeds
        ("decode_windows_group_ddpm:R", _decode_windows_group, dict(W, R=33, Ts=[GT] * 33, seeds=[1] * 33)),
        ("decode_windows_group_dpm:R", _decode_windows_group, dict(W, sampler=2, R=33, Ts=[GT] * 33)),
        ("sample_windows_group_ddpm:R", _sample_windows_group, dict(I, R=33, Ls=[GL] * 33, Fs=[GF] * 33, seeds=[1] * 33)),
        ("decode_windows_group_ddpm:no_seeds", _decode_windows_group, dict(W, seeds=None)),
        ("decode_windows_group_ddim:no_seeds", _decode_windows_group, dict(W, sampler=1, eta=1.0, n_steps=4, seeds=None)),
        ("sample_windows_group_ddpm:no_seeds", _sample_windows_group, dict(I, seeds=None)),
    ]
    # What the entries that look at the context first refuse behind it (the issue's list does not name these; a later merge of the
    # wordings needs them pinned all the same).  ddim_schedule's eta range and its n_steps <= t_start, from every entry that reaches it:
    ddim = [("decode_ddim", _decode_ddim, W), ("decode_ragged", _decode_ragged, W), ("decode_seeded", _decode_seeded, dict(W, sampler=1)),
            ("decode_seeded_alone", _decode_seeded, dict(W, sampler=1, lens=None)), ("decode_ddim_windows", _decode_ddim_windows, W),
            ("decode_windows_group_ddim", _decode_windows_group, dict(W, sampler=1)), ("ddim_sample", _ddim_sample, I),
            ("ddim_sample_windows", _ddim_sample_windows, I), ("sample_windows_group_ddim", _sample_windows_group, dict(I, sampler=1)),
            ("sample_seeded_ddim", _sample_seeded, dict(I, sampler=1)), ("decode_codes_ragged", _decode_codes_ragged, K)]
    for name, fn, a in ddim:
        rows.append((f"{name}:eta", fn, dict(a, eta=1.5)))
        rows.append((f"{name}:eta_nan", fn, dict(a, eta=float("nan"))))
        rows.append((f"{name}:n_steps_gt", fn, dict(a, n_steps=31)))
        rows.append((f"{name}:eta+t_start", fn, dict(a, eta=-0.5, t_start=big)))      # (eta is looked at first)
        rows.append((f"{name}:t_start+n_steps_gt", fn, dict(a, t_start=big, n_steps=big + 1)))
    rows += [
        # the tensors and sizes, and their precedence against the sampler's arguments
        ("decode:bad_args", _decode, dict(W, wav=None)),
        ("decode:bad_args#2", _decode, dict(W, out=None)),
        ("decode:bad_args#3", _decode, dict(W, B=0)),
        ("decode:bad_args#4", _decode, dict(W, T=0)),
        ("decode:bad_args+n_steps", _decode, dict(W, out=None, n_steps=big)),
        ("decode:n_steps+T", _decode, dict(W, n_steps=0, T=GT + 32)),
        ("decode_ddim:bad_args", _decode_ddim, dict(W, wav=None)),
        ("decode_ddim:bad_args+eta", _decode_ddim, dict(W, B=0, eta=1.5)),
        ("decode_ddim:eta+T", _decode_ddim, dict(W, eta=1.5, T=GT + 32)),
        ("decode_ragged:bad_args", _decode_ragged, dict(W, wav=None)),
        ("decode_ragged:bad_args+t_start", _decode_ragged, dict(W, B=0, t_start=-1)),
        ("decode_ragged:t_start_neg", _decode_ragged, dict(W, t_start=-1)),
        ("decode_ragged:t_start_neg+lengths", _decode_ragged, dict(W, t_start=-1, lens=None)),
        ("decode_ragged:lengths", _decode_ragged, dict(W, lens=None)),
        ("decode_ragged:len_off+eta", _decode_ragged, dict(W, lens=[GT - 320], eta=1.5)),
        ("decode_seeded_alone:bad_args", _decode_seeded, dict(W, lens=None, out=None)),
        ("decode_seeded_alone:bad_args+n_steps", _decode_seeded, dict(W, lens=None, T=0, n_steps=big)),
        ("get_cond_ragged:bad_args", _get_cond_ragged, dict(W, wav=None)),
        ("get_cond_ragged:bad_args#2", _get_cond_ragged, dict(W, out=None)),
        ("get_cond_ragged:bad_args+lengths", _get_cond_ragged, dict(W, B=0, lens=None)),
        ("get_cond_ragged:lengths", _get_cond_ragged, dict(W, lens=None)),
        ("decode_windows:bad_args", _decode_windows, dict(W, wav=None)),
        ("decode_windows:bad_args+n_steps", _decode_windows, dict(W, T=0, n_steps=big)),
        ("decode_ddim_windows:bad_args", _decode_ddim_windows, dict(W, out=None)),
        ("decode_ddim_windows:bad_args+eta", _decode_ddim_windows, dict(W, T=0, eta=1.5)),
        ("decode_windows_group_ddpm:bad_args", _decode_windows_group, dict(W, wav=None)),
        ("decode_windows_group_ddpm:bad_args+n_steps", _decode_windows_group, dict(W, R=0, n_steps=big)),
        ("decode_windows_group_ddim:bad_args+eta", _decode_windows_group, dict(W, sampler=1, out=None, eta=1.5)),
        ("denoise:tensors", _denoise, dict(I, img=None)),
        ("denoise:tensors#2", _denoise, dict(I, cond=None)),
        ("denoise:tensors+n_steps", _denoise, dict(I, cond=None, n_steps=big)),
        ("denoise:n_steps+sizes", _denoise, dict(I, n_steps=0, L=GL + 1)),
        ("denoise:sizes", _denoise, dict(I, L=GL + 1)),
        ("denoise:sizes#2", _denoise, dict(I, B=0)),
        ("ddim_sample:tensors", _ddim_sample, dict(I, img=None)),
        ("ddim_sample:tensors+sizes", _ddim_sample, dict(I, cond=None, L=GL + 1)),
        ("ddim_sample:sizes+eta", _ddim_sample, dict(I, L=GL + 1, eta=1.5)),
        ("denoise_windows:tensors", _denoise_windows, dict(I, cond=None)),
        ("denoise_windows:tensors+n_steps", _denoise_windows, dict(I, img=None, n_steps=big)),
        ("ddim_sample_windows:tensors+eta", _ddim_sample_windows, dict(I, img=None, eta=1.5)),
        ("sample_windows_group_ddpm:tensors", _sample_windows_group, dict(I, img=None)),
        ("sample_windows_group_ddpm:tensors+n_steps", _sample_windows_group, dict(I, cond=None, n_steps=big)),
        ("sample_seeded:tensors", _sample_seeded, dict(I, img=None)),
        ("sample_seeded:tensors+n_steps", _sample_seeded, dict(I, cond=None, n_steps=big)),
        ("sample_seeded:n_steps+sizes", _sample_seeded, dict(I, n_steps=0, L=GL + 1)),
        ("sample_seeded_ddim:sizes+eta", _sample_seeded, dict(I, sampler=1, L=GL + 1, eta=1.5)),
        ("dpm_sample:sizes", _dpm_sample, dict(I, L=GL + 1)),
        ("dpm_sample:sizes+t_start", _dpm_sample, dict(I, B=0, t_start=big)),
    ]
    return [(name, (lambda lib, ctx, fn=fn, a=a: fn(lib, ctx, a))) for name, fn, a in rows]


def fp8_calls(bufs):
    """the ragged refusal of an fp8 engine, from every entry that gives it (none of them reads Lw, overlap or R)"""
    W = dict(WAV, wav=bufs["wav"], out=bufs["out"], B=1, T=GT, lens=[GT], seeds=[1])
    K = dict(CODES, codes=bufs["codes"], out=bufs["out"], stride=GNB, B=1, F=GF, frames=[GF], seeds=[1])
    rows = [
        ("fp8:decode_ragged", _decode_ragged, W),
        ("fp8:decode_ragged_dpm", _decode_ragged_dpm, W),
        ("fp8:decode_seeded", _decode_seeded, W),
        ("fp8:decode_codes_ragged", _decode_codes_ragged, K),
        ("fp8:decode_codes_seeded_ragged", _decode_codes_seeded, dict(K, t_start=0)),
    ]
    return [(name, (lambda lib, ctx, fn=fn, a=a: fn(lib, ctx, a))) for name, fn, a in rows]


def device_buffers():
    import torch
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    t = dict(wav=z(2 * 2 * GT), out=z(2 * 2 * GT), codes=z(6 * 2 * 2 * GF, torch.int64), packed=z(4 * GNB, torch.uint8), img=z(2 * 128 * 2 * GL),
             cond=z(2 * 128 * 2 * GF))
    bufs = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    bufs["_keep"] = t
    return bufs


def gpu_names():
    """the ids of the live-context list (no device buffer is made for this)"""
    none = dict.fromkeys(("wav", "out", "codes", "packed", "img", "cond"))
    return [name for name, _ in gpu_calls(none) + fp8_calls(none)]


def run(calls, *ctx):
    lib = L.load()
    return {name: [int(fn(lib, *ctx)), lib.ldc_last_error().decode()] for name, fn in calls}


def load_table():
    with open(TABLE) as fo:
        return json.load(fo)


def _record(which):
    table = load_table() if os.path.exists(TABLE) else {}
    if which == "cpu":
        table["cpu"] = run(cpu_calls())
    else:
        from gpu_common import engine
        bufs = device_buffers()
        table["gpu"] = run(gpu_calls(bufs), engine("r84", "f32")._ctx)
        table["gpu"].update(run(fp8_calls(bufs), engine("r84", "fp8")._ctx))
    with open(TABLE, "w") as fo:
        json.dump(table, fo, indent=1, sort_keys=True)
        fo.write("\n")
    print("recorded", which, len(table[which]), "calls")


if __name__ == "__main__":
    _record(sys.argv[1])
