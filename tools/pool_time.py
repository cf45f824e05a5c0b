"""Decode-pool step timings at the BASELINE configs[1] model (diff_dims 256, enc_ratios 8 4, bf16 UNet, synthetic weights), 2.4 s items.

    python tools/pool_time.py [--rounds 7] [--slots 32] [--occupied 1 8 16 32]

  pool      ms per step of a `--slots`-slot pool with 1, 8, 16 and 32 occupied slots (the idle slots are computed on and discarded):
            `DecodePool.step(20)` on a warmed pool, device-event timed, / 20
  ragged    ms per step of `Engine.decode_ragged` at the same B, all lengths equal: the time of a 30-step decode minus that of a
            10-step decode, / 20 (the codec ends and the front end cancel)
  denoise   ms per step of `Engine.denoise` at B = 1 (the fused equal-length plan): 30 steps minus 10 steps, / 20

Every figure is the median over --rounds with min-max, after warm-up (plans built, graphs captured).  One process; run it under its
own `timeout`.  Prints text lines and one JSON line.  A measurement, not a test: nothing is asserted about the numbers."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ragged_time import build_engine  # noqa: E402

T = 38400
STEPS = 20


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    import torch
    from ladiffcodec_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--occupied", type=int, nargs="+", default=[1, 8, 16, 32])
    a = ap.parse_args()
    e = build_engine()
    wav = torch.from_numpy(synth.synthetic_wav(a.slots, T, seed=3)).cuda() * 0.5
    out = {"pool": {}, "ragged": {}, "denoise": {}}

    pool = e.open_pool(a.slots, T)
    tickets = []
    for occ in sorted(a.occupied):
        while len(tickets) < occ:                      # items that outlast the measurement (Philox noise)
            k = len(tickets)
            tickets.append(pool.submit(wav=wav[k:k + 1], n_steps=1000))
        pool.step(2 * STEPS)                           # warm: the first call also captures the graphs
        torch.cuda.synchronize()
        ms = [timed(lambda: pool.step(STEPS)) / STEPS for _ in range(a.rounds)]
        out["pool"][occ] = stats(ms)
        print(f"pool of {a.slots}, {occ} occupied: {out['pool'][occ]} ms per step")
    pool.close()

    def per_step(fn):
        for n in (10, 30):
            for _ in range(2):
                fn(n)
        torch.cuda.synchronize()
        return [(timed(lambda: fn(30)) - timed(lambda: fn(10))) / STEPS for _ in range(a.rounds)]

    for B in sorted(a.occupied):
        w = wav[:B].contiguous()
        out["ragged"][B] = stats(per_step(lambda n: e.decode_ragged(w, [T] * B, n)))
        print(f"decode_ragged B = {B}: {out['ragged'][B]} ms per step")
    img, cond = e.pool_front(wav=wav[:1])
    out["denoise"][1] = stats(per_step(lambda n: e.denoise(img, cond, n)))
    print(f"denoise B = 1: {out['denoise'][1]} ms per step")
    print(json.dumps({"case": "pool_time", "slots": a.slots, "seconds": T / 16000, "steps_timed": STEPS, "rounds": a.rounds, "ms_per_step": out}))
    e.close()


if __name__ == "__main__":
    main()
