"""Time loudnorm's dynamic mode on a multichannel track (MultiChannelJob.dynamic, DESIGN.md
3.9): the frame-by-frame kernel k_ln_dyn<C> and the steps around it.

The case: C = 6, 5 minutes at 48 kHz, synth.mix_like * 0.12 with 50-sample full-scale
bursts twice a second (the tests' signal), which loudnorm sends to dynamic mode.  One
process, HIP events, medians of --reps runs after 3 warm-ups, every step under its own time
limit (a step that passes it ends the process):

  filter1    amx_mc_loudnorm_192k, pass 1: the pairs' upsampling and the filter
  measure    the 192 kHz measurement of its output over the C channels
  filter2    amx_mc_loudnorm_192k, pass 2, on pass 1's 192 kHz stream
  alimiter   the C-channel alimiter at 192 kHz

with the kernel's own cycle split of pass 2 (fill / detect / envelope / output / stats /
r128_out).  --oracle times the CPU oracle's filter (orc_loudnorm, pass 2's options) on the
same track instead, without a GPU; its seconds go into the GPU run's file through
--oracle-cpu-s.  No pass mark: the numbers go to profiles/mc_dynamic_bench.json and
DESIGN.md 3.9.  --device-only: the steps alone, for a pass under a kernel-tracing profiler.

    python scripts/mc_dynamic_bench.py [--seconds 300] [--channels 6] [--reps 15]
"""
import argparse
import faulthandler
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-mastering-engine_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 300
TARGET = -14.0


def git_rev():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                              text=True, check=True).stdout.strip()
    except Exception:   # noqa: BLE001 -- a tree without git metadata
        return None


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed(fn, reps, warmup=3):
    """HIP-event ms of fn() on the current stream, under the step's time limit"""
    import torch
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    try:
        ms = []
        for i in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        return stats(ms)
    finally:
        faulthandler.cancel_dump_traceback_later()


def signal(seconds, fs, C, seed=7):
    """int16 [n, C]: the tests' dynamic-mode signal"""
    import numpy as np
    from amx import synth
    n = int(fs * seconds)
    x = synth.mix_like(n, fs, C, seed=seed) * 0.12
    rng = np.random.default_rng(seed)
    for k in rng.integers(0, n - 200, max(2, int(seconds * 2))):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, C))
    x = np.clip(x, -1.0, 1.0)
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def oracle_time(args):
    import oracle
    x16 = signal(args.seconds, args.fs, args.channels)
    st = oracle.loudnorm_measure(x16, args.fs)
    t0 = time.perf_counter()
    oracle.loudnorm(x16, args.fs, TARGET, measured=st, offset=2.0)
    dt = time.perf_counter() - t0
    print(json.dumps({"oracle_cpu_s": round(dt, 2), "stats": st, "seconds": args.seconds, "channels": args.channels}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--fs", type=int, default=48000)
    ap.add_argument("--channels", type=int, default=6)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--oracle", action="store_true", help="time the CPU oracle's filter on the track (no GPU)")
    ap.add_argument("--oracle-cpu-s", type=float, default=None, help="that time, to record beside the GPU's")
    ap.add_argument("--device-only", action="store_true", help="the steps alone, for a profiler pass")
    ap.add_argument("--rev", default=None, help="the revision to record (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_dynamic_bench.json"))
    args = ap.parse_args()
    if args.oracle:
        return oracle_time(args)
    import torch
    from amx import capi, loudness
    from amx.engine import MultiChannelJob
    from amx.settings import LOUDNORM_LRA, LOUDNORM_TP
    assert torch.cuda.is_available(), "mc_dynamic_bench needs a GPU"
    C, fs = args.channels, args.fs
    x16 = signal(args.seconds, fs, C)
    n = x16.shape[0]
    job = MultiChannelJob(fs, C, {"lufs": TARGET}, n, input_s16=True, chunks=[(0, 0, n)])
    job.out[:n].copy_(torch.from_numpy(x16))
    job.measure(lufs_on=True)
    rep = job.fetch_report(raise_dynamic=False)
    st = rep["stats"][0]
    side = job._side192()
    d1 = capi.LoudnormDesc(TARGET, LOUDNORM_LRA, LOUDNORM_TP, 0.0, 0.0, 99.0, -70.0, 0.0)
    res = {"what": "MultiChannelJob.dynamic's steps on one track (HIP events, medians of %d after 3 warm-ups)"
                   % args.reps,
           "git": args.rev or git_rev(), "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "channels": C, "sample_rate": fs, "frames_192k": side.n192, "mode": rep["modes"][0], "stats": st}
    res["filter1"] = timed(lambda: job.dyn_filter(d1), args.reps)
    res["measure"] = timed(lambda: job.dyn_measure(lufs_on=True), args.reps)
    offset = loudness._fmt(TARGET - float(side.one.stats[0, 0].item()))
    d2 = capi.LoudnormDesc(TARGET, LOUDNORM_LRA, LOUDNORM_TP, float(st["input_i"]), float(st["input_lra"]),
                           float(st["input_tp"]), float(st["input_thresh"]), float(offset))
    d2.reuse_stream = 1
    res["target_offset"] = offset
    res["filter2"] = timed(lambda: job.dyn_filter(d2), args.reps)
    prof = side.summ.cpu().numpy()
    cyc = {k: float(prof[i]) for i, k in enumerate(("fill", "detect", "envelope", "output", "stats", "r128_out"),
                                                   start=2)}
    tot = sum(cyc.values()) or 1.0
    res["filter2_cycle_share"] = {k: round(v / tot, 4) for k, v in cyc.items()}
    res["filter2_detect_calls"], res["filter2_serial_chunks"] = int(prof[8]), int(prof[9])
    res["alimiter"] = timed(lambda: job.dyn_limit(), args.reps)
    res["total_ms"] = round(sum(res[k]["median_ms"] for k in ("filter1", "measure", "filter2", "alimiter")), 3)
    if args.oracle_cpu_s is not None:
        res["oracle_filter_cpu_s"] = args.oracle_cpu_s
    line = json.dumps(res)
    print(line)
    if not args.device_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    job.close()


if __name__ == "__main__":
    main()
