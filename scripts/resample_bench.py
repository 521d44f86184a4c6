"""Time the output resampler (amx_resampler_run) on the masters it is for,
beside the device-to-host copy it shortens.

Cases: the C3 programme (5 minutes of stereo) as loudnorm's dynamic mode leaves it, 57.6 M
frames at 192 kHz, to 48 kHz and to 44.1 kHz; and as its linear mode leaves it, 14.4 M
frames at 48 kHz, to 44.1 kHz.  The samples are random full-range int16 (the kernel's time
does not depend on them).  One process, HIP events, medians of --reps runs after 3
warm-ups, every step under its own time limit (a step that passes it ends the process):

  kernel        amx_resampler_run alone
  d2h_out       the resampled master to pinned host memory
  d2h_master    the unresampled master to pinned host memory: what a caller copies without
                the key, the yardstick kernel + d2h_out stands against

The kernel's name and time also come from a pass of their own under a kernel-tracing
profiler (--device-only: the kernels alone).  No pass mark: the numbers go to
profiles/resample_bench.json and DESIGN.md 3.12.

    python scripts/resample_bench.py [--seconds 300] [--reps 15]
"""
import argparse
import faulthandler
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-mastering-engine_amd"))
sys.path.insert(0, ROOT)

CASES = [("dynamic_192k_to_48k", 192000, 48000), ("dynamic_192k_to_44k1", 192000, 44100),
         ("linear_48k_to_44k1", 48000, 44100)]
STEP_LIMIT_S = 120


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--device-only", action="store_true", help="the kernels alone, for a profiler pass")
    ap.add_argument("--rev", default=None, help="the revision to record (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    args = ap.parse_args()
    import torch
    from amx import capi
    from amx.resample import Resampler
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    res = {"what": "amx_resampler_run on a stereo master beside the pinned D2H it shortens (HIP events, medians "
                   "of %d after 3 warm-ups)" % args.reps,
           "git": args.rev or git_rev(), "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "cases": {}}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, fi, fo in CASES:
        n = int(args.seconds * fi)
        y = torch.randint(-32768, 32768, (n, 2), dtype=torch.int16, device="cuda", generator=gen)
        rs = Resampler(fi, fo, 2)
        n_out = rs.out_frames(n)
        out = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")

        def kernel():
            capi.check(rs.run(y, out, n_out), "amx_resampler_run")

        r = {"in_rate": fi, "out_rate": fo, "frames": n, "out_frames": n_out, "master_bytes": n * 4,
             "out_bytes": n_out * 4}
        r["kernel"] = timed(kernel, args.reps)
        if not args.device_only:
            h_out = torch.empty((n_out, 2), dtype=torch.int16, pin_memory=True)
            h_y = torch.empty((n, 2), dtype=torch.int16, pin_memory=True)
            r["d2h_out"] = timed(lambda: h_out.copy_(out, non_blocking=True), args.reps)
            r["d2h_master"] = timed(lambda: h_y.copy_(y, non_blocking=True), args.reps)
            r["kernel_plus_d2h_out_ms"] = round(r["kernel"]["median_ms"] + r["d2h_out"]["median_ms"], 4)
            r["saved_ms"] = round(r["d2h_master"]["median_ms"] - r["kernel_plus_d2h_out_ms"], 4)
            del h_out, h_y
        res["cases"][name] = r
        rs.close()
        del y, out
    line = json.dumps(res)
    print(line)
    if not args.device_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
