"""Time master_files against a loop of master_audio over the same settings dicts
(DESIGN.md 3.13): the file-to-file rate of the product's entry points.

Input: --files (8) WAV files of --seconds (300) of 48 kHz stereo s16 (C4's programme,
synth.mix_tiled, one seed per file) in a temporary directory, whose filesystem is recorded.
Two lists of jobs over them, one with *.wav and one with *.flac outputs, both with C3's
settings (tests/test_gpu_dropin.py) and lufs = -14.

Yardstick: `for job in jobs: master_audio(job)` in the same process -- what a caller
has to do without master_files.  Method: one warm-up of each side, then --reps (5)
alternating repetitions on the host clock with the device drained before and after; the
medians and each side's spread (max - min) are reported, and "faster" means the medians
differ by more than the loop's own spread.  The warm-up's output files of both sides are
compared byte for byte before anything is timed.

Split (master_files only): perf_counter sums per stage -- header, read (summed over the
reader threads), stage (the calling thread's H2D enqueue and conversion launch), d2h (its
wait for the D2H events), md5 and write (summed over the writer threads) -- and the device
stage by HIP events.  The thread sums overlap each other and the device stage, so they do
not add up to the wall time: the stage whose sum divided by its threads comes closest to
the wall time bounds the call.

    python scripts/master_files_bench.py [--files 8] [--seconds 300] [--reps 5] [--workers 8]
                                         [--dir DIR] [--out profiles/master_files_bench.json]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-mastering-engine_amd"))
sys.path.insert(0, ROOT)

MB = dict(multiband=True, low_thresh=-25.0, low_ratio=6.0, mid_thresh=-20.0, mid_ratio=3.0,
          high_thresh=-15.0, high_ratio=4.0)
C3 = dict(bass_boost=-1.0, mid_cut=2.0, presence_boost=2.5, treble_boost=1.0, lufs=-14.0,
          width=1.3, analog_character=40.0, **MB)


def git_rev():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                              text=True, check=True).stdout.strip()
    except Exception:   # noqa: BLE001 -- a tree without git metadata
        return None


def filesystem_of(path):
    """(mount point, type) of the filesystem holding path, from /proc/mounts"""
    path = os.path.realpath(path)
    best = ("", "unknown")
    try:
        with open("/proc/mounts") as f:
            for line in f:
                parts = line.split()
                if len(parts) >= 3 and (path == parts[1] or path.startswith(parts[1].rstrip("/") + "/")):
                    if len(parts[1]) >= len(best[0]):
                        best = (parts[1], parts[2])
    except OSError:
        pass
    return {"mount": best[0], "type": best[1]}


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
            "spread_ms": round(max(ms) - min(ms), 2), "runs_ms": [round(v, 2) for v in ms]}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--dir", default=None, help="where the temporary directory is made")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "master_files_bench.json"))
    a = ap.parse_args()
    if not 1 <= a.workers <= 16:
        ap.error("--workers must be in 1..16")
    import numpy as np
    import torch
    import audio_mastering_engine as ame
    from amx import files, synth, wavio
    fs = 48000
    n = int(fs * a.seconds)
    tmp = tempfile.mkdtemp(prefix="amx_files_bench_", dir=a.dir)
    result = {"git": git_rev(), "device": torch.cuda.get_device_name(0), "files": a.files, "seconds": a.seconds,
              "sample_rate": fs, "workers": a.workers, "reps": a.reps, "filesystem": filesystem_of(tmp),
              "settings": "C3 (tests/test_gpu_dropin.py), lufs -14", "lists": {}}
    try:
        t0 = time.perf_counter()
        inputs = []
        for k in range(a.files):
            x = synth.mix_tiled(n, fs, 2, seed=k)
            p = os.path.join(tmp, "in_%d.wav" % k)
            wavio.write_wav_pcm(p, np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16), fs, "s16")
            inputs.append(p)
        result["input_seconds_to_make"] = round(time.perf_counter() - t0, 2)
        result["input_bytes_each"] = os.path.getsize(inputs[0])
        for ext in ("wav", "flac"):
            def jobs(side):
                d = os.path.join(tmp, "%s_%s" % (side, ext))
                os.makedirs(d, exist_ok=True)
                return [dict(C3, input_file=p, output_file=os.path.join(d, "m_%d.%s" % (k, ext)))
                        for k, p in enumerate(inputs)]
            loop_jobs, batch_jobs = jobs("loop"), jobs("batch")

            def loop():
                for job in loop_jobs:
                    ame.master_audio(job)

            def batch(split=None):
                res = files.master_files(ame, batch_jobs, workers=a.workers, _times=split)
                bad = [r for r in res if r["error"] is not None]
                if bad:
                    raise bad[0]["error"]
                return res
            # warm-up of each side, and the contract on these very files
            timed(loop)
            _, res = timed(batch)
            for lj, bj in zip(loop_jobs, batch_jobs):
                with open(lj["output_file"], "rb") as f, open(bj["output_file"], "rb") as g:
                    if f.read() != g.read():
                        raise SystemExit("master_files' %s differs from master_audio's" % bj["output_file"])
            t_loop, t_batch, splits = [], [], []
            for _ in range(a.reps):
                t_loop.append(timed(loop)[0])
                split = {}
                t_batch.append(timed(lambda: batch(split))[0])
                splits.append(split)
            sl, sb = stats(t_loop), stats(t_batch)
            keys = ("header", "read", "stage", "d2h_enqueue", "d2h", "md5", "write", "device_events_ms")
            med = {}
            for k in keys:
                v = [s.get(k, 0.0) * (1.0 if k.endswith("_ms") else 1e3) for s in splits]
                med[k if k.endswith("_ms") else k + "_ms"] = round(statistics.median(v), 2)
            ratio = sl["median_ms"] / sb["median_ms"]
            diff = abs(sl["median_ms"] - sb["median_ms"])
            result["lists"][ext] = {
                "master_audio_loop": sl, "master_files": sb, "ratio_loop_over_master_files": round(ratio, 3),
                "faster": bool(sb["median_ms"] < sl["median_ms"] and diff > sl["spread_ms"]),
                "groups": sorted({r["group"] for r in res}), "modes": [r["mode"] for r in res],
                "output_bytes_each": os.path.getsize(batch_jobs[0]["output_file"]),
                "stage_sums_median": med, "staging_peak_bytes": list(splits[-1].get("staging_peak", (0, 0)))}
            print(ext, json.dumps(result["lists"][ext]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
