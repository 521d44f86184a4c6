"""Time a FLAC input's way to the chain's s16 frames: the host decoder and its upload
beside the device decoder (amx_flac_decode_device).

The input is the C3 programme (bench.py's default synthetic input, seed 0: 5 minutes of
stereo 48 kHz, 14.4 M frames) as int16, encoded by the device encoder at each --lpc-order.
Both legs run in the same process, medians of --reps runs after 3 warm-ups, on the host
clock from the file's bytes in memory to a finished stream (the legs hold host work):

  (a) host    decode_flac at --threads threads + raw.copy() + the pageable .to("cuda") +
              amx_pcm_to_s16: what _device_input does without flac_decode = "device"
  (b) device  decode_flac_device (scan, the pinned staging copy, one H2D, three kernels, the
              result read-back) + amx_pcm_to_s16: what it does with it

and (b) once more in pieces: the host scan and the staging copy on the host clock; the H2D,
the three kernels together and amx_pcm_to_s16 by HIP events.  The kernels' own times come
from a separate pass under a kernel-tracing profiler (--device-only keeps that pass to leg
(b)).  Both legs' s16 frames are compared before anything is timed.  No pass mark: the
numbers go to profiles/flac_decode_bench.json and DESIGN.md 3.11.

    python scripts/flac_decode_bench.py [--seconds 300] [--reps 15] [--lpc-order 0,8] [--threads 16]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-mastering-engine_amd"))
sys.path.insert(0, ROOT)


def git_rev():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                              text=True, check=True).stdout.strip()
    except Exception:   # noqa: BLE001 -- a tree without git metadata
        return None


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def wall(fn, reps, warmup=3):
    """host-clock ms of fn() with the device drained before and after"""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def to_s16(d_raw, frames, channels):
    import torch
    from amx import capi
    d_in = torch.empty((max(1, frames), 2), dtype=torch.int16, device="cuda")
    capi.check(capi.load().amx_pcm_to_s16(capi.ptr(d_raw), frames, channels, capi.PCM_FORMATS["s32"], capi.ptr(d_in),
                                          capi.ptr_stream()), "amx_pcm_to_s16")
    return d_in


def leg_host(data, threads):
    import torch
    from amx import flacio
    x, info = flacio.decode_flac(data, threads=threads)
    raw = x.view("uint8").reshape(-1)
    d_raw = torch.from_numpy(raw.copy()).to("cuda")
    return to_s16(d_raw, x.shape[0], info.channels)


def leg_device(data):
    from amx import flacio
    x, info, _ = flacio.decode_flac_device(data)
    return to_s16(x, int(x.shape[0]), info.channels)


def pieces(data, reps, warmup=3):
    """leg (b) step by step on preallocated buffers"""
    import numpy as np
    import torch
    from amx import capi, flacio
    L = capi.load()
    raw = np.frombuffer(data, np.uint8)
    size = raw.size
    rec = ctypes.sizeof(capi.FlacCand)
    t_off = (size + 15) & ~15
    stage = torch.empty(t_off + (size // 256 + 1024) * rec, dtype=torch.uint8, pin_memory=True)
    h = stage.numpy()
    rc, sc, tab = flacio.flac_scan(raw, room=h[t_off:])
    assert rc == capi.AMX_OK and tab.ctypes.data == h.ctypes.data + t_off
    n_up = t_off + tab.size
    d_all = torch.empty(n_up, dtype=torch.uint8, device="cuda")
    out = torch.empty((sc.total_frames, sc.channels), dtype=torch.int32, device="cuda")
    d_blocks = torch.empty(sc.n_cand, dtype=torch.int32, device="cuda")
    d_res = torch.empty(4, dtype=torch.int64, device="cuda")
    ws = torch.empty((sc.workspace_bytes + 15) // 16 * 2, dtype=torch.int64, device="cuda")
    d_s16 = torch.empty((sc.total_frames, 2), dtype=torch.int16, device="cuda")
    t = {k: [] for k in ("scan_host", "stage_copy_host", "h2d", "decode_kernels", "pcm_to_s16")}
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        h[:size] = raw
        t1 = time.perf_counter()
        rc, sc, tab = flacio.flac_scan(h[:size], room=h[t_off:])
        t2 = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        d_all.copy_(stage[:n_up], non_blocking=True)
        ev[1].record()
        capi.check(L.amx_flac_decode_device(capi.ptr(d_all), size, capi.ptr(d_all[t_off:]), ctypes.byref(sc),
                                            capi.ptr(out), sc.total_frames, capi.ptr(d_blocks), sc.n_cand,
                                            capi.ptr(d_res), capi.ptr(ws), ws.numel() * 8, capi.ptr_stream()),
                   "amx_flac_decode_device")
        ev[2].record()
        capi.check(L.amx_pcm_to_s16(capi.ptr(out), sc.total_frames, sc.channels, capi.PCM_FORMATS["s32"],
                                    capi.ptr(d_s16), capi.ptr_stream()), "amx_pcm_to_s16")
        ev[3].record()
        ev[3].synchronize()
        assert int(d_res[0]) == capi.AMX_OK
        if i >= warmup:
            t["stage_copy_host"].append((t1 - t0) * 1e3)
            t["scan_host"].append((t2 - t1) * 1e3)
            t["h2d"].append(ev[0].elapsed_time(ev[1]))
            t["decode_kernels"].append(ev[1].elapsed_time(ev[2]))
            t["pcm_to_s16"].append(ev[2].elapsed_time(ev[3]))
    r = {k: stats(v) for k, v in t.items()}
    r.update(candidates=int(sc.n_cand), flac_frames=int(d_res[2]), scratch_bytes=int(sc.scratch_samples) * 4,
             workspace_bytes=int(sc.workspace_bytes), upload_bytes=int(n_up))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--lpc-order", default=[0, 8], type=lambda s: [int(v) for v in s.split(",")])
    ap.add_argument("--device-only", action="store_true", help="leg (b) alone, for a profiler pass")
    ap.add_argument("--rev", default=None, help="the revision to record (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_decode_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from amx import flacio
    assert torch.cuda.is_available(), "flac_decode_bench needs a GPU"
    fs = 48000
    n = int(args.seconds * fs)
    x = bench.synth_input(n, fs, 0, "mix")
    x16 = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    res = {"what": "a FLAC input to s16 frames on the device: host decoder + upload vs amx_flac_decode_device "
                   "(host clock, medians of %d)" % args.reps,
           "git": args.rev or git_rev(), "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "threads": args.threads, "block": args.block, "streams": {}}
    for order in args.lpc_order:
        data = flacio.flac_bytes(x16, fs, block=args.block, md5=False, lpc_order=order)
        r = {"frames": n, "file_bytes": len(data), "decoded_bytes": n * 2 * 4, "lpc_order": order}
        if args.device_only:
            for _ in range(args.reps):
                leg_device(data)
            torch.cuda.synchronize()
        else:
            a, b = leg_host(data, args.threads), leg_device(data)
            r["legs_equal"] = bool(torch.equal(a, b)) and bool(torch.equal(a.cpu(), torch.from_numpy(x16)))
            del a, b
            r["host_leg"] = wall(lambda: leg_host(data, args.threads), args.reps)
            r["device_leg"] = wall(lambda: leg_device(data), args.reps)
            r["device_pieces"] = pieces(data, args.reps)
            r["speedup"] = round(r["host_leg"]["median_ms"] / r["device_leg"]["median_ms"], 2)
        res["streams"]["lpc%d" % order] = r
    line = json.dumps(res)
    print(line)
    if not args.device_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
