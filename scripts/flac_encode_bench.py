"""Time the device FLAC encoder (amx_flac_encode) beside the copy it replaces.

Two masters of the C3 programme (bench.py's default synthetic input, seed 0):
  c3      the 5-minute stereo 48 kHz master (14.4 M frames), the linear ending
  dyn192  the same programme made to take loudnorm's dynamic mode: a 57.6 M-frame stereo
          192 kHz master (bench.py's --input dynamic)
and for each, with HIP events after warm-up, the median of --reps runs of
  encode    amx_flac_encode on preallocated buffers (its three kernels)
  d2h_raw   the int16 master into pinned host memory: the cost of today's WAV ending
  d2h_flac  the encoded bytes into pinned host memory
plus the compression ratio and, on the host clock, hashlib.md5 over the raw PCM (what
write_flac(md5=True) adds: it also needs the raw copy).  No pass mark: the numbers go to
profiles/flac_encode_bench.json and DESIGN.md 3.10.

--lpc-order takes one order or a comma-separated list (amx_flac_encode_ex; 0 is the
FIXED-only encoder): "masters" holds the first order's numbers, "masters_lpcN" those of every
further order N, measured on the same masters in the same process
(profiles/flac_lpc_bench.json).

    python scripts/flac_encode_bench.py [--seconds 300] [--reps 15] [--block 4096] [--lpc-order 0,4,8]
"""
import argparse
import ctypes
import hashlib
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


def masters(seconds):
    """{name: (int16 device tensor [frames, 2], sample rate)}"""
    import torch
    import bench
    from amx.engine import MasteringJob
    fs = 48000
    n = int(seconds * fs)
    out = {}
    for name, kind in (("c3", "mix"), ("dyn192", "dynamic")):
        x = bench.synth_input(n, fs, 0, kind)
        job = MasteringJob(fs, 2, bench.C3, [n])
        y = job.run(torch.from_numpy(x).cuda())
        rep = job.fetch_report(raise_dynamic=False)
        mode = rep["modes"][0]
        if mode == "dynamic":
            y, info = job.dynamic_track(0, rep["stats"][0])
            rate = info["sample_rate"]
        else:
            rate = fs
        assert (mode == "dynamic") == (name == "dyn192"), (name, mode)
        out[name] = (y.clone(), rate)
        del job
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return out


def timed(fn, reps, warmup=3):
    """median / min / max ms of fn() by device events"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def measure(y, rate, block, reps, lpc_order=0):
    import torch
    from amx import capi, flacio
    L = capi.load()
    frames, C = int(y.shape[0]), int(y.shape[1])
    nf, cap, wsb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    capi.check(L.amx_flac_encode_size_ex(frames, C, block, lpc_order, ctypes.byref(nf), ctypes.byref(cap),
                                         ctypes.byref(wsb)), "amx_flac_encode_size_ex")
    out = torch.empty(cap.value, dtype=torch.uint8, device="cuda")
    fb = torch.empty(nf.value, dtype=torch.int32, device="cuda")
    total = torch.empty(1, dtype=torch.int64, device="cuda")
    ws = torch.empty((wsb.value + 7) // 8, dtype=torch.int64, device="cuda")

    def encode():
        capi.check(L.amx_flac_encode_ex(capi.ptr(y), frames, C, rate, block, lpc_order, capi.ptr(out), cap.value,
                                        capi.ptr(fb), None, capi.ptr(total), capi.ptr(ws), ws.numel() * 8,
                                        capi.ptr_stream()), "amx_flac_encode_ex")

    r = {"frames": frames, "channels": C, "sample_rate": rate, "block": block, "flac_frames": nf.value,
         "lpc_order": lpc_order}
    r["encode"] = timed(encode, reps)
    n_enc = int(total.item())
    raw_bytes = frames * C * 2
    h_raw = torch.empty((frames, C), dtype=torch.int16).pin_memory()
    h_enc = torch.empty(n_enc, dtype=torch.uint8).pin_memory()
    r["d2h_raw"] = timed(lambda: h_raw.copy_(y, non_blocking=True), reps)
    r["d2h_flac"] = timed(lambda: h_enc.copy_(out[:n_enc], non_blocking=True), reps)
    r["raw_bytes"], r["flac_bytes"] = raw_bytes, n_enc
    r["ratio"] = round(n_enc / raw_bytes, 4)
    raw = h_raw.numpy()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        digest = hashlib.md5(raw.data).digest()
        t.append((time.perf_counter() - t0) * 1e3)
    r["host_md5_ms"] = round(min(t), 2)
    # the stream is real: it decodes to the master, and STREAMINFO's MD5 is the hash above
    data = flacio.flac_container(h_enc.numpy().tobytes(), fb.cpu().numpy(), rate, C, frames, block, digest)
    got, _ = flacio.decode_flac(data)
    r["decodes_to_master"] = bool(((got >> 16) == raw).all())
    # the endings, from the medians: today's WAV ending moves the raw PCM; the FLAC ending
    # encodes and moves the stream, and with md5 also moves and hashes the raw PCM
    wav = r["d2h_raw"]["median_ms"]
    fl = r["encode"]["median_ms"] + r["d2h_flac"]["median_ms"]
    r["ending_ms"] = {"wav": round(wav, 3), "flac_md5_off": round(fl, 3),
                      "flac_md5_on": round(fl + wav + r["host_md5_ms"], 3)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--lpc-order", default=[0], type=lambda s: [int(v) for v in s.split(",")],
                    help="LPC order 0..8, or a comma-separated list of orders")
    ap.add_argument("--rev", default=None, help="the revision to record (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_encode_bench.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "flac_encode_bench needs a GPU"
    res = {"what": "amx_flac_encode vs the pinned D2H of the raw int16 master (HIP events, medians of %d)" % args.reps,
           "git": args.rev or git_rev(), "device": torch.cuda.get_device_name(0), "seconds": args.seconds,
           "masters": {}}
    for name, (y, rate) in masters(args.seconds).items():
        for i, order in enumerate(args.lpc_order):
            res.setdefault("masters" if i == 0 else "masters_lpc%d" % order, {})[name] = \
                measure(y, rate, args.block, args.reps, order)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
