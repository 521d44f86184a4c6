"""Bit-identity cases for af_loudnorm's frame-by-frame kernel k_ln_dyn<C> (csrc/amx_ln_dyn.hip):
the kernel's int16 output and its 16-word summary on tracks that make it run from end to
end, stereo through amx_loudnorm_192k_ex and C = 3..8 through amx_mc_loudnorm_192k.
tests/test_gpu_ln_dyn_digests.py compares each case's digest with the one recorded in
tests/golden/ln_dyn_digests.json; no oracle is involved.

The signals are tests/test_gpu_dynamic.py's and tests/test_gpu_mc_dynamic.py's, quantised
as ffmpeg does (clip(lrintf(x * 32768))).  Stereo cases carry pass-2 options that keep
above_threshold at 0 (measured_i = the measured input_i + 6, measured_thresh = 0, offset
0), so the parallel form leaves the whole track to k_ln_dyn with r128_out on every frame;
`handover` is test_quiet_start_handover_vs_oracle's case.  C-channel cases run both passes
(`.pass1`: the measured_* defaults; `.pass2`: the pass-1 strings, offset 2.37, on pass 1's
192 kHz stream).

    python tests/ln_dyn_cases.py --write PATH [--rev COMMIT]

records every case's digest (needs a GPU); run it in a checkout of the commit whose
output is to be the reference, with this module copied in.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np

TARGET = -14.0

STEREO = ("never_lifts", "partial_441", "first_burst", "linear_2s", "handover")
MC = ("c3_7p3s", "c6_lfe", "c8_96k", "c6_quiet", "c3_2s")
CASES = STEREO + tuple("%s.pass%d" % (m, p) for m in MC for p in (1, 2))


def quantize(x):
    v = np.rint(np.asarray(x, np.float32) * np.float32(32768.0))
    return np.clip(v, -32768, 32767).astype(np.int16)


def _stereo_signal(name):
    from test_gpu_dynamic import _dynamic_signal
    from test_gpu_mc_dynamic import edge_signal
    if name == "never_lifts":
        return _dynamic_signal(8.0, 48000, 5), 48000
    if name == "partial_441":
        return _dynamic_signal(8.03, 44100, 5), 44100
    if name == "first_burst":
        return edge_signal(8.0, 48000, 2, 5, "start"), 48000
    if name == "linear_2s":
        return _dynamic_signal(2.0, 48000, 5), 48000
    return _dynamic_signal(40.0, 48000, 29, intro=6.0), 48000


def _mc_signal(name):
    from test_gpu_mc_dynamic import mc_signal, single_channel_signal
    if name == "c3_7p3s":
        return mc_signal(7.3, 48000, 3, 23), 48000
    if name == "c6_lfe":
        return single_channel_signal(10.0, 48000, 6, 66, [3, 5, 0]), 48000
    if name == "c8_96k":
        return mc_signal(5.0, 96000, 8, 28), 96000
    if name == "c6_quiet":
        return mc_signal(9.0, 48000, 6, 91, intro=4.0), 48000
    return mc_signal(2.0, 48000, 3, 93), 48000


def _measured(capi, st, measured_i, thresh, offset):
    return capi.LoudnormDesc(TARGET, 11.0, -1.5, measured_i, float(st["input_lra"]), float(st["input_tp"]),
                             thresh, offset)


def _run_stereo(name, signal=None):
    """signal: (float32 [n, 2], rate) in place of the named case's (tests/up192_cases.py)"""
    import torch
    from amx import capi
    from amx.engine import MasteringJob
    x, fs = signal if signal is not None else _stereo_signal(name)
    x16 = quantize(x)
    n = x16.shape[0]
    env = {"AMX_LN_SEG": "4", "AMX_LN_WARM": "3"} if name == "handover" else {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    job = MasteringJob(fs, 2, {"lufs": TARGET}, [n], input_s16=True, chunks=[(0, 0, n)], measure_only=True)
    try:
        job.out[:n].copy_(torch.from_numpy(x16))
        job.loudness_pass1(tail=False)
        job.loudness_pass2(carry=False)
        job.histograms()
        job.decide()
        st = job.fetch_report(raise_dynamic=False)["stats"][0]
        n192, job2, ws2, summ = job._job192(0, cached=False)[0:4]
        if name == "handover":
            d = _measured(capi, st, float(st["input_i"]), float(st["input_thresh"]), 8.0)
        else:
            d = _measured(capi, st, float(st["input_i"]) + 6.00, 0.00, 0.0)
        summ.zero_()
        job.loudnorm_192k(0, d, job2, ws2, summ)
        y, s = job2.out[:n192].cpu().numpy(), summ.cpu().numpy()
        job2.close()
    finally:
        job.close()
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return {name: (y, s)}


def _run_mc(name):
    import torch
    from amx import capi
    from amx.engine import MultiChannelJob
    x, fs = _mc_signal(name)
    x16 = quantize(x)
    n, C = x16.shape
    job = MultiChannelJob(fs, C, {"lufs": TARGET}, n, input_s16=True, chunks=[(0, 0, n)])
    try:
        job.out[:n].copy_(torch.from_numpy(x16))
        job.measure(lufs_on=True)
        st = job.fetch_report(raise_dynamic=False)["stats"][0]
        side = job._side192()
        d1 = capi.LoudnormDesc(TARGET, 11.0, -1.5, 0.0, 0.0, 99.0, -70.0, 0.0)
        d2 = _measured(capi, st, float(st["input_i"]), float(st["input_thresh"]), 2.37)
        d2.reuse_stream = 1
        out = {}
        for p, d in ((1, d1), (2, d2)):
            job.dyn_filter(d)
            out["%s.pass%d" % (name, p)] = (side.y192[:side.n192].cpu().numpy(), side.summ.cpu().numpy())
    finally:
        job.close()
    return out


@functools.lru_cache(maxsize=None)
def _run(base):
    return _run_stereo(base) if base in STEREO else _run_mc(base)


def run_case(name):
    """(int16 [n192, C] the kernel's output, float64 [16] its summary)"""
    return _run(name.split(".")[0])[name]


def digest(y, summary):
    return {"sha256": hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest(), "frames": int(y.shape[0]),
            "summary01": [float(summary[0]).hex(), float(summary[1]).hex()]}


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", required=True)
    ap.add_argument("--rev", default=None, help="the commit this checkout is at")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "audio-mastering-engine_amd"))
    doc = {"what": "k_ln_dyn's output per case of tests/ln_dyn_cases.py: SHA-256 of the int16 bytes, summary "
                   "words 0-1 (float.hex)",
           "recorded_at_commit": args.rev,
           "regenerate": "in a checkout of that commit, with tests/ln_dyn_cases.py copied in, on an MI355X: "
                         "python tests/ln_dyn_cases.py --write tests/golden/ln_dyn_digests.json --rev COMMIT",
           "cases": {}}
    for name in CASES:
        y, s = run_case(name)
        doc["cases"][name] = digest(y, s)
        print(name, doc["cases"][name], "summary", [float(v) for v in s[:2]], s[7], s[12], s[14], flush=True)
    with open(args.write, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
