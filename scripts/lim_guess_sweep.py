"""Sweep of scripts/lim_guess_model.c over tests/limiter_cases.py's signals: how often is a
segment's guessed start state equal to the true one in its scalars but not in its live list
(the case the walker's list comparison exists for), and does `d <= delta` in place of
`d < delta` ever change the attenuation trace?  CPU only.

    python scripts/lim_guess_sweep.py [sets, comma separated] [seeds: 1 .. N-1]

Prints the totals and the first hits.  First checks the model's trace against the oracle's."""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "audio-mastering-engine_amd")]
import numpy as np      # noqa: E402
import limiter_cases as lc      # noqa: E402
import oracle as O      # noqa: E402

_so = os.path.join(tempfile.mkdtemp(), "lim_guess_model.so")
subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-o", _so,
                       os.path.join(ROOT, "scripts", "lim_guess_model.c"), "-lm"])
L = ctypes.CDLL(_so)


def check_model():
    bad = 0
    for pname in lc.A_SETS:
        P = lc.PARAMS[pname]
        for sig in lc.SIGNALS:
            x = np.ascontiguousarray(lc.signal(sig, 20000, 44100, P, seed=3))
            att = np.zeros(20000)
            L.trace(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(20000), 44100, ctypes.c_double(P["level_in"]),
                    ctypes.c_double(P["limit"]), ctypes.c_double(P["attack"]), ctypes.c_double(P["release"]),
                    att.ctypes.data_as(ctypes.c_void_p))
            bad += int((att.view(np.int64) != lc.reference(O, x, 44100, P)[1].view(np.int64)).any())
    assert bad == 0, "%d model traces differ from the oracle's" % bad


check_model()


def run(x, fs, P, LS, W):
    out = (ctypes.c_int64 * 6)()
    x = np.ascontiguousarray(x)
    L.sweep(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(x.shape[0]), fs, ctypes.c_double(P['level_in']), ctypes.c_double(P['limit']),
            ctypes.c_double(P['attack']), ctypes.c_double(P['release']), LS, W, out)
    return np.array(list(out))
tot = np.zeros(6, np.int64); hits = []; t0 = time.time(); runs = 0
sets = sys.argv[1].split(',') if len(sys.argv) > 1 else ['ref', 'half', 'att0.7', 'levels', 'unit-edge', 'att20-rel1']
for seed in range(1, int(sys.argv[2]) if len(sys.argv) > 2 else 40):
    for pname in sets:
        P = lc.PARAMS[pname]
        for fs in (8000, 44100, 48000):
            B = lc.ring_frames(fs, P)
            if B < 2: continue
            for sig in lc.SIGNALS:
                x = lc.signal(sig, 20000, fs, P, seed=seed)
                for LS in (max(64, B), 256 if B <= 256 else 2 * B, 1000 if B <= 1000 else 3 * B):
                    for W in (0, 1, 7, B // 2, B - 1, B, B + 1, 2 * B, 3 * B + 17):
                        r = run(x, fs, P, LS, W); tot += r; runs += 1
                        if r[2] or r[4]: hits.append((seed, pname, fs, sig, LS, W, r.tolist()))
print('runs', runs, 'totals [guesses, scalars differ, scalars equal lists differ, equal, le-trace diff frames, d==delta events]', tot.tolist(), '%.0fs' % (time.time() - t0))
for h in hits[:40]: print(h)
print(len(hits), 'hits')
