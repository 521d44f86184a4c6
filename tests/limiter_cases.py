"""Signals, parameter sets and cases for the stereo gain and limiter stage (k_final<UNIT>,
csrc/amx_final.hip): tests/test_gpu_final_stage.py runs them on the GPU one stage at a time,
tests/test_limiter_cases.py asserts their preconditions on the CPU, from the oracle's output
and attenuation trace alone (oracle.alimiter(..., trace=True)).

Every signal is int16 [n, 2], seeded, and built around ``thr``: the raw sample magnitude (in
LSB, a float) above which a sample is over the limit once the gain and level_in are applied,
limit * 32768 / (level_in * gain).  Over-limit magnitudes are thr times a factor > 1, capped
at 32768; a magnitude of 32768 exists only as -32768, so at a limit next to full scale the
over-limit samples are all negative.

Groups (the letters of the test ids):
  A  the general limiter over parameter sets, rates, signals and gains
  B  segments, warm-ups and the walker
  C  the idle path (final_fast_block) on inputs that never reach the limit
  D  spans that start inside a track (halo and carried state)
"""
import numpy as np

RATES = (8000, 11025, 22050, 44100, 48000, 88200, 96000, 176400, 192000, 384000)
SIGNALS = ("bursts", "am", "square", "impulses", "equal_peaks", "ramp_up", "ramp_down", "full_scale")

REF = dict(level_in=1.0, level_out=1.0, limit=0.98, attack=5.0, release=50.0, auto_level=True)


def _p(**kw):
    d = dict(REF)
    d.update(kw)
    return d


# the oracle's keyword arguments per set; "limit-exact" is group C's (32112 / 32768 is exact)
PARAMS = {
    "ref": _p(),
    "half": _p(limit=0.5, attack=1.0, release=10.0),
    "att0.7": _p(attack=0.7),
    "att20-rel1": _p(attack=20.0, release=1.0),
    "rel500": _p(release=500.0),
    "levels": _p(level_in=2.0, level_out=0.5, limit=0.9, auto_level=False),
    "unit-edge": _p(limit=32767.0 / 32768.0),
    "unit-over": _p(limit=float(np.nextafter(32767.0 / 32768.0, 2.0))),
    "lim1-in1.5": _p(limit=1.0, level_in=1.5),
    "limit-exact": _p(limit=32112.0 / 32768.0),
}
A_SETS = ("ref", "half", "att0.7", "att20-rel1", "rel500", "levels", "unit-edge", "unit-over", "lim1-in1.5")
GAINS = {"off": -1.0, "1.0": 1.0, "0.5": 0.5, "-3.2dB": 10.0 ** (-3.2 / 20.0), "1.7": 1.7}


def ring_frames(fs, params):
    """B: af_alimiter's look-ahead ring in frames (config_input, two channels)"""
    attack = params["attack"] / 1000.0
    bs = int(fs * attack * 2)
    bs -= bs % 2
    return bs // 2


def is_unit(params):
    """launch_final's choice of k_final<true>"""
    return params["level_in"] == 1.0 and params["level_out"] == 1.0 and params["limit"] * 32768.0 <= 32767.0


def threshold(params, gain=-1.0):
    return params["limit"] * 32768.0 / (params["level_in"] * (gain if gain > 0 else 1.0))


def can_engage(params, gain=-1.0):
    """whether any int16 input is over the limit after the gain stage (which clips) and level_in"""
    top = 32768.0 if gain <= 0 else min(32768.0, float(np.rint(32768.0 * gain)))
    return (top * (1.0 / 32768.0)) * params["level_in"] > params["limit"]


def reference(O, x16, fs, params, gain=-1.0, trace=True):
    """the oracle on the gained signal: (y, att)"""
    g16 = O.linear_gain(x16, gain) if gain > 0 else x16
    return O.alimiter(g16, fs, trace=trace, **params)


# ------------------------------------------------------------------------------ signals
def _over(thr, f):
    """an over-limit magnitude: about f * thr (f > 1), at least one step over thr, at most 32768"""
    m = int(np.ceil(f * thr))
    if m <= thr:
        m += 1
    return min(m, 32768)


def _signed(mag, sign):
    """mag * sign as int16 values; a magnitude of 32768 only exists as -32768"""
    mag = np.minimum(np.asarray(mag, np.int64), 32768)
    v = mag * np.asarray(sign, np.int64)
    return np.where(mag >= 32768, -32768, v)


def _s16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _bed(n, fs, thr, rng, level=0.25):
    """quiet 'music': two sines per channel and a little noise, peaks under 0.3 thr"""
    t = np.arange(n)[:, None] / float(fs)
    c = np.arange(2)[None, :]
    ph = rng.uniform(0, 2 * np.pi, (1, 2))
    x = level * thr * (0.7 * np.sin(2 * np.pi * (220 + 111 * c) * t + ph) + 0.3 * np.sin(2 * np.pi * (1370 + 90 * c) * t))
    return x + rng.integers(-2, 3, (n, 2)) * max(1.0, 0.01 * thr) / 2.0


def _gap(rng, fs, rest, lo_ms=1.0, hi_ms=30.0):
    """frames between two events: mostly short, three in ten long enough for the limiter to rest"""
    if rng.random() < 0.3:
        return int(rest * rng.uniform(1.3, 2.2))
    return int(rng.integers(max(1, int(lo_ms * fs / 1000)), max(2, int(hi_ms * fs / 1000)) + 1))


def _bursts(n, fs, B, thr, rest, rng):
    x = _bed(n, fs, thr, rng)
    f = int(rng.integers(0, 20))
    while f < n:
        m = int(rng.integers(max(1, int(0.002 * fs)), int(0.04 * fs) + 1))
        v = int(_signed(_over(thr, rng.uniform(1.02, 2.0)), 1 if rng.random() < 0.5 else -1))
        ch = int(rng.integers(0, 3))
        if ch == 2:
            x[f:f + m] = v
        else:
            x[f:f + m, ch] = v
        f += m + _gap(rng, fs, rest)
    return _s16(x)


def _am(n, fs, B, thr, rest, rng):
    t = np.arange(n)[:, None] / float(fs)
    c = np.arange(2)[None, :]
    # both channels share the slow swing (so the limiter rests once a period); frame 0 is over
    a = thr * (0.97 + 0.06 * np.sin(2 * np.pi * 3.1 * t + 1.0 + 0.3 * c) + 0.05 * np.sin(2 * np.pi * (41 + 6 * c) * t))
    return _s16(a * np.sin(2 * np.pi * (197 + 61 * c) * t + np.pi / 2 - 0.2 * c))


def _square(n, fs, B, thr, rest, rng):
    s = np.where(np.sin(2 * np.pi * 997.0 * np.arange(n) / float(fs)) >= 0, 1, -1)
    x = np.stack([_signed(_over(thr, 1.25), s), _signed(_over(thr, 1.05), -s)], axis=1)
    return x.astype(np.int16)


def _impulses(n, fs, B, thr, rest, rng):
    a = max(1, int(0.03 * thr))
    x = rng.integers(-a, a + 1, (n, 2)).astype(np.int64)

    def put(f):
        if f < n:
            x[f, int(rng.integers(0, 2))] = _signed(_over(thr, rng.uniform(1.02, 1.4)), 1 if rng.random() < 0.5 else -1)

    f, k = int(rng.integers(0, B + 1)), 0
    while f < n:
        sp = (B - 1, B, B + 1, 0, 0)[k % 5]          # pairs B - 1, B, B + 1 apart, then two singles
        put(f)
        if sp > 0:
            put(f + sp)
        f += sp + int(rng.integers(B // 2 + 2, 2 * B + 4))
        k += 1
    return x.astype(np.int16)


def _equal_peaks(n, fs, B, thr, rest, rng):
    x = rng.integers(-3, 4, (n, 2)).astype(np.int64)
    f, k = int(rng.integers(0, B + 1)), 0
    while f < n:
        m = int(rng.integers(B // 2 + 1, 3 * B + 3))
        i = np.arange(f, min(n, f + m))
        mag = _over(thr, (1.2, 1.45)[k % 2])
        x[i, i & 1] = _signed(mag, np.where((i >> 1) & 1, 1, -1))
        f += m + (int(rest * rng.uniform(1.3, 2.2)) if rng.random() < 0.3 else int(rng.integers(B // 4 + 1, 2 * B + 2)))
        k += 1
    return x.astype(np.int16)


def _ramps(n, fs, B, thr, rest, rng, down):
    """negative peaks from just under thr to 1.6 thr (at most 32768): fast ramps (a few rings
    long, a step or more every frame where the range allows it) and slow ones (1.5 releases:
    slower than the release slope, so the pending-peak list grows by an entry per new peak),
    concave and convex in turn"""
    x = rng.integers(-3, 4, (n, 2)).astype(np.int64)
    lo, hi = int(0.995 * thr), min(int(np.ceil(1.6 * thr)), 32768)
    f, j = int(rng.integers(0, B + 1)), 0
    while f < n:
        m = max(280, B + 40) if j % 2 == 0 else max(300, int(1.5 * rest))
        u = (np.arange(m) / float(m)) ** ((0.5, 2.0)[(j // 2) % 2])
        mag = np.rint(lo + (hi - lo) * u).astype(np.int64)
        if hi - lo >= 2 * m:
            k = np.arange(m)
            mag = np.maximum.accumulate(mag - k) + k      # strictly increasing
        if down:
            mag = mag[::-1]
        i = np.arange(f, min(n, f + m))
        x[i, j % 2] = _signed(mag[:i.size], -1)
        f += m + (int(rest * rng.uniform(1.3, 2.2)) if rng.random() < 0.3 else int(rng.integers(B // 2 + 1, 2 * B + 2)))
        j += 1
    return x.astype(np.int16)


def _full_scale(n, fs, B, thr, rest, rng):
    return np.where(rng.random((n, 2)) < 0.5, -32768, 32767).astype(np.int16)


_MAKE = dict(bursts=_bursts, am=_am, square=_square, impulses=_impulses, equal_peaks=_equal_peaks,
             ramp_up=lambda *a: _ramps(*a, down=False), ramp_down=lambda *a: _ramps(*a, down=True),
             full_scale=_full_scale)


def signal(name, n, fs, params, gain=-1.0, seed=0):
    """int16 [n, 2]: the named signal for a parameter set and gain"""
    B = ring_frames(fs, params)
    rest = int(fs * (params["release"] + params["attack"]) / 1000.0) + 1
    rng = np.random.default_rng([seed, SIGNALS.index(name), fs])
    return _MAKE[name](int(n), fs, B, threshold(params, gain), rest, rng)


def allowed_range(O, params, gain=-1.0):
    """(lo, hi): the raw int16 values whose gained sample is at or under the limit"""
    v = np.arange(-32768, 32768).astype(np.int16)
    g = O.linear_gain(v, gain) if gain > 0 else v
    ok = np.abs((g.astype(np.float64) * (1.0 / 32768.0)) * params["level_in"]) <= params["limit"]
    idx = np.nonzero(ok)[0]
    assert ok[idx[0]:idx[-1] + 1].all()
    return int(v[idx[0]]), int(v[idx[-1]])


def quiet(n, fs, lo, hi, seed, top=None):
    """a signal inside [lo, hi] that touches both ends (first and last frame included); top:
    the largest positive value instead of hi"""
    rng = np.random.default_rng([seed, n, fs])
    hi = hi if top is None else top
    t = np.arange(n)[:, None] / float(fs)
    c = np.arange(2)[None, :]
    x = 0.6 * hi * np.sin(2 * np.pi * (311 + 97 * c) * t + c) + rng.integers(-hi // 3, hi // 3 + 1, (n, 2))
    x = np.clip(np.rint(x), lo, hi).astype(np.int16)
    k = rng.integers(0, n, 6)
    x[k[:3], 0] = hi
    x[k[3:], 1] = lo if top is None else -hi
    x[0] = (lo if top is None else -hi, hi)
    x[n - 1] = (hi, lo if top is None else -hi)
    return x


# ------------------------------------------------------------------------------ group A
def a_length(fs, params):
    return max(12 * ring_frames(fs, params), 4096)


def a_cases():
    """[(signal, set, fs, gain name)]: every signal x set at 44.1 and 48 kHz, bursts and am x
    three sets at every rate, every gain x two sets on bursts and full_scale at 48 kHz"""
    out = []

    def add(*c):
        if c not in out:
            out.append(c)

    for fs in (44100, 48000):
        for s in SIGNALS:
            for p in A_SETS:
                add(s, p, fs, "off")
    for fs in RATES:
        for s in ("bursts", "am"):
            for p in ("ref", "half", "levels"):
                add(s, p, fs, "off")
    for g in GAINS:
        for p in ("ref", "levels"):
            for s in ("bursts", "full_scale"):
                add(s, p, 48000, g)
    return out


def a_id(c):
    return "A-%s-%s-%d-g%s-%s" % (c[0], c[1], c[2], c[3], "unit" if is_unit(PARAMS[c[1]]) else "general")


def a_signal(c):
    s, p, fs, g = c
    return signal(s, a_length(fs, PARAMS[p]), fs, PARAMS[p], GAINS[g], seed=1)


# ------------------------------------------------------------------------------ group B
B_RATES = (8000, 44100, 48000)
B_SIGNALS = ("bursts", "square", "am")
# burst seeds per rate whose traces give every B case its boundaries (asserted in
# tests/test_limiter_cases.py on the oracle)
B_SEEDS = {8000: 2, 44100: 2, 48000: 4}
LONG_CASE = ("bursts", 8000, 64, 64, 64 * 2050 + 5)


def b_warms(fs):
    B = ring_frames(fs, PARAMS["ref"])
    return (-1, 0, 1, 63, 64, 65, B - 1, 3 * int(fs * PARAMS["ref"]["release"] / 1000.0) + B)


def b_cases():
    """[(signal, fs, LS, W, frames)], the reference's parameter set throughout"""
    out = []

    def add(*c):
        if c not in out:
            out.append(c)

    for fs in B_RATES:
        B = ring_frames(fs, PARAMS["ref"])
        ls_min = max(64, B)                      # 64 at 8 kHz (B = 40), B above
        warms = b_warms(fs)
        for s in B_SIGNALS:
            # the walker's 64-boundary batches, a length that is no multiple of LS, one under 64
            # frames (two segments have one boundary, which cannot be both active and at rest: it
            # is active, and the at-rest precondition is asked of spans with two boundaries or more)
            for cnt in (1, 2, 64, 65, 66, 129, 130):
                for W in (-1, 0):
                    add(s, fs, ls_min, W, cnt * ls_min)
            for W in (-1, 0):
                add(s, fs, ls_min, W, 37 * ls_min + 17)
                add(s, fs, ls_min, W, 50)
            # every warm-up at three segment lengths, on a span of twelve full warm-ups or more
            for LS in (ls_min, 256, 1000):
                n = -(-max(8 * LS, 12 * warms[-1]) // LS) * LS + 3
                for W in warms:
                    add(s, fs, LS, W, n)
            add(s, fs, 16384, -1, 12000)         # one segment
    add(*LONG_CASE)
    return out


def b_id(c):
    return "B-%s-%d-LS%d-W%d-n%d" % c


def b_signal(c):
    s, fs, LS, W, n = c
    return signal(s, n, fs, PARAMS["ref"], seed=B_SEEDS[fs])


def b_boundaries(c):
    s, fs, LS, W, n = c
    return np.arange(LS, n, LS)


# ------------------------------------------------------------------------------ group C
C_RATES = (88200, 48000, 11025, 22050, 176400, 384000)
C_WINDOW = {88200: 0, 48000: 1, 11025: 2, 22050: 3, 176400: 3, 384000: 1}    # r = (4 - (h & 3)) & 3


def c_lengths(fs):
    B = ring_frames(fs, PARAMS["ref"])
    return (1, B - 2, B - 1, B, B + 1, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 5)


def c_cases():
    """[(fs, frames, set, gain name, step below the limit)]"""
    out = []
    for fs in C_RATES:
        for n in c_lengths(fs):
            out.append((fs, n, "ref", "off", 0))
    for fs in C_RATES[:5]:
        for n in (4097, 3 * 2048 + 5):
            for p in ("ref", "levels", "unit-edge", "unit-over"):
                for g in ("off", "0.5", "1.7"):
                    if (p, g) != ("ref", "off"):
                        out.append((fs, n, p, g, 0))
    for fs in (48000, 88200):
        out.append((fs, 3 * 2048 + 5, "limit-exact", "off", 0))
        out.append((fs, 3 * 2048 + 5, "limit-exact", "off", 1))
    return out


def c_id(c):
    return "C-%d-r%d-n%d-%s-g%s-%s%s" % (c[0], C_WINDOW[c[0]], c[1], c[2], c[3],
                                        "unit" if is_unit(PARAMS[c[2]]) else "general", "-below" if c[4] else "")


def c_signal(O, c):
    fs, n, p, g, below = c
    lo, hi = allowed_range(O, PARAMS[p], GAINS[g])
    return quiet(n, fs, lo, hi, seed=3, top=hi - 1 if below else None)


# ------------------------------------------------------------------------------ group D
D_SETUPS = ((44100, "ref"), (48000, "ref"), (48000, "half"))
D_FRAMES = 20000
D_SEED = 4
D_CUTS = ("active", "rest", "1", "B-2", "B", "active+rest", "active+near", "1+B-2", "1+active+rest", "B+active+near",
          "rest+rest")


def d_signal(fs, p):
    return signal("bursts", D_FRAMES, fs, PARAMS[p], seed=D_SEED)


def d_points(att, B):
    """from the oracle's trace: `active`, a frame in the middle of the longest stretch with att
    != 1 that starts after frame 2 B; `rest`, a frame whose B frames before it and itself are at
    att = 1, after that stretch (none: before it); `rest2`, 100 frames on (still at rest)"""
    on = att != 1.0                                        # (a release may end a hair over 1)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], on.view(np.int8), [0]])))
    runs = [(a, b) for a, b in zip(edges[0::2], edges[1::2]) if a > 2 * B]
    a, b = max(runs, key=lambda r: r[1] - r[0])
    active = int((a + b) // 2)
    busy = np.concatenate([[0], np.cumsum(on)])
    f = np.arange(2 * B, att.size - 101)
    idx = f[busy[f + 101] - busy[f - B] == 0]              # att = 1 on [f - B, f + 100]
    later = idx[idx > b]
    rest = int(later[0] if later.size else idx[0])
    return dict(active=active, rest=rest, rest2=rest + 100)


def d_cuts(name, pts, B):
    near = pts["active"] + B - 3                           # two cuts fewer than B frames apart
    table = {"active": [pts["active"]], "rest": [pts["rest"]], "1": [1], "B-2": [B - 2], "B": [B],
             "active+rest": sorted([pts["active"], pts["rest"]]), "active+near": [pts["active"], near],
             "1+B-2": [1, B - 2], "1+active+rest": sorted([1, pts["active"], pts["rest"]]),
             "B+active+near": [B, pts["active"], near], "rest+rest": [pts["rest"], pts["rest2"]]}
    return table[name]
