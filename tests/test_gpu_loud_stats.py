"""GPU: the loudness histogram and decision kernels (k_hist, k_decide) on crafted inputs.

Both kernels take plain device arrays, so the tests write values straight into a
measure-only MasteringJob's ``hops`` / ``hist`` / ``st_hist`` / ``peak`` tensors and call
``job.histograms()`` / ``job.decide()``: no audio is processed, a job of T tracks is T cases
per launch.

1. k_hist against an exact restatement (``_ref_hist``).  Every hop energy of a track is an
   integer multiple of one power of two, and any 60 of them sum below 2^53 of it, so every
   partial sum is exact in any order and the one division rounds identically everywhere:
   the comparison is equality on all 1000 bins, with no allowance.  Block energies are
   searched on the CPU to sit on the last double below a bin bound and on the bound itself
   (``_quotient_search``: an exact sum below 2^53 granules cannot reach every double, so a
   bound is met exactly by its gating case, its short-term case or both).

2. k_decide's statistics against the C oracle (``oracle.loudness_stats``): raw values to
   1e-9 dB (the sums are bit-identical by construction, only log10 may differ between the
   device's libm and the host's, by a few ulp, < 1e-13 dB), ``round2`` against exact decimal
   formatting of the device's own raw values, and the rounded values against the oracle's
   "%.2f" strings.  ``test_stat_cases_clear_of_ties`` (no GPU) asserts that every reference
   value lies at least 1e-6 dB from a rounding tie, so the 1e-9 can never flip a digit.
   NOT covered: round2's branch for a product that rounds to exactly k + 0.5.  It cannot be
   reached with certainty through this ABI (it needs control of the last bit of a log10).
   For the same reason no case here is a lone gating bin: a lone block in bin j has
   I = j / 10 - 69.95 up to a few ulp, which IS a "%.2f" tie, so the "one block in bin j"
   cases put the lone block in the short-term histogram (bin j's owner lane and slot serve
   both percentiles) and give the gating histogram a second block 41 bins away; the
   "two distant bins" cases split the upper bin in two for the same reason.

3. The decision (mode, gain, control word) against ``oracle.loudnorm_linear_gain`` on the
   oracle's strings, over every track, for every launch of ``_launches()``: the default
   targets, target_tp / target_lra set to exactly the measured value and to the next double below,
   a wide target_tp (so that the TP sentinel 99.00 alone decides), level_in 2, a limit that
   the gained peak meets exactly, and loudnorm off (NULL histograms).

4. The limiter-idle bit (AMX_CTL_FAST) against the real gain stage: ``oracle.linear_gain``
   on the samples [m, -m], FAST exactly when max |sample| / 32768 * level_in <= limit.

5. ``test_matrix_reaches_every_branch`` (no GPU) asserts on the reference arithmetic that
   the matrix takes every branch, mode, sentinel and equality at least once.
"""
import functools
import math

import numpy as np
import pytest

HOP = 19200                      # 100 ms of the 192 kHz measurement stream
BIG = 2.0 ** 40                  # fills the hop rows past a track's own hops: never counted
TIE_MARGIN_DB = 1e-6
RAW_TOL_DB = 1e-9
GAIN_TOL_ULP = 4
TARGET_I, TARGET_TP, TARGET_LRA = -14.0, -1.5, 11.0
LIMIT = 0.98
PEAK_M = (0, 1, 32111, 32112, 32113, 32767, 32768)


# =============================================================== 1. k_hist
def _nh(n, fs):
    return -(-n * 192000 // fs) // HOP


def _ref_hist(h, bounds):
    """h: [nh, 2] hop energies.  Gating block k = hops k..k+3, short-term block m = the 30
    hops that end at hop 30 + 10 m, both channels; a block below bounds[0] is dropped, else
    it lands in the largest bin whose lower bound is <= its energy (capped at 999)."""
    hist, st = np.zeros(1000, np.uint64), np.zeros(1000, np.uint64)
    nh = h.shape[0]

    def put(dst, lo, hi, frames):
        e = math.fsum(h[lo:hi].ravel().tolist()) / float(frames)
        if e >= bounds[0]:
            dst[int(np.searchsorted(bounds[:1000], e, side="right")) - 1] += 1

    for k in range(nh - 3):
        put(hist, k, k + 4, 4 * HOP)
    m = 0
    while 30 + 10 * m <= nh:
        put(st, 10 * m, 30 + 10 * m, 30 * HOP)
        m += 1
    return hist, st


def _quotient_search(b, frames):
    """(g, N_below, N_at): a power of two g and neighbouring integers N < 2^53 with
    N_below g / frames the largest such quotient below b and N_at g / frames the smallest at
    or above b.  With N in [2^52, 2^53) the quotients are 0.5 to 2 ulp apart, so they are
    the last double below b and b itself for most bounds, and never more than 2 ulp away."""
    g = 2.0 ** (math.frexp(b * frames)[1] - 53)          # b frames / g in [2^52, 2^53)
    n0 = int(b * frames / g)
    below = at = None
    for n in range(n0 - 16, n0 + 17):
        q = (float(n) * g) / float(frames)
        if q < b:
            below = n
        elif at is None:
            at = n
    assert below is not None and at == below + 1 and at < 2 ** 53
    return g, below, at


def _spread(total, count, rng):
    """count positive integers that sum to total, uneven"""
    base = total // count
    v = [base] * count
    v[0] += total - base * count
    for i in range(0, count - 1, 2):
        r = int(rng.integers(0, base // 2))
        v[i] -= r
        v[i + 1] += r
    assert sum(v) == total and min(v) > 0
    return v


def _dyadic_track(nh, rng, lo=12, hi=46):
    """[nh, 2] multiples of 2^-30 below 2^16, log-uniform"""
    k = np.floor(2.0 ** rng.uniform(lo, hi, size=(nh, 2)))
    return k * 2.0 ** -30


BOUND_BINS = (0, 1, 16, 500, 992, 999, 1000)     # bounds[j]: the first, a lane seam, the top
LENGTHS_NH = (0, 3, 4, 5, 29, 30, 31, 39, 40, 41)


@functools.lru_cache(maxsize=None)
def _hist_jobs():
    """{job name: (fs, [track dict])}; a track: n frames, nh, h [nh, 2], g (its granule), and
    for a bound case: edge = (kind, bound index, side)"""
    import oracle as O
    _, B = O.ebur128_tables()
    rng = np.random.default_rng(20240611)
    many = []
    for nh in LENGTHS_NH:
        many.append(dict(n=4800 * nh + (4799 if nh % 2 == 0 else 1), h=_dyadic_track(nh, rng), g=2.0 ** -30))
    many.append(dict(n=4800 * 40, h=np.zeros((40, 2)), g=2.0 ** -30, zero=True))
    for j in BOUND_BINS:
        for kind, nh, cnt, frames in (("gating", 4, 8, 4 * HOP), ("short", 30, 60, 30 * HOP)):
            g, below, at = _quotient_search(B[j], frames)
            for side, N in (("below", below), ("at", at)):
                v = np.array(_spread(N, cnt, rng), np.float64).reshape(nh, 2) * g
                many.append(dict(n=4800 * nh, h=v, g=g, edge=(kind, j, side)))
    # far above the top bound: bin 999
    many.append(dict(n=4800 * 4, h=np.full((4, 2), 2.0 ** 25), g=2.0 ** -10, top=True))
    many.append(dict(n=4800 * 30, h=np.full((30, 2), 2.0 ** 25 + 2.0 ** -10), g=2.0 ** -10, top=True))
    while len(many) < 70:                                   # more than one wave's worth of blocks
        nh = int(rng.integers(4, 42))
        many.append(dict(n=4800 * nh + int(rng.integers(0, 4800)), h=_dyadic_track(nh, rng, 20, 40), g=2.0 ** -30))
    long48 = [dict(n=4800 * 300 + 17, h=_dyadic_track(300, rng, 18, 46), g=2.0 ** -30),
              dict(n=4800 * 5, h=_dyadic_track(5, rng), g=2.0 ** -30),
              dict(n=4799, h=np.zeros((0, 2)), g=2.0 ** -30)]
    r441 = []
    for k in (1, 4, 5, 30, 31, 40, 41, 300):                # 4410 k frames are k hops exactly
        for n in (4410 * k, 4410 * k - 1):
            nh = _nh(n, 44100)
            r441.append(dict(n=n, h=_dyadic_track(nh, rng, 16, 44), g=2.0 ** -30))
    jobs = {"48k-many": (48000, many), "48k-long": (48000, long48), "44k1": (44100, r441)}
    for fs, tracks in jobs.values():
        for tr in tracks:
            tr["nh"] = _nh(tr["n"], fs)
            assert tr["h"].shape == (tr["nh"], 2), (tr["n"], fs, tr["h"].shape)
            tr["ref"] = _ref_hist(tr["h"], B)
            tr["h"].setflags(write=False)
    return jobs


def test_hist_inputs_are_exact(oracle_mod):
    """the k_hist cases' preconditions, on the CPU: exact sums, the lengths asked for, and
    block energies on both sides of the bounds"""
    _, B = oracle_mod.ebur128_tables()
    jobs = _hist_jobs()
    for name, (fs, tracks) in jobs.items():
        for tr in tracks:
            k = tr["h"] / tr["g"]
            assert np.all(k == np.floor(k)) and np.all(k >= 0), name
            if k.size:
                # any sum of up to 60 hop values (a short-term block, both channels) is exact
                most = sum(int(v) for v in k.ravel()) if k.size <= 60 else 60 * int(k.max())
                assert most < 2 ** 53, name
    many = jobs["48k-many"][1]
    assert len(many) > 64
    assert {tr["nh"] for tr in many} >= set(LENGTHS_NH)
    assert {tr["nh"] for tr in jobs["44k1"][1]} >= set(LENGTHS_NH) | {299, 300}
    assert {tr["nh"] for tr in jobs["48k-long"][1]} == {300, 5, 0}
    # the ceiling decides: 4410 k - 1 frames are one hop fewer than 4410 k
    for a, b in zip(jobs["44k1"][1][0::2], jobs["44k1"][1][1::2]):
        assert a["nh"] == b["nh"] + 1
    seen, exact = set(), set()
    for tr in many:
        if "edge" not in tr:
            continue
        kind, j, side = tr["edge"]
        frames = (4 if kind == "gating" else 30) * HOP
        e = math.fsum(tr["h"].ravel().tolist()) / frames
        ref = tr["ref"][0 if kind == "gating" else 1]
        assert int(ref.sum()) == (0 if (j == 0 and side == "below") else 1)
        ulp = float(np.spacing(B[j]))
        if side == "below":
            assert B[j] - 2 * ulp <= e < B[j]
            assert j == 0 or ref[j - 1] == 1
            if e == np.nextafter(B[j], -np.inf):
                exact.add((j, side))
        else:
            assert B[j] <= e <= B[j] + 2 * ulp
            assert ref[min(j, 999)] == 1
            if e == B[j]:
                exact.add((j, side))
        seen.add(tr["edge"])
    assert len(seen) == len(BOUND_BINS) * 4
    # every bound is met exactly, and missed by one ulp, by its gating or its short-term case
    assert exact == {(j, side) for j in BOUND_BINS for side in ("below", "at")}
    for tr in many:
        if tr.get("zero"):
            assert tr["ref"][0].sum() == 0 and tr["ref"][1].sum() == 0
        if tr.get("top"):
            assert tr["ref"][0][999] == tr["nh"] - 3 and tr["ref"][0].sum() == tr["nh"] - 3
            assert tr["ref"][1][999] == (1 if tr["nh"] >= 30 else 0)
    # the references are not all alike: many bins are hit
    assert len(np.nonzero(sum(tr["ref"][0] for tr in many))[0]) > 100


def _hist_job(fs, tracks):
    from amx.engine import MasteringJob
    job = MasteringJob(fs, 2, {"lufs": TARGET_I}, [tr["n"] for tr in tracks], input_s16=True,
                       measure_only=True)
    assert job.plan.info.hop_frames == HOP
    assert job.max_hops > max(tr["nh"] for tr in tracks)
    return job


def _hop_rows(job, tracks, fill=None):
    """the [T, max_hops, 2] hop array: each track's own hops, BIG past them"""
    a = np.full((len(tracks), job.max_hops, 2), BIG, np.float64)
    for t, tr in enumerate(tracks):
        a[t, :tr["nh"]] = tr["h"] if fill is None else fill
    return a


def _histograms(job, rows):
    import torch
    job.hops.copy_(torch.from_numpy(rows))
    job.histograms()
    torch.cuda.synchronize()
    return job.hist.cpu().numpy().view(np.uint64), job.st_hist.cpu().numpy().view(np.uint64)


def _assert_hist(tracks, hist, st, refs, what):
    for t, tr in enumerate(tracks):
        rh, rs = refs[t]
        bad = np.nonzero(hist[t] != rh)[0]
        assert bad.size == 0, "%s track %d (nh %d, %s): gating bins %s: %s, reference %s" % (
            what, t, tr["nh"], tr.get("edge"), bad[:8], hist[t][bad[:8]], rh[bad[:8]])
        bad = np.nonzero(st[t] != rs)[0]
        assert bad.size == 0, "%s track %d (nh %d, %s): short-term bins %s: %s, reference %s" % (
            what, t, tr["nh"], tr.get("edge"), bad[:8], st[t][bad[:8]], rs[bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["48k-many", "48k-long", "44k1"])
def test_hist_equals_exact_reference(gpu, oracle_mod, name):
    """k_hist, all 1000 bins of both histograms of every track, equal to the restatement;
    the histograms start as garbage (they are written whole) and the rows past a track's
    own hops hold large values that must not be counted"""
    fs, tracks = _hist_jobs()[name]
    job = _hist_job(fs, tracks)
    job.hist.fill_(0x7f7f7f7f7f7f)
    job.st_hist.fill_(-3)
    hist, st = _histograms(job, _hop_rows(job, tracks))
    _assert_hist(tracks, hist, st, [tr["ref"] for tr in tracks], name)
    print("LOUDSTATS k_hist %s: %d tracks, %d gating and %d short-term blocks, bins equal" % (
        name, len(tracks), int(hist.sum()), int(st.sum())))
    job.plan.close()


@pytest.mark.gpu
def test_hist_second_call_leaves_nothing_stale(gpu, oracle_mod):
    """two calls on the same histogram tensors with different hops: the second result is the
    second input's alone"""
    _, B = oracle_mod.ebur128_tables()
    fs, tracks = _hist_jobs()["48k-many"]
    job = _hist_job(fs, tracks)
    one = 2.0 ** -3                     # every hop alike: every block of every track in one bin
    hist, st = _histograms(job, _hop_rows(job, tracks, fill=one))
    refs = [_ref_hist(np.full((tr["nh"], 2), one), B) for tr in tracks]
    _assert_hist(tracks, hist, st, refs, "first call")
    assert sum(int(r[0].sum()) for r in refs) == sum(max(0, tr["nh"] - 3) for tr in tracks)
    hist, st = _histograms(job, _hop_rows(job, tracks))
    _assert_hist(tracks, hist, st, [tr["ref"] for tr in tracks], "second call")
    job.plan.close()


# ============================================= 2. k_decide: the statistic cases
def _bins(d):
    a = np.zeros(1000, np.uint64)
    for j, c in d.items():
        a[j] = c
    return a


def _walk(hist, st, E, B):
    """ebur128_gated_loudness / relative threshold / loudness range on histograms, restated
    with the branches it takes: (I, lra, thr, flags, relative gate).  Empty bins add an exact 0.0, so the
    sums run over the non-empty bins in ascending order."""
    lufs = lambda e: 10 * math.log10(e) - 0.691
    flags = set()

    def gate_bin(v, name):
        if v < B[0]:
            flags.add(name + "<b0")
            return 0
        flags.add(name + ">=b0")
        j = int(np.searchsorted(B[:1000], v, side="right")) - 1
        if v > E[j]:
            flags.add("++" + name)
            return j + 1
        flags.add("no++" + name)
        return j

    I, thr, lra, rel = -math.inf, -70.0, 0.0, None
    nz = [int(j) for j in np.nonzero(hist)[0]]
    if nz:
        rel, cnt = 0.0, 0
        for j in nz:
            rel += float(int(hist[j])) * E[j]
            cnt += int(hist[j])
        rel /= float(cnt)
        rel *= 0.1
        thr = lufs(rel)
        start = gate_bin(rel, "start")
        g, above = 0.0, 0
        for j in nz:
            if j >= start:
                g += float(int(hist[j])) * E[j]
                above += int(hist[j])
        if above:
            I = lufs(g / float(above))
        if above < cnt:
            flags.add("gate-removes")
    nz = [int(j) for j in np.nonzero(st)[0]]
    if nz:
        size, power = 0.0, 0.0
        for j in nz:
            size += float(int(st[j]))
            power += float(int(st[j])) * E[j]
        power /= size
        index = gate_bin(0.01 * power, "index")
        kept = [j for j in nz if j >= index]
        if len(kept) < len(nz):
            flags.add("lra-gate-removes")
        tot = float(sum(int(st[j]) for j in kept))
        if tot:
            plo, phi = int((tot - 1) * 0.1 + 0.5), int((tot - 1) * 0.95 + 0.5)
            flags.add(("plo", plo) if tot <= 24 else "plo-large")
            flags.add(("phi", phi) if tot <= 24 else "phi-large")
            c, jl, jh = 0, None, None
            for j in kept:
                c += int(st[j])
                if jl is None and c > plo:
                    jl = j
                if jh is None and c > phi:
                    jh = j
            lra = lufs(E[jh]) - lufs(E[jl])
    return I, lra, thr, flags, rel


def _tie_distance_db(v):
    """distance of v from the nearest "%.2f" rounding tie, in dB"""
    if not math.isfinite(v):
        return math.inf
    x = abs(v) * 100.0
    return abs(x - math.floor(x) - 0.5) / 100.0


def _fmt(v):
    return "%.2f" % v


def _search_two_bins(O, lo, hi, want, which, cmax=60):
    """counts (a, b) for bins lo and hi whose statistic `which` (0 I, 2 threshold) prints as
    `want`, clear of a tie"""
    for a in range(1, cmax):
        for b in range(1, cmax):
            s = O.loudness_stats(_bins({lo: a, hi: b}), _bins({}))
            if _fmt(s[which]) == want and _tie_distance_db(s[which]) > 1e-4 and math.isfinite(s[0]):
                return a, b
    return None


ST_PLAIN = {610: 3, 640: 4, 655: 2}          # LRA 4.5: inside (0, 11]
HIST_PLAIN = {520: 6, 545: 9, 560: 4}        # I about -16: gain above 1


@functools.lru_cache(maxsize=None)
def _stat_cases():
    """[(name, hist, st_hist)] -- made once, shared, read-only"""
    import oracle as O
    E, B = O.ebur128_tables()
    rng = np.random.default_rng(9639)
    C = []
    add = lambda name, h, s: C.append((name, _bins(h), _bins(s)))
    add("empty-both", {}, {})
    add("empty-gating", {}, {500: 3, 540: 2})
    add("empty-short-term", {500: 3, 540: 2}, {})
    for j in (0, 1, 15, 16, 17, 499, 992, 998, 999):
        # the lone block: short-term (see the module docstring); gating gets a second bin
        add("one-block-%d" % j, {j: 1, (j + 41 if j + 41 < 1000 else j - 41): 1}, {j: 1})
        add("one-block-st-%d" % j, HIST_PLAIN, {j: 1, (j + 23 if j + 23 < 1000 else j - 23): 1})
    # two distant bins, lopsided: the relative gate below / inside (both halves) / above
    # the lower bin; the upper bin is split over two (a lone survivor would be a tie)
    for lo, up in ((400, 600), (3, 40), (16, 215)):
        found = {}
        for ca in sorted({int(round(1.005 ** k)) for k in range(0, 2400)}):
            _, _, _, f, rel = _walk(_bins({lo: ca, up: 1000, up + 3: 500}), _bins({}), E, B)
            if "start<b0" in f:
                key = "below-b0"
            elif rel < B[lo]:
                key = "below"
            elif rel >= B[lo + 1]:
                key = "above"
            else:
                key = "inside-taken" if "++start" in f else "inside-not-taken"
            found.setdefault(key, ca)
        for key, ca in sorted(found.items()):
            add("distant-%d-%d-%s" % (lo, up, key), {lo: ca, up: 1000, up + 3: 500},
                {lo + 150: ca, up: 1000, up + 3: 500})
    # adjacent bins across a lane seam
    for a in (15, 511, 991, 998):
        add("seam-%d-%d" % (a, a + 1), {a: 3, a + 1: 5}, {a: 2, a + 1: 7})
    # the relative gate (10 dB down) and the LRA gate (20 dB down) walked over the seam 15 | 16
    for k in range(10, 22):
        add("gate-at-%d" % k, {100 + k: 1, 101 + k: 2}, {200 + k: 1, 201 + k: 2, 260: 1})
    j = np.arange(1000)
    add("all-bins", dict(zip(j, (j * 7919) % 13 + 1)), dict(zip(j, (j * 104729) % 7 + 1)))
    add("all-bins-max", dict(zip(j, [2 ** 32 - 1] * 1000)), dict(zip(j, [2 ** 32 - 1] * 1000)))
    add("max-counts", {300: 2 ** 32 - 1, 650: 2 ** 32 - 1, 651: 1}, {640: 2 ** 32 - 1, 700: 2 ** 32 - 2, 701: 5})
    add("max-counts-low", {520: 2 ** 32 - 1, 560: 2 ** 31 + 12345}, {600: 2 ** 32 - 1, 655: 2 ** 30 + 7})
    # n single short-term blocks: every step of both percentile indices
    for n in list(range(1, 25)) + [101, 199]:
        step = 5 if n <= 24 else 1
        add("st-singles-%d" % n, {440 + 5 * (n % 25): 10, 455 + 5 * (n % 25): 7, 470 + 5 * (n % 25): 3},
            {600 + step * i: 1 for i in range(n)})
    add("st-1001", HIST_PLAIN, dict([(700 + i, 5) for i in range(200)] + [(650, 1)]))
    # short-term blocks more than 20 dB below the mean: removed by the LRA gate
    add("st-gated-half", HIST_PLAIN, {300: 5, 700: 5, 730: 2})
    add("st-gated-one", HIST_PLAIN, {480: 1, 690: 100, 700: 100})
    add("st-gate-below-b0", HIST_PLAIN, {50: 2, 60: 1, 95: 3})
    for i in range(36):
        def sparse():
            k = int(rng.integers(1, 13))
            where = rng.choice(1000, size=k, replace=False)
            return {int(b): int(2.0 ** rng.uniform(0, 32)) for b in where}
        add("random-%d" % i, sparse(), sparse())
    # sentinels: the threshold prints -70.00 while I is finite; I prints 0.00 and -0.00
    a, b = _search_two_bins(O, 98, 102, "-70.00", 2)
    add("thr-minus-70", {98: a, 102: b}, ST_PLAIN)
    a, b = _search_two_bins(O, 699, 700, "0.00", 0)
    add("i-zero", {699: a, 700: b}, ST_PLAIN)
    a, b = _search_two_bins(O, 699, 700, "-0.00", 0)
    add("i-minus-zero", {699: a, 700: b}, ST_PLAIN)
    add("lra-zero", HIST_PLAIN, {640: 4})
    add("lra-wide", HIST_PLAIN, {500: 3, 640: 4, 655: 2})           # LRA 15.5 > 11
    add("plain", HIST_PLAIN, ST_PLAIN)
    add("plain-loud", {640: 6, 660: 9, 671: 4}, ST_PLAIN)           # I above the target: gain < 0.98
    add("plain-near", {555: 6, 560: 9, 566: 4}, {620: 3, 640: 4})   # I near the target: gain near 1
    names = [c[0] for c in C]
    assert len(set(names)) == len(names)
    for _, h, s in C:
        h.setflags(write=False)
        s.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _oracle_stats():
    import oracle as O
    return [O.loudness_stats(h, s) for _, h, s in _stat_cases()]


# ================================================== 3./4. tracks, peaks, launches
def _peak_of_db(db):
    return 10.0 ** (db / 20.0)


@functools.lru_cache(maxsize=None)
def _tracks():
    """[(case index, (pk L, pk R, out L, out R), tag)]: every statistic case once, then the
    decision and limiter-bit cases on chosen statistic cases"""
    import oracle as O
    cases = _stat_cases()
    idx = {c[0]: i for i, c in enumerate(cases)}
    stats = _oracle_stats()
    rng = np.random.default_rng(1770)
    T = []

    def add(name, tp_db, m, tag, left_max=True, pk=None):
        pk = _peak_of_db(tp_db) if pk is None else pk
        po = m / 32768.0
        pair = lambda v, w: (v, w) if left_max else (w, v)
        T.append((idx[name], pair(pk, pk * 0.7) + pair(po, po * 0.5), tag))

    for i, (name, _, _) in enumerate(cases):
        add(name, float(rng.uniform(-60.0, -25.0)), PEAK_M[i % len(PEAK_M)], "stat", left_max=i % 2 == 0)
    # measured peak 0 (TP -inf), with and without an output peak
    add("plain", 0.0, 0, "pk-zero", pk=0.0)
    add("plain", 0.0, 32113, "pk-zero", pk=0.0, left_max=False)
    add("empty-both", 0.0, 32768, "pk-zero", pk=0.0)
    # the sentinels alone: everything else would be linear (tp 99 needs the wide target_tp)
    add("thr-minus-70", -60.0, 1, "sentinel-thr")
    add("i-zero", -30.0, 1, "sentinel-i")
    add("i-minus-zero", -30.0, 1, "sentinel-i")
    add("lra-zero", -30.0, 1, "sentinel-lra")
    add("plain", 99.0, 1, "sentinel-tp")
    add("plain", 98.99, 1, "sentinel-tp-neighbour", left_max=False)
    # the target equalities are taken on this track
    add("plain", -12.34, 20000, "equality")
    # TP too high for linear: dynamic by the comparison alone
    add("plain", -1.0, 20000, "tp-too-high")
    add("lra-wide", -30.0, 20000, "lra-too-high")
    # the limiter bit: every peak value on a gain below 0.98, near 1 and above 1, on a
    # dynamic and on a skipped track; and the peaks whose gained value is 32112 / 32113
    for name in ("plain", "plain-loud", "plain-near", "lra-zero", "empty-both"):
        for k, m in enumerate(PEAK_M):
            add(name, -40.0, m, "fast", left_max=k % 2 == 0)
    for name in ("plain", "plain-near"):
        I = stats[idx[name]][0]
        g = 10.0 ** ((TARGET_I - float(_fmt(I))) / 20.0)
        y = O.linear_gain(np.arange(1, 32768, dtype=np.int16), g).astype(np.int64)
        for want in (32112, 32113):
            hit = np.nonzero(y == want)[0]          # a gain above 1 steps over some values
            if hit.size:
                add(name, -40.0, int(hit[0]) + 1, "fast-gained-%d" % want)
    assert {"fast-gained-32112", "fast-gained-32113"} <= {t[2] for t in T}
    return T


def _equality_targets():
    """the equality track's offset_tp and slra under the default target_i"""
    trk = [t for t in _tracks() if t[2] == "equality"]
    assert len(trk) == 1
    ci, pk, _ = trk[0]
    I, lra, _ = _oracle_stats()[ci]
    stp = float(_fmt(20.0 * np.log10(max(pk[0], pk[1]))))
    si, slra = float(_fmt(I)), float(_fmt(lra))
    return stp + (TARGET_I - si), slra


@functools.lru_cache(maxsize=None)
def _launches():
    otp, slra = _equality_targets()
    base = dict(lufs_on=1, target_i=TARGET_I, target_tp=TARGET_TP, target_lra=TARGET_LRA, level_in=1.0,
                limit=LIMIT)
    L = {"default": {}, "tp-equal": dict(target_tp=otp),
         "tp-next-below": dict(target_tp=float(np.nextafter(otp, -np.inf))),
         "lra-equal": dict(target_lra=slra),
         "lra-next-below": dict(target_lra=float(np.nextafter(slra, -np.inf))),
         "tp-wide": dict(target_tp=200.0), "level-in-2": dict(level_in=2.0),
         "limit-exact": dict(limit=32112.0 / 32768.0), "lufs-off": dict(lufs_on=0)}
    return {k: dict(base, **v) for k, v in L.items()}


LAUNCH_NAMES = ("default", "tp-equal", "tp-next-below", "lra-equal", "lra-next-below", "tp-wide",
                "level-in-2", "limit-exact", "lufs-off")
MODE_NUM = {"off": 0, "skip": 1, "linear": 2, "dynamic": 3}


@functools.lru_cache(maxsize=None)
def _expected(launch):
    """per track, from the oracle alone: raw statistics, the "%.2f" strings, mode, gain,
    the gained peak and the limiter bit"""
    import oracle as O
    L = _launches()[launch]
    stats = _oracle_stats()
    out = []
    for ci, pk, tag in _tracks():
        I, lra, thr = stats[ci] if L["lufs_on"] else (-math.inf, 0.0, -70.0)
        p, po = max(pk[0], pk[1]), max(pk[2], pk[3])
        tp = 20.0 * np.log10(p) if p > 0 else -math.inf
        s = {"input_i": _fmt(I), "input_tp": _fmt(tp), "input_lra": _fmt(lra), "input_thresh": _fmt(thr)}
        if L["lufs_on"]:
            mode, gain = O.loudnorm_linear_gain(s, L["target_i"], L["target_tp"], L["target_lra"])
        else:
            mode, gain = "off", None
        m = int(round(po * 32768.0))
        x = np.array([min(m, 32767), -m], np.int16)
        y = O.linear_gain(x, gain) if gain is not None else x
        amax = int(np.abs(y.astype(np.int64)).max())
        fast = amax / 32768.0 * L["level_in"] <= L["limit"]
        out.append(dict(raw=(I, lra, thr, float(tp)), strings=s, mode=mode, gain=gain, amax=amax,
                        fast=bool(fast), pk=p, pk_out=po, tag=tag, case=ci))
    return out


def test_stat_cases_clear_of_ties(oracle_mod):
    """every reference statistic (I, LRA, threshold of every case, TP of every track) lies
    at least 1e-6 dB from a "%.2f" rounding tie -- a case that fails this is replaced, never
    excluded at run time -- and the branch restatement agrees with the oracle"""
    E, B = oracle_mod.ebur128_tables()
    worst = math.inf
    for (name, h, s), ref in zip(_stat_cases(), _oracle_stats()):
        for k, v in enumerate(ref):
            d = _tie_distance_db(v)
            assert d >= TIE_MARGIN_DB, "%s: statistic %d = %r is %.3g dB from a tie" % (name, k, v, d)
            worst = min(worst, d)
        I, lra, thr, _, _ = _walk(h, s, E, B)
        for a, b in zip((I, lra, thr), ref):
            assert a == b or abs(a - b) <= RAW_TOL_DB, (name, a, b)
    for e in _expected("default"):
        d = _tie_distance_db(e["raw"][3])
        assert d >= TIE_MARGIN_DB, "track %s: TP %r is %.3g dB from a tie" % (e["tag"], e["raw"][3], d)
        worst = min(worst, d)
    print("LOUDSTATS %d statistic cases, %d tracks, %d launches; closest tie %.3g dB" % (
        len(_stat_cases()), len(_tracks()), len(LAUNCH_NAMES), worst))


def test_matrix_reaches_every_branch(oracle_mod):
    """on the reference arithmetic alone: the matrix takes each branch, mode, sentinel and
    equality at least once"""
    E, B = oracle_mod.ebur128_tables()
    flags = set()
    for _, h, s in _stat_cases():
        flags |= _walk(h, s, E, B)[3]
    for f in ("start<b0", "start>=b0", "++start", "no++start", "index<b0", "index>=b0", "++index",
              "no++index", "gate-removes", "lra-gate-removes", "plo-large", "phi-large"):
        assert f in flags, f
    # every step of both percentile indices for 1 to 24 blocks
    assert {f[1] for f in flags if isinstance(f, tuple) and f[0] == "plo"} >= {0, 1, 2}
    assert {f[1] for f in flags if isinstance(f, tuple) and f[0] == "phi"} >= set(range(0, 23))
    assert len(_tracks()) > 64
    exp = {n: _expected(n) for n in LAUNCH_NAMES}
    assert {e["mode"] for e in exp["default"]} == {"skip", "linear", "dynamic"}
    assert {e["mode"] for e in exp["lufs-off"]} == {"off"}
    # FAST set and cleared, with and without a gain; the peaks on both sides of the limit
    for n in ("default", "level-in-2", "limit-exact"):
        assert {(e["gain"] is not None, e["fast"]) for e in exp[n]} == {(a, b) for a in (0, 1) for b in (0, 1)}, n
    assert {e["fast"] for e in exp["lufs-off"]} == {True, False}
    for gained in (False, True):
        am = {e["amax"] for e in exp["default"] if (e["gain"] is not None) == gained}
        assert {32112, 32113} <= am, gained
    # amax * level_in == limit exactly (FAST), and one step above (not FAST)
    le = exp["limit-exact"]
    assert any(e["amax"] == 32112 and e["fast"] for e in le) and any(e["amax"] == 32113 and not e["fast"] for e in le)
    assert any(e["amax"] / 32768.0 * 2.0 > LIMIT >= e["amax"] / 32768.0 for e in exp["level-in-2"])
    # the sentinels, each alone: with the sentinel's own value replaced the track is linear
    by = lambda n, tag: [e for e in exp[n] if e["tag"] == tag]
    import oracle as O

    def alone(e, launch, key, other):
        L = _launches()[launch]
        assert e["mode"] == "dynamic", (e["tag"], e["strings"])
        s = dict(e["strings"], **{key: other})
        assert O.loudnorm_linear_gain(s, L["target_i"], L["target_tp"], L["target_lra"])[0] == "linear", e["tag"]

    (e,) = by("default", "sentinel-thr")
    assert e["strings"]["input_thresh"] == "-70.00" and e["strings"]["input_i"] != "-inf"
    alone(e, "default", "input_thresh", "-70.01")
    zeros = by("default", "sentinel-i")
    assert sorted(e["strings"]["input_i"] for e in zeros) == ["-0.00", "0.00"]
    for e in zeros:
        alone(e, "default", "input_i", "0.01")
    (e,) = by("default", "sentinel-lra")
    assert e["strings"]["input_lra"] == "0.00"
    alone(e, "default", "input_lra", "0.01")
    (e,) = by("tp-wide", "sentinel-tp")
    assert e["strings"]["input_tp"] == "99.00"
    alone(e, "tp-wide", "input_tp", "99.01")
    (e,) = by("tp-wide", "sentinel-tp-neighbour")
    assert e["strings"]["input_tp"] == "98.99" and e["mode"] == "linear"
    # the equalities, both sides
    otp, slra = _equality_targets()
    for n, mode in (("default", "linear"), ("tp-equal", "linear"), ("tp-next-below", "dynamic"),
                    ("lra-equal", "linear"), ("lra-next-below", "dynamic")):
        (e,) = by(n, "equality")
        assert e["mode"] == mode, n
    (e,) = by("tp-equal", "equality")
    L = _launches()["tp-equal"]
    assert float(e["strings"]["input_tp"]) + (L["target_i"] - float(e["strings"]["input_i"])) == L["target_tp"]
    assert float(e["strings"]["input_lra"]) == _launches()["lra-equal"]["target_lra"]
    (e,) = by("default", "tp-too-high")
    assert e["mode"] == "dynamic"
    assert any(e["mode"] == "dynamic" and float(e["strings"]["input_lra"]) > TARGET_LRA for e in exp["default"])
    # TP -inf, left above right and right above left
    assert any(e["pk"] == 0.0 and e["raw"][3] == -math.inf for e in exp["default"])
    sides = {(pk[0] > pk[1], pk[2] > pk[3]) for _, pk, _ in _tracks() if pk[0] != pk[1] and pk[2] != pk[3]}
    assert sides == {(True, True), (False, False)}


# ------------------------------------------------------------------ GPU side
_STATE = {}


@pytest.fixture(scope="module", autouse=True)
def _close_decide_job():
    yield
    job = _STATE.pop("job", None)
    if job is not None:
        import torch
        torch.cuda.synchronize()
        job.plan.close()


def _decide_job():
    """one measure-only job of one short track per case; the histograms and peaks are
    written once and never changed"""
    if "job" not in _STATE:
        import torch
        from amx.engine import MasteringJob
        tracks, cases = _tracks(), _stat_cases()
        T = len(tracks)
        job = MasteringJob(48000, 2, {"lufs": TARGET_I}, [480] * T, input_s16=True, measure_only=True)
        assert job.n_tracks == T and job.plan.info.hop_frames == HOP
        H = np.stack([cases[ci][1] for ci, _, _ in tracks]).view(np.int64)
        S = np.stack([cases[ci][2] for ci, _, _ in tracks]).view(np.int64)
        P = np.array([pk for _, pk, _ in tracks], np.float64)
        job.hist.copy_(torch.from_numpy(H))
        job.st_hist.copy_(torch.from_numpy(S))
        job.peak.copy_(torch.from_numpy(P))
        _STATE["job"] = job
        _STATE["runs"] = {}
    return _STATE["job"]


def _run(launch, publish=None):
    """k_decide under the launch's descriptors: {stats, gains, ctl} (one launch per name)"""
    import torch
    job = _decide_job()
    if publish is None and launch in _STATE["runs"]:
        return _STATE["runs"][launch]
    L = _launches()[launch]
    job.dd.lufs_on = L["lufs_on"]
    job.dd.target_i, job.dd.target_tp, job.dd.target_lra = L["target_i"], L["target_tp"], L["target_lra"]
    job.fd.level_in, job.fd.limit = L["level_in"], L["limit"]
    job.stats.fill_(float("nan"))
    job.gains.fill_(float("nan"))
    job.ctl.fill_(-1)
    job.plan.set_publish(publish)
    try:
        job.decide()
        torch.cuda.synchronize()
    finally:
        job.plan.set_publish(None)
    r = dict(stats=job.stats.cpu().numpy(), gains=job.gains.cpu().numpy(), ctl=job.ctl.cpu().numpy())
    if publish is None:
        _STATE["runs"][launch] = r
    return r


# stats[4..7] = round2 of I, TP, LRA, threshold = stats[0], [3], [1], [2]
ROUNDED = ((4, 0, "input_i"), (5, 3, "input_tp"), (6, 1, "input_lra"), (7, 2, "input_thresh"))


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["default", "lufs-off"])
def test_decide_raw_statistics(gpu, oracle_mod, launch):
    """stats[0..3] (I, LRA, threshold, TP) within 1e-9 dB of the oracle, -inf exactly"""
    st = _run(launch)["stats"]
    worst = 0.0
    for t, e in enumerate(_expected(launch)):
        for k, ref in enumerate(e["raw"]):
            got = float(st[t, k])
            if math.isinf(ref):
                assert got == ref, (t, e["tag"], k, got, ref)
                continue
            d = abs(got - ref)
            worst = max(worst, d)
            assert d <= RAW_TOL_DB, "track %d (%s) statistic %d: %r, oracle %r" % (t, e["tag"], k, got, ref)
    print("LOUDSTATS raw statistics, launch %s: largest |device - oracle| = %.3g dB" % (launch, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["default", "lufs-off"])
def test_decide_round2_matches_decimal_formatting(gpu, oracle_mod, launch):
    """stats[4..7] == float("%.2f" % raw), on the device's own raw values"""
    st = _run(launch)["stats"]
    for t, e in enumerate(_expected(launch)):
        for r, k, _ in ROUNDED:
            assert float(st[t, r]) == float(_fmt(float(st[t, k]))), (t, e["tag"], r, st[t, r], st[t, k])


@pytest.mark.gpu
@pytest.mark.parametrize("launch", ["default", "lufs-off"])
def test_decide_rounded_statistics(gpu, oracle_mod, launch):
    """stats[4..7] equal the oracle's "%.2f" values"""
    st = _run(launch)["stats"]
    for t, e in enumerate(_expected(launch)):
        for r, _, key in ROUNDED:
            assert float(st[t, r]) == float(e["strings"][key]), (t, e["tag"], key, st[t, r], e["strings"][key])


@pytest.mark.gpu
@pytest.mark.parametrize("launch", LAUNCH_NAMES)
def test_decision_every_track(gpu, oracle_mod, launch):
    """mode, gain (stats[9] and gains[t]), the control word, the limiter bit and the peaks
    of every track, against the oracle's decision under the launch's descriptors"""
    r = _run(launch)
    st, gains, ctl = r["stats"], r["gains"], r["ctl"]
    worst = 0.0
    for t, e in enumerate(_expected(launch)):
        what = "launch %s track %d (%s) %s" % (launch, t, e["tag"], e["strings"])
        assert int(st[t, 8]) == MODE_NUM[e["mode"]], what
        assert (int(ctl[t]) >> 4) & 15 == MODE_NUM[e["mode"]], what
        assert int(ctl[t]) & ~0xf1 == 0, what
        assert float(gains[t]) == float(st[t, 9]), what
        if e["gain"] is None:
            assert float(st[t, 9]) == -1.0, what
        else:
            ulp = abs(float(st[t, 9]) - e["gain"]) / float(np.spacing(e["gain"]))
            worst = max(worst, ulp)
            assert ulp <= GAIN_TOL_ULP, "%s: gain %r, oracle %r (%.1f ulp)" % (what, st[t, 9], e["gain"], ulp)
        # the limiter-idle bit promises that the gain stage's largest sample stays in the limit
        assert bool(int(ctl[t]) & 1) == e["fast"], "%s: gained peak %d" % (what, e["amax"])
        assert float(st[t, 10]) == (1.0 if e["fast"] else 0.0), what
        assert float(st[t, 11]) == e["pk"] and float(st[t, 12]) == e["pk_out"], what
    print("LOUDSTATS decision, launch %s: %d tracks, largest gain difference %.2f ulp" % (
        launch, len(gains), worst))


@pytest.mark.gpu
def test_skip_and_lufs_off(gpu, oracle_mod):
    """an empty gating histogram: mode 1, gain -1, control nibble 1; NULL histograms
    (loudnorm off): mode 0, gain -1, and the limiter bit still computed"""
    on, off = _run("default"), _run("lufs-off")
    n_skip = 0
    for t, (ci, _, _) in enumerate(_tracks()):
        if not _stat_cases()[ci][1].any():
            n_skip += 1
            assert on["stats"][t, 8] == 1.0 and on["stats"][t, 9] == -1.0 and on["gains"][t] == -1.0
            assert int(on["ctl"][t]) >> 4 == 1
    assert n_skip >= 3
    assert np.all(off["stats"][:, 8] == 0.0) and np.all(off["gains"] == -1.0) and np.all(off["ctl"] >> 4 == 0)
    fast = np.array([e["fast"] for e in _expected("lufs-off")])
    assert fast.any() and not fast.all()
    np.testing.assert_array_equal((off["ctl"] & 1).astype(bool), fast)
    assert np.all(np.isneginf(off["stats"][:, 0])) and np.all(off["stats"][:, 1] == 0.0)
    assert np.all(off["stats"][:, 2] == -70.0)


@pytest.mark.gpu
def test_target_equality(gpu, oracle_mod):
    """offset_tp <= target_tp and slra <= target_lra hold with equality: linear at the exact
    double, dynamic at the next double below"""
    (t,) = [i for i, tr in enumerate(_tracks()) if tr[2] == "equality"]
    for launch, mode in (("default", 2.0), ("tp-equal", 2.0), ("tp-next-below", 3.0), ("lra-equal", 2.0),
                         ("lra-next-below", 3.0)):
        r = _run(launch)
        assert r["stats"][t, 8] == mode, (launch, r["stats"][t])
        assert (r["gains"][t] > 0) == (mode == 2.0), launch
    # the device's own rounded values are the ones the targets were made from
    st = _run("default")["stats"][t]
    otp, slra = _equality_targets()
    assert st[5] + (TARGET_I - st[4]) == otp and st[6] == slra


@pytest.mark.gpu
def test_sentinels_force_dynamic(gpu, oracle_mod):
    """stp 99.00, sthr -70.00, slra 0.00 and si 0.00 / -0.00: each alone gives mode 3"""
    tags = [tr[2] for tr in _tracks()]
    d, w = _run("default")["stats"], _run("tp-wide")["stats"]
    (t,) = [i for i, g in enumerate(tags) if g == "sentinel-thr"]
    assert d[t, 7] == -70.0 and math.isfinite(d[t, 0]) and d[t, 8] == 3.0
    zs = [i for i, g in enumerate(tags) if g == "sentinel-i"]
    assert len(zs) == 2 and all(d[i, 4] == 0.0 and d[i, 8] == 3.0 for i in zs)
    assert sorted(bool(np.signbit(d[i, 4])) for i in zs) == [False, True]
    (t,) = [i for i, g in enumerate(tags) if g == "sentinel-lra"]
    assert d[t, 6] == 0.0 and d[t, 8] == 3.0
    (t,) = [i for i, g in enumerate(tags) if g == "sentinel-tp"]
    assert w[t, 5] == 99.0 and w[t, 8] == 3.0
    (t,) = [i for i, g in enumerate(tags) if g == "sentinel-tp-neighbour"]
    assert w[t, 5] == 98.99 and w[t, 8] == 2.0


@pytest.mark.gpu
def test_publish_equals_ctl(gpu, oracle_mod):
    """amx_plan_set_publish: the pinned words equal ctl for every track"""
    import torch
    T = len(_tracks())
    pin = torch.full((T,), -7, dtype=torch.int32).pin_memory()
    r = _run("default", publish=pin)
    np.testing.assert_array_equal(pin.numpy(), r["ctl"])
    np.testing.assert_array_equal(r["ctl"], _run("default")["ctl"])
    exp = _expected("default")
    np.testing.assert_array_equal(pin.numpy(), [MODE_NUM[e["mode"]] << 4 | int(e["fast"]) for e in exp])
