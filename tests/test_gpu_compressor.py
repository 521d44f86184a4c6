"""GPU: the multiband compressor (csrc/amx_dyn.hip) across its settings, rates and edges.

The chain under test is int16 stereo input with ``multiband`` on and no EQ, width or
analog stage, so the compressor (k_rms, the envelope kernels, k_gain_overlay and their
3..8-channel forms) and the overlay are the only non-trivial stages after the crossover.
Every case is compared per chunk with ``oracle.chunk`` BIT FOR BIT; the oracle's compressor
is pinned to the pydub restatement on the same ground by
tests/test_oracle.py::test_compressor_edges_match_pydub_restatement.

  group  what varies                                                            cases
  set    (threshold, ratio): the twelve PAIRS on all bands, six mixed triples,  23
         five seeded draws over the GUI's range; 48 / 44.1 kHz alternating
  setx   the two pairs whose thresholds music does not reach, on dc, sq110, alt 4
  rate   nine rates (detector window forms LP 256 / 512 / 1024, three rates     18
         with a fractional attack frame count) x defaults, (-40, 10)
  len    fifteen chunk lengths in one plan at 22.05 / 44.1 / 48 kHz (pydub's    6
         millisecond rounding: 0 output frames, growth by 9, cuts)
  edge   eight crafted signals (compressor_signals.py) x 48 / 96 kHz x           48
         (-40, 10), (-90, 10), (-25, 6)
  clamp  the overlay's two saturating adds on bands that saturate, 4 rates x    9
         compressor idle two ways; one case with width and EQ at 3 LSB
  split  set and edge at (-40, 10) / (-90, 10) under four envelope work splits  136
  div    both division forms of the envelope step (plan value env_rcp)          4
  mc     3 and 8 channels x four settings x two signals                         16

Shapes: two chunks of 12001 and 12023 frames (three or more k_rms tiles per chunk at
every LP: head tile, whole-tile fast path, tail tile; 11 or more envelope segments per
band).  The ``set`` / ``rate`` signal is ``synth.music_like`` at -1 dBFS whose level drops
by 60 dB half way through the second chunk (the 1.5 s tail at x 1e-3 begins there; the
chunk ends 6012 frames into it), so every band holds an attenuation over whole waves.

What a case must be able to show is asserted on the ORACLE ALONE in ``_reference``
(``test_preconditions_on_the_oracle`` runs that half without a GPU).

The envelope re-run counters are read as ``reruns + wide``: a segment re-run by the chain
walkers or by the optimistic parallel pass before them.

Three things the oracle showed while the cases were laid out, kept as assertions:
* no band of the -1 dBFS music reaches an rms of 16384 or 32764 over 5 ms, so the pairs
  (20 log10 0.5, 2) and (-0.001, 10) leave it untouched (QUIET_ON_MUSIC); the ``setx`` cases
  put them on signals where they engage;
* no band of this chain holds |sample| = 32767 for a whole detector window (see the comment
  in ``_reference``): the detector's top is r = 32765 on ``alt``, and ``sq110+sq5k`` clips its
  mid band on thousands of samples with r above 30000;
* with the VOCAL EQ the clipped squares' high band all but vanishes (the negative bass
  shelf), so the width + EQ case of ``clamp`` runs the overlay behind those stages without
  the two clamp orders differing; the eight plain cases differ on 3982 to 5870 samples.

That the tests can fail: five arithmetic-only changes to amx_dyn.hip, one at a time --
rms_floor without ``down`` (63 of the 265 tests fail: every group but clamp), ``look - 1`` in
k_rms (181: every group but clamp and mc, which has its own detector kernel), ``att < m`` in
env_step3 (185: every group but clamp), one clamp in k_gain_overlay (10: the eight plain clamp
cases and two of set), ``trunc`` in mul16 (223: every group but clamp).
"""
import functools
import math

import numpy as np
import pytest

from compressor_signals import PAIRS, SIGNALS, edge_signal
from test_gpu_multichannel import _chain as _mc_chain
from test_gpu_parity import VOCAL, _chunk_chain, _cmp

LENGTHS = (12001, 12023)
DEFAULT = ((-25.0, 6.0), (-20.0, 3.0), (-15.0, 4.0))
UNTOUCHED = ((-40.0, 1.0), (0.0, 10.0), (3.0, 4.0))       # ratio 1, or no rms over the threshold
# two thresholds no band of the -1 dBFS music reaches over a 5 ms window (rms 16384 and 32764):
# on music they pin the activity skip (ChainDev::rq high in the table); the crafted signals
# ``dc`` and ``sq110+sq5k`` carry them into the gain (the ``setx`` cases)
QUIET_ON_MUSIC = (PAIRS[9], PAIRS[11])
P40, P90, P25 = PAIRS[0], PAIRS[5], PAIRS[10]
assert (P40, P90, P25) == ((-40.0, 10.0), (-90.0, 10.0), (-25.0, 6.0))
IDLE = ((0.0, 1.0),) * 3

MIXED = ((P40, PAIRS[2], P90), (P90, PAIRS[1], P25), (PAIRS[3], PAIRS[4], PAIRS[6]),
         (PAIRS[7], PAIRS[8], P40), (PAIRS[11], P90, PAIRS[9]), (PAIRS[4], PAIRS[6], PAIRS[3]))
_rng = np.random.default_rng(20251)
DRAWN = tuple(tuple((float(_rng.uniform(-40.0, 0.0)), float(_rng.uniform(1.0, 10.0))) for _ in range(3))
              for _ in range(5))
TRIPLES = tuple((p,) * 3 for p in PAIRS) + MIXED + DRAWN
assert len(TRIPLES) == 23

RATES = (11025, 22050, 32000, 44100, 64000, 88200, 96000, 176400, 192000)
LEN_RATES = (22050, 44100, 48000)
CHUNK_LENGTHS = (1, 7, 21, 22, 23, 33, 45, 219, 220, 221, 241, 4799, 8193, 12001, 12023)
SPLITS = ((0, 0), (0, 1), (64, 2), (-1, -1))
ENV_FLOOR = 1024            # envelope segments are cut at multiples of 512 or 1024 frames here
DENORMAL = float.fromhex("0x0.df09e5c90a99p-1022")

CASES = {}


def _case(name, **kw):
    assert name not in CASES
    CASES[name] = dict(dict(lengths=LENGTHS, ch=2, extra={}, seed=400 + len(CASES)), **kw)
    return name


def _tag(triple):
    return "default" if triple == DEFAULT else "%g_%g" % triple[0] if len(set(triple)) == 1 else "mixed"


SET = [_case("set-%02d" % i, group="set", sig="tail", fs=(48000, 44100)[i % 2], triple=t)
       for i, t in enumerate(TRIPLES)]
# rms 16384 engages on dc's 30000 and on sq110's clipped bands; rms 32764.2 only where a band
# sits within two counts of full scale (alt's high band, r = 32765: 2e-4 dB over), not on dc
SETX = [_case("setx-%s-%s" % (sig, _tag((p,) * 3)), group="set", sig=sig, fs=fs, triple=(p,) * 3, expect=e)
        for sig, fs, p, e in (("dc", 44100, PAIRS[9], "most"), ("sq110+sq5k", 48000, PAIRS[9], "most"),
                              ("alt", 48000, PAIRS[11], "tiny"), ("dc", 44100, PAIRS[11], "none"))]
RATE = [_case("rate-%d-%s" % (fs, _tag(t)), group="rate", sig="tail", fs=fs, triple=t)
        for fs in RATES for t in (DEFAULT, (P40,) * 3)]
LEN = [_case("len-%d-%s" % (fs, _tag(t)), group="len", sig="music", fs=fs, triple=t, lengths=CHUNK_LENGTHS)
       for fs in LEN_RATES for t in (DEFAULT, (P40,) * 3)]
EDGE = [_case("edge-%s-%d-%s" % (s, fs, _tag((p,) * 3)), group="edge", sig=s, fs=fs, triple=(p,) * 3)
        for s in SIGNALS for fs in (48000, 96000) for p in (P40, P90, P25)]
CLAMP = [_case("clamp-%d-%s" % (fs, _tag(t)), group="clamp", sig="sq110+sq5k", fs=fs, triple=t,
               lengths=(12000, 12023))
         for fs in (22050, 44100, 48000, 96000) for t in (IDLE, (PAIRS[3],) * 3)]
CLAMP_EQ = _case("clamp-48000-width-eq", group="clamp", sig="sq110+sq5k", fs=48000, triple=IDLE,
                 lengths=(12000, 12023), extra=dict(VOCAL, width=1.3), loose=True)
SPLIT = [n for n in SET + EDGE if CASES[n]["triple"] in ((P40,) * 3, (P90,) * 3)]
assert len(SPLIT) == 2 + 32
DIV = [_case("div-%d-%s" % (fs, _tag(t)), group="div", sig="tail", fs=fs, triple=t)
       for fs in (48000, 96000) for t in (DEFAULT, (P40,) * 3)]
MC = [_case("mc%d-%s-%s" % (C, s, _tag(t)), group="mc", sig=s, fs=48000, triple=t, ch=C)
      for C in (3, 8) for t in (DEFAULT, (P40,) * 3, (P90,) * 3, IDLE) for s in ("am", "sq110+sq5k")]


def _settings(triple, extra=()):
    s = dict(multiband=True)
    for band, (t, r) in zip(("low", "mid", "high"), triple):
        s[band + "_thresh"], s[band + "_ratio"] = t, r
    s.update(extra)
    return s


def _look(fs):
    return int(5 * fs / 1000)


def _input(spec):
    from amx import synth
    fs, L = spec["fs"], spec["lengths"]
    if spec["sig"] == "tail":
        drop = L[0] + L[1] // 2
        x = synth.music_like(drop + int(1.5 * fs), fs, 2, seed=spec["seed"], peak_dbfs=-1.0)
        x[drop:] *= 1e-3
        x16 = synth.to_s16(x)
    elif spec["sig"] == "music":
        x16 = synth.to_s16(synth.music_like(sum(L), fs, 2, seed=spec["seed"], peak_dbfs=-1.0))
    else:
        x16 = edge_signal(spec["sig"], L, fs, spec["seed"], spec["ch"])
    cuts = np.concatenate([[0], np.cumsum(L)])
    return x16, [(int(cuts[k]), int(L[k])) for k in range(len(L))]


def _rms(band, look):
    """audioop.rms of the look frames before each frame (0 at frame 0), in exact integers"""
    sq = (band.astype(np.int64) ** 2).sum(axis=1)
    P = np.concatenate([[0], np.cumsum(sq)])
    i = np.arange(band.shape[0])
    lo = np.maximum(i - look, 0)
    S, cnt = P[i] - P[lo], band.shape[1] * (i - lo)
    r = np.floor(np.sqrt(S / np.maximum(cnt, 1))).astype(np.int64)
    return r + ((r + 1) ** 2 * cnt <= S) - (r * r * cnt > S)


def _sat(a):
    return np.clip(a, -32768, 32767)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the case's input, chunk cuts, settings and oracle output -- made once, shared by the
    precondition test and the GPU tests, and not modified by either -- and what the oracle
    says of the case (``facts``).  Asserts the case's preconditions on the oracle alone."""
    import oracle as O
    spec = CASES[name]
    fs, triple, group = spec["fs"], spec["triple"], spec["group"]
    x16, chunks = _input(spec)
    settings = _settings(triple, spec["extra"])
    facts = dict(rerun=False)
    if spec["ch"] > 2:
        ref = [O.chunk_mc(x16[s:s + n], fs, settings) for s, n in chunks]
        idle = [O.chunk_mc(x16[s:s + n], fs, _settings(IDLE)) for s, n in chunks]
        f = float(np.mean(np.concatenate(ref) != np.concatenate(idle)))
        assert (f == 0.0) if triple == IDLE else (f >= 0.30), "%s: the compressor changes %.4f" % (name, f)
    else:
        ref = [O.chunk(x16[s:s + n], fs, settings) for s, n in chunks]
        bands, comp, att = [[], [], []], [[], [], []], [[], [], []]
        clamp2 = 0
        for k, (s, n) in enumerate(chunks):
            f = O.eq(x16[s:s + n].astype(np.float32) / np.float32(32768.0), fs, settings)
            if settings.get("width", 1.0) != 1.0:
                f = O.width(f, settings["width"])
            bk = O.crossover(O.f32_to_s16(f), fs)
            ck = [O.compress(b, fs, t, r, trace=True) for b, (t, r) in zip(bk, triple)]
            # the band-level view below is the chain's: its overlay is the chunk's output
            assert np.array_equal(O.overlay3(*[c[0] for c in ck], fs), ref[k]), name
            for b in range(3):
                bands[b].append(bk[b])
                comp[b].append(ck[b][0])
                att[b].append(ck[b][1])
                if (ck[b][1][ENV_FLOOR - 1::ENV_FLOOR][:(n - 1) // ENV_FLOOR] != 0).any():
                    facts["rerun"] = True      # a segment's true start state is not the 0 it guesses
            if k == 0:
                lo, mid, hi = [c[0].astype(np.int32) for c in ck]
                clamp2 = int((_sat(_sat(lo + mid) + hi) != _sat(lo + mid + hi)).sum())
        changed = [float(np.mean(np.concatenate(comp[b]) != np.concatenate(bands[b]))) for b in range(3)]
        top = [float(np.max(np.concatenate(att[b]))) for b in range(3)]
        facts.update(changed=changed, top=top, clamp2=clamp2)
        assert min(int(np.concatenate(bands[b]).min()) for b in range(3)) >= -32767, name
        for b, p in enumerate(triple):
            if p in UNTOUCHED or p[1] == 1.0 or (p in QUIET_ON_MUSIC and spec["sig"] == "tail"):
                assert changed[b] == 0.0, "%s: band %d changed (%g) at %r" % (name, b, changed[b], p)
        if name in SETX:
            if spec["expect"] == "most":
                ok = max(changed) >= 0.30
            elif spec["expect"] == "none":
                ok = max(changed) == 0.0
            else:
                ok = max(changed) > 0.0 and 0.0 < max(top) < 1e-3
            assert ok, "%s: %r of the bands' samples change, attenuation %r dB" % (name, changed, top)
        elif group in ("set", "div") and len(set(triple)) == 1 and triple[0] not in UNTOUCHED + QUIET_ON_MUSIC:
            assert max(changed) >= 0.30, "%s: only %r of a band's samples change" % (name, changed)
            if triple[0] == P90:
                assert max(top) >= 60.0, "%s: attenuation reaches only %r dB" % (name, top)
            if triple[0] == PAIRS[8]:
                assert 0.0 < max(top) <= 0.01, "%s: attenuation %r dB" % (name, top)
        if group == "set" and len(set(triple)) > 1:
            assert max(changed) > 0.0, name
        if group == "rate":
            assert max(changed) >= 0.30, "%s: only %r of a band's samples change" % (name, changed)
        if group == "edge":
            sig, look = spec["sig"], _look(fs)
            # The detector's top.  No band of this chain can hold 32767 for a whole window: the
            # int16 -> float32 -> int16 step before the crossover scales by 32767 / 32768 and the
            # Butterworth bands have no gain, so 32767 comes only from overshoot (clipped, shorter
            # than 5 ms).  alt's high band sits at +-32765 (r = 32765); sq110's mid band clips on
            # thousands of samples with r over 30000
            if sig == "alt":
                assert max(int(_rms(c, look).max()) for c in bands[2]) >= 32765, name
            if sig == "sq110+sq5k":
                full = max(int((np.abs(np.concatenate(bands[b]).astype(np.int32)) == 32767).sum()) for b in range(3))
                assert full >= 1000 and max(int(_rms(c, look).max()) for c in bands[1]) >= 30000, (name, full)
            if sig == "noise_lo":
                assert max(int(_rms(c, look).max()) for b in range(3) for c in bands[b]) <= 3, name
                if triple[0] == P25:
                    assert max(changed) == 0.0, name
            if sig == "dc" and triple[0] == P90:
                assert changed[0] >= 0.99, "%s: %g of the low band changes" % (name, changed[0])
            if sig == "step":
                # r = 0 stretches, and a chunk whose frame 0 has energy (the cnt = 2 i head)
                assert any((_rms(c, look)[1:] == 0).sum() >= look for c in bands[0]), name
                assert any(np.abs(bands[b][1][0]).max() > 0 and _rms(bands[b][1], look)[1] > 0 for b in range(3)), name
            if sig in ("dc", "am", "step", "one_ch") and triple[0] == P90:
                assert max(top) >= 50.0, "%s: attenuation reaches only %r dB" % (name, top)
        if group == "clamp":
            assert max(changed) == 0.0, name
            # (the VOCAL EQ's negative bass shelf leaves the high band within +-56: with it the two
            # clamp orders agree everywhere, and the case only runs the overlay behind EQ and width)
            assert clamp2 >= (0 if spec["extra"] else 1000), "%s: the clamp order shows on %d samples" % (name, clamp2)
        if group == "len":
            out = [O.overlay_len(n, fs) for n in spec["lengths"]]
            grow = dict(zip(spec["lengths"], out))
            assert 0 in out and max(o - n for n, o in grow.items()) >= 9 and min(o - n for n, o in grow.items()) < 0
            if fs == 44100:
                assert (grow[8193], grow[12001], grow[12023]) == (8202, 11995, 12039)
            if fs == 48000:
                assert grow[12023] == 12000
    ref = np.concatenate(ref)
    ref.setflags(write=False)
    x16.setflags(write=False)
    return x16, chunks, settings, ref, facts


def test_matrix_reaches_every_window_form_and_setting():
    looks = [_look(fs) for fs in RATES]
    assert any(k <= 256 for k in looks) and any(256 < k <= 512 for k in looks) and any(512 < k <= 1024 for k in looks)
    assert {_look(64000), _look(88200), _look(176400)} == {320, 441, 882}
    assert sum(5 * fs % 1000 != 0 for fs in RATES) >= 3                    # A = 5 fs / 1000 fractional
    assert {CASES[n]["triple"] for n in SETX if CASES[n]["expect"] != "none"} == {(p,) * 3 for p in QUIET_ON_MUSIC}
    assert {CASES[n]["triple"] for n in SET[:12]} == {(p,) * 3 for p in PAIRS}
    for t in MIXED:
        assert len(set(t)) == 3
    for t in DRAWN:
        assert all(-40.0 <= a <= 0.0 and 1.0 <= r <= 10.0 and a != round(a) and r != round(r) for a, r in t)
    assert {CASES[n]["fs"] for n in SET} == {48000, 44100}
    assert len(CASES) == 23 + 4 + 18 + 6 + 48 + 9 + 4 + 16


@pytest.mark.parametrize("group", ["set", "rate", "len", "edge", "clamp", "div", "mc"])
def test_preconditions_on_the_oracle(oracle_mod, group):
    """the oracle half of every case of a group (no GPU): its preconditions hold"""
    names = [n for n in CASES if CASES[n]["group"] == group]
    assert names
    for n in names:
        _reference(n)
    if group == "edge":
        # the fix-up has work on the new regimes: some case of each kind needs a re-run
        assert sum(_reference(n)[4]["rerun"] for n in SPLIT) >= len(SPLIT) // 2


def _run(name, extra=()):
    x16, chunks, settings, ref, facts = _reference(name)
    settings = dict(settings, **dict(extra))
    if CASES[name]["ch"] > 2:
        return _mc_chain(x16, CASES[name]["fs"], settings, chunks), None
    return _chunk_chain(x16, CASES[name]["fs"], settings, chunks)


def _check(name, out, note=""):
    ref = _reference(name)[3]
    what = "compressor %s%s" % (name, note)
    if out.shape == ref.shape and out.size:
        d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
        bad = np.argwhere(d != 0)
        print("COMPRESSOR %s max|diff| %d differing %d of %d%s" % (
            what, d.max(), len(bad), d.size, " first at %s" % bad[0].tolist() if len(bad) else ""))
    if CASES[name].get("loose"):
        _cmp(out, ref, what)
    else:
        _cmp(out, ref, what, exact_min=1.0, tol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SET + SETX)
def test_settings_grid(gpu, oracle_mod, name):
    """1: the twelve pairs on every band, mixed triples, seeded draws over the GUI's range"""
    _check(name, _run(name)[0])


@pytest.mark.gpu
def test_ratio_zero_is_refused(gpu):
    """the reference divides by zero at ratio 0: the plan is refused with AMX_EINVAL"""
    from amx import capi
    from amx.engine import MasteringJob
    with pytest.raises(capi.AmxError, match=r"\(%d\).*ratio" % capi.AMX_EINVAL):
        MasteringJob(48000, 2, _settings((P40, (-20.0, 0.0), P25)), [4800], input_s16=True, chunks=[(0, 0, 4800)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", RATE)
def test_rates_and_window_forms(gpu, oracle_mod, name):
    """2: k_rms<256 | 512 | 1024> at nine rates, whole and fractional attack frame counts"""
    _check(name, _run(name)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", LEN)
def test_chunk_lengths(gpu, oracle_mod, name):
    """2: fifteen chunk lengths in one plan: 0 output frames, padded and cut chunks"""
    _check(name, _run(name)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE)
def test_detector_and_gain_edges(gpu, oracle_mod, name):
    """3: the detector's top and bottom, frame-0 energy, 50-80 dB and 1e-6 dB attenuations"""
    _check(name, _run(name)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLAMP + [CLAMP_EQ])
def test_overlay_clamp_order(gpu, oracle_mod, name):
    """4: clamp(clamp(lo + mid) + hi) where it differs from one clamp of the sum"""
    _check(name, _run(name)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("warm,rounds", SPLITS)
@pytest.mark.parametrize("name", SPLIT)
def test_work_split(gpu, oracle_mod, name, warm, rounds):
    """5: exact however the envelope's work is split, and the fix-up is seen working"""
    out, job = _run(name, dict(_env_warm=warm, _env_rounds=rounds))
    _check(name, out, " warm=%d rounds=%d" % (warm, rounds))
    ctr = job.env_counters()
    redone = sum(r["reruns"] + r["wide"] for r in ctr)
    facts = _reference(name)[4]
    if (warm, rounds) == (0, 0):
        assert redone == 0, "%s: no fix-up round, yet counters %r" % (name, ctr)
    if (warm, rounds) == (0, 1) and facts["rerun"]:
        assert redone > 0, "%s: segments start from a non-zero state, yet counters %r" % (name, ctr)


def _m_tables(triple):
    tabs = []
    for t, ratio in triple:
        thr = 32768.0 * 10.0 ** (t / 20.0)
        k = 1.0 - (1.0 / ratio)
        tabs.append(np.array([0.0] + [k * max(20 * (math.log(r / thr) / math.log(10)), 0) for r in range(1, 32769)]))
    return tabs


@pytest.mark.gpu
@pytest.mark.parametrize("name", DIV)
def test_division_form(gpu, oracle_mod, name):
    """6: env_div<true> and env_div<false>.  The plan checks the reciprocal form on every
    table value and divides plainly when one fails; entry 32768 (r = 32768 cannot occur: band
    samples are >= -32767) set to a denormal for which the check fails selects that form."""
    tabs = _m_tables(CASES[name]["triple"])
    keyless, job = _run(name)
    assert job.env_rcp() == 1
    _check(name, keyless)
    same, job = _run(name, dict(_comp_m_table=tabs))
    assert job.env_rcp() == 1 and np.array_equal(same, keyless), "%s: the tables restated in Python differ" % name
    for t in tabs:
        t[32768] = DENORMAL
    out, job = _run(name, dict(_comp_m_table=tabs))
    assert job.env_rcp() == 0, "%s: the plan kept the reciprocal form" % name
    _check(name, out, " plain division")


@pytest.mark.gpu
@pytest.mark.parametrize("name", MC)
def test_three_to_eight_channels(gpu, oracle_mod, name):
    """8: k_mc_rms and k_mc_gain_overlay at C = 3 and 8 against oracle.chunk_mc"""
    _check(name, _run(name)[0])
