"""CPU: the preconditions of tests/test_gpu_final_stage.py's cases (tests/limiter_cases.py),
asserted from the oracle's output and attenuation trace alone: the limiter engages, segment
boundaries fall inside active stretches no warm-up can span and (but for the square) at rest,
the idle-path inputs never move the attenuation, and the cut points of group D are what
their names say.  No case is skipped."""
import numpy as np
import pytest

import limiter_cases as lc


def _engaged(att):
    return float((att < 1.0).mean())


@pytest.mark.parametrize("case", lc.a_cases(), ids=lc.a_id)
def test_a_limiter_engages(oracle_mod, case):
    s, p, fs, g = case
    x16 = lc.a_signal(case)
    assert x16.shape == (lc.a_length(fs, lc.PARAMS[p]), 2) and x16.shape[0] <= 23040
    _, att = lc.reference(oracle_mod, x16, fs, lc.PARAMS[p], lc.GAINS[g])
    if lc.can_engage(lc.PARAMS[p], lc.GAINS[g]):
        assert _engaged(att) >= 0.01, "engaged on %.2f %% of the frames" % (100 * _engaged(att))
    else:
        # no int16 input reaches the limit after this gain (0.98 x 32768 > 32768 g): the case
        # holds the general path to the idle result instead
        assert lc.GAINS[g] in (0.5, lc.GAINS["-3.2dB"]) and p == "ref"
        assert (att == 1.0).all()


def test_a_covers_both_instantiations_and_every_rate():
    cases = lc.a_cases()
    assert {lc.is_unit(lc.PARAMS[c[1]]) for c in cases} == {True, False}
    assert {c[2] for c in cases} == set(lc.RATES)
    assert lc.is_unit(lc.PARAMS["unit-edge"]) and not lc.is_unit(lc.PARAMS["unit-over"])
    assert lc.ring_frames(44100, lc.PARAMS["att0.7"]) == 30        # 61.74 samples: a ring under 64 frames
    assert (3 * 2 * lc.ring_frames(384000, lc.PARAMS["ref"]) + 256) * 8 > 64 * 1024


def test_ramps_are_strictly_monotone_past_two_search_steps():
    """the over-limit part of a ramp changes every frame for more than 2 x 64 frames"""
    for name, sgn in (("ramp_up", -1), ("ramp_down", 1)):
        x = lc.signal(name, 4096, 48000, lc.PARAMS["ref"], seed=1).astype(np.int64)
        thr = lc.threshold(lc.PARAMS["ref"])
        peak = np.abs(x).max(axis=1)
        step = np.sign(np.diff(peak)) == -sgn              # ramp_up: growing magnitudes
        over = (peak[1:] > thr) & (peak[:-1] > thr) & step
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], over.view(np.int8), [0]]))))[0::2]
        assert runs.max() > 128, (name, runs.max())


@pytest.mark.parametrize("case", lc.b_cases(), ids=lc.b_id)
def test_b_boundaries(oracle_mod, case):
    s, fs, LS, W, n = case
    B = lc.ring_frames(fs, lc.PARAMS["ref"])
    assert LS >= 64 and LS >= B
    x16 = lc.b_signal(case)
    _, att = lc.reference(oracle_mod, x16, fs, lc.PARAMS["ref"])
    assert _engaged(att) >= 0.01
    bnd = lc.b_boundaries(case)
    if bnd.size == 0:
        return
    active = [int(b) for b in bnd if att[b] != 1.0]
    assert active, "no boundary inside an active stretch"
    if W >= 0:
        # the limiter is never at rest in the W frames before the boundary (which lie inside
        # the span): a warm-up that starts at rest guesses wrong and the walker must repair
        hard = [b for b in active if b - W >= 1 and (att[b - W:b + 1] != 1.0).all()]
        assert hard, "every active boundary has a frame at rest within %d frames before it" % W
    if s != "square" and bnd.size >= 2:
        assert any(att[b] == 1.0 and att[b - 1] == 1.0 for b in bnd), "no boundary at rest"


def test_b_covers_the_walker_batches():
    cases = lc.b_cases()
    for fs in lc.B_RATES:
        B = lc.ring_frames(fs, lc.PARAMS["ref"])
        mine = [c for c in cases if c[1] == fs]
        counts = {-(-c[4] // c[2]) for c in mine}
        assert {1, 2, 64, 65, 66, 129, 130} <= counts
        assert {c[3] for c in mine} == set(lc.b_warms(fs))
        assert {c[2] for c in mine} == {max(64, B), 256, 1000, 16384}
        assert any(c[4] % c[2] for c in mine) and any(c[4] < 64 for c in mine)
    assert lc.LONG_CASE in cases and -(-lc.LONG_CASE[4] // lc.LONG_CASE[2]) > 2048     # AMX_LIM_MAX_BLOCKS


@pytest.mark.parametrize("case", lc.c_cases(), ids=lc.c_id)
def test_c_trace_is_all_ones(oracle_mod, case):
    fs, n, p, g, below = case
    B = lc.ring_frames(fs, lc.PARAMS[p])
    assert lc.C_WINDOW[fs] == (4 - ((B - 1) & 3)) & 3
    x16 = lc.c_signal(oracle_mod, case)
    assert x16.shape == (n, 2)
    g16 = oracle_mod.linear_gain(x16, lc.GAINS[g]) if lc.GAINS[g] > 0 else x16
    top = (np.abs(g16.astype(np.float64)).max() * (1.0 / 32768.0)) * lc.PARAMS[p]["level_in"]
    _, att = lc.reference(oracle_mod, x16, fs, lc.PARAMS[p], lc.GAINS[g])
    assert (att == 1.0).all()
    if p == "limit-exact":
        assert top * 32768.0 == (32111.0 if below else 32112.0)
    if not below:
        # clipped beforehand to the raw values the gain leaves at or under the limit, and
        # touching both ends: one raw step more would be over it (or is no int16 value)
        lo, hi = lc.allowed_range(oracle_mod, lc.PARAMS[p], lc.GAINS[g])
        assert int(x16.max()) == hi and int(x16.min()) == lo
        assert g != "1.7" or lo > -32768


def test_c_covers_every_window():
    assert {lc.C_WINDOW[fs] for fs in lc.C_RATES} == {0, 1, 2, 3}
    assert {lc.is_unit(lc.PARAMS[c[2]]) for c in lc.c_cases()} == {True, False}


@pytest.mark.parametrize("fs,p", lc.D_SETUPS, ids=["D-%d-%s" % s for s in lc.D_SETUPS])
def test_d_cut_points(oracle_mod, fs, p):
    B = lc.ring_frames(fs, lc.PARAMS[p])
    x16 = lc.d_signal(fs, p)
    _, att = lc.reference(oracle_mod, x16, fs, lc.PARAMS[p])
    assert _engaged(att) >= 0.01
    pts = lc.d_points(att, B)
    a, r, r2 = pts["active"], pts["rest"], pts["rest2"]
    assert (att[a - 1:a + B + 1] != 1.0).all(), "the active cut and the one B - 3 frames on lie in one active stretch"
    assert (att[r - B:r + 1] == 1.0).all() and (att[r2 - B:r2 + 1] == 1.0).all()
    # from_rest: the halo frames before the resting cut are all under the limit
    peak = np.abs(x16[r - (B - 1):r].astype(np.float64)).max() * (1.0 / 32768.0) * lc.PARAMS[p]["level_in"]
    assert peak <= lc.PARAMS[p]["limit"]
    for name in lc.D_CUTS:
        cuts = lc.d_cuts(name, pts, B)
        assert cuts == sorted(set(cuts)) and 0 < cuts[0] and cuts[-1] < lc.D_FRAMES and 2 <= len(cuts) + 1 <= 4
    assert {len(lc.d_cuts(n, pts, B)) for n in lc.D_CUTS} == {1, 2, 3}
