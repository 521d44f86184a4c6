"""GPU: the stereo gain and limiter stage (k_final<UNIT>, csrc/amx_final.hip), one stage at a
time.

A known int16 signal is put straight into a MasteringJob's chain output (the chain is
bypassed), the gains, decision words, halo and carried limiter state are set by hand, and
finalize() runs on it alone.  The result is held to oracle.alimiter(oracle.linear_gain(x, g))
bit for bit: the int16 output, and on the general path the attenuation trace
(amx_plan_set_limiter_trace) as bit patterns.  There is no tolerance anywhere in this file.

The cases are tests/limiter_cases.py's; tests/test_limiter_cases.py asserts their
preconditions on the oracle alone.  Groups, by the letter that starts a test id:
  A  general limiter x parameter sets (both k_final instantiations: ...-unit / ...-general),
     rates 8 .. 384 kHz (the 384 kHz ring needs more than 64 KiB of LDS), signals and gains
  B  segment lengths, warm-ups, segment counts about the walker's 64-boundary batches, more
     segments than blocks; the refused geometries
  C  the idle path: every window r of its vector form, both offset alignments, against the
     oracle and against the general path
  D  spans that start inside a track: halo, carried state over 2..4 spans, from_rest
  E  one job run three times: the re-armed counter, old segment slots and traces

Not pinned here: the walker's live-list comparison (its st == 2 path and lim_equal's loop) and
the strictness of `d < delta` in lim_seq.  Kernels mutated there pass every case of this file.
scripts/lim_guess_sweep.py (a host model of guess against truth, 1.7 M guesses over these
signals) found no guess equal to the truth in its scalars and unequal in its list, and no frame
on which `d <= delta` changes the trace; DESIGN.md section 3.5 has the table.
"""
import numpy as np
import pytest

import limiter_cases as lc

pytestmark = pytest.mark.gpu

CTL_GENERAL, CTL_IDLE = 0, 1          # AMX_CTL_FAST


def _cmp(got, ref, what):
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    if got.size == 0:
        return
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32)).max(axis=1)
    bad = np.flatnonzero(d)
    assert bad.size == 0, "%s: %d of %d frames differ (max %d LSB), first at %d: %r vs %r" % (
        what, bad.size, d.size, d.max(), bad[0], got[bad[0]], ref[bad[0]])


def _cmp_att(att, ref, what):
    """the attenuation traces as bit patterns"""
    assert att.shape == ref.shape, "%s: att shape %s vs %s" % (what, att.shape, ref.shape)
    bad = np.nonzero(att.view(np.int64) != ref.view(np.int64))[0]
    assert bad.size == 0, "%s: att differs on %d of %d frames, first %d: %r vs %r" % (
        what, bad.size, att.size, bad[0], att[bad[0]], ref[bad[0]])


class Stage:
    """a MasteringJob reduced to its final stage: one span per entry of `lengths`"""

    def __init__(self, fs, params, lengths, LS=0, W=-1, frame0=None, total=None, trace=False):
        import torch
        from amx import capi
        from amx.engine import MasteringJob
        lengths = [int(n) for n in lengths]
        chunks, off = [], 0
        for t, n in enumerate(lengths):
            chunks.append((t, off, n))
            off += n
        lim = {k: params[k] for k in ("limit", "attack", "release", "level_in", "level_out")}
        job = MasteringJob(fs, 2, {"lufs": None}, lengths, input_s16=True, chunks=chunks, measure_only=True,
                           limiter=lim, limiter_seg_frames=LS, limiter_warm_frames=W,
                           track_frame0=frame0, track_total=total)
        self.job, self.n, self.lengths = job, off, lengths
        job.fd.level_in, job.fd.level_out = params["level_in"], params["level_out"]
        job.fd.auto_level = 1 if params["auto_level"] else 0
        assert job.info.out_frames == off and job.bs // 2 == lc.ring_frames(fs, params)
        assert job.halo_frames == job.bs // 2 - 1
        self.offsets = [int(s.out_offset) for s in job.spans]
        assert [int(s.out_frames) for s in job.spans] == lengths
        self.att = None
        if trace:
            self.att = torch.empty((off,), dtype=torch.float64, device=job.device)
            capi.check(capi.load().amx_plan_set_limiter_trace(job.plan.h, capi.ptr(self.att)),
                       "amx_plan_set_limiter_trace")

    def run(self, tracks, gains=None, fast=False, ctl=None, halos=None, state=None, from_rest=False):
        """-> (per-track int16 outputs, per-track traces or None).  fast None: per track ctl"""
        import torch
        job = self.job
        x = np.ascontiguousarray(np.concatenate(tracks))
        assert x.shape == (self.n, 2) and x.dtype == np.int16
        job.out[:self.n].copy_(torch.from_numpy(x))
        job.y.fill_(0x5a5a)
        g = [-1.0] * len(tracks) if gains is None else list(gains)
        job.gains.copy_(torch.tensor(g, dtype=torch.float64))
        if ctl is not None:
            job.ctl.copy_(torch.tensor(list(ctl), dtype=torch.int32))
        if halos is not None:
            job.halo.copy_(torch.from_numpy(np.ascontiguousarray(np.stack(halos))))
        if state is not None:
            job.lim_state.copy_(state)
        if self.att is not None:
            self.att.fill_(float("nan"))
        job.finalize(fast=fast, from_rest=from_rest)
        torch.cuda.synchronize()
        y = job.y[:self.n].cpu().numpy()
        att = self.att.cpu().numpy() if self.att is not None else None
        cut = lambda a: [a[o:o + n].copy() for o, n in zip(self.offsets, self.lengths)]
        return cut(y), (cut(att) if att is not None else None)

    def close(self):
        self.job.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _general_vs_oracle(O, x16, fs, params, gain, what, LS=0, W=-1, trace=True):
    ref, att = lc.reference(O, x16, fs, params, gain)
    with Stage(fs, params, [x16.shape[0]], LS=LS, W=W, trace=trace) as st:
        y, a = st.run([x16], [gain], fast=False)
    _cmp(y[0], ref, what)
    if trace:
        _cmp_att(a[0], att, what)
    return ref, att


# ------------------------------------------------------------------------------ group A
@pytest.mark.parametrize("case", lc.a_cases(), ids=lc.a_id)
def test_general_limiter(gpu, oracle_mod, case):
    """every signal x parameter set at 44.1 and 48 kHz, bursts and am at every rate, every gain
    at 48 kHz: output and trace are the oracle's.  Where no int16 input can reach the limit
    (the reference's set with gain 0.5 or -3.2 dB) the idle path must give the same bytes"""
    s, p, fs, g = case
    params, gain = lc.PARAMS[p], lc.GAINS[g]
    x16 = lc.a_signal(case)
    ref, _ = _general_vs_oracle(oracle_mod, x16, fs, params, gain, lc.a_id(case))
    if not lc.can_engage(params, gain):
        with Stage(fs, params, [x16.shape[0]]) as st:
            _cmp(st.run([x16], [gain], fast=True)[0][0], ref, lc.a_id(case) + " idle path")


def test_large_lds_ring_384k(gpu, oracle_mod):
    """384 kHz: B = 1920 frames, a 94 KiB ring (over the 64 KiB a kernel gets unasked), on the
    general path with two segments and no warm-up"""
    fs, params = 384000, lc.PARAMS["ref"]
    B = lc.ring_frames(fs, params)
    assert (3 * 2 * B + 4 * 64) * 8 > 64 * 1024
    x16 = lc.signal("bursts", 5 * B + 7, fs, params, seed=6)
    _general_vs_oracle(oracle_mod, x16, fs, params, -1.0, "384 kHz", LS=2 * B + 100, W=0)


# ------------------------------------------------------------------------------ group B
@pytest.mark.parametrize("case", lc.b_cases(), ids=lc.b_id)
def test_segments_and_walker(gpu, oracle_mod, case):
    """segment lengths from the smallest allowed to one segment, warm-ups from none to three
    releases, 1 .. 130 segments (the walker checks 64 boundaries per step) and 2051 segments
    on 2048 blocks: whatever the guesses, the walker leaves the oracle's output and trace"""
    s, fs, LS, W, n = case
    _general_vs_oracle(oracle_mod, lc.b_signal(case), fs, lc.PARAMS["ref"], -1.0, lc.b_id(case), LS=LS, W=W)


def test_refused_geometries(gpu):
    """segments under 64 frames or under the ring, and a ring too large for a CU's LDS, come
    back as AMX_EINVAL / AMX_ERANGE from amx_limiter_prepare; nothing is launched after them"""
    import ctypes
    from amx import capi
    L = capi.load()
    with Stage(48000, lc.PARAMS["ref"], [4096]) as st:          # B = 240
        fd = st.job.fd
        for LS in (63, 1, 239, 128):
            assert L.amx_limiter_prepare(st.job.plan.h, ctypes.byref(fd), LS, -1) == capi.AMX_EINVAL, LS
        assert L.amx_limiter_prepare(st.job.plan.h, ctypes.byref(fd), 240, -1) == capi.AMX_OK
    with Stage(8000, lc.PARAMS["ref"], [4096]) as st:           # B = 40
        assert L.amx_limiter_prepare(st.job.plan.h, ctypes.byref(st.job.fd), 40, -1) == capi.AMX_EINVAL
        assert L.amx_limiter_prepare(st.job.plan.h, ctypes.byref(st.job.fd), 64, -1) == capi.AMX_OK
    with Stage(384000, lc.PARAMS["ref"], [4096]) as st:
        fd = capi.FinalDesc.from_buffer_copy(st.job.fd)
        fd.attack_ms = 10.0                                    # 7680 samples: 186 KiB
        assert L.amx_limiter_prepare(st.job.plan.h, ctypes.byref(fd), 0, -1) == capi.AMX_ERANGE
    with pytest.raises(capi.AmxError):
        Stage(48000, lc.PARAMS["ref"], [4096], LS=100)


# ------------------------------------------------------------------------------ group C
def _both_paths(O, st, tracks, gains, fs, params, what):
    """oracle trace all ones (the premise), fast=True equals the oracle, fast=False the same"""
    refs = []
    for x16, g in zip(tracks, gains):
        ref, att = lc.reference(O, x16, fs, params, g)
        assert (att == 1.0).all(), what + ": the oracle's limiter moves"
        refs.append(ref)
    idle, _ = st.run(tracks, gains, fast=True)
    for t, ref in enumerate(refs):
        _cmp(idle[t], ref, "%s idle path track %d" % (what, t))
    gen, _ = st.run(tracks, gains, fast=False)
    for t, ref in enumerate(refs):
        _cmp(gen[t], idle[t], "%s general path vs idle path track %d" % (what, t))


@pytest.mark.parametrize("case", lc.c_cases(), ids=lc.c_id)
def test_idle_path(gpu, oracle_mod, case):
    """final_fast_block at every window r = (4 - (h & 3)) & 3 of its 16-byte loads, lengths
    about the ring and about its 2048-frame blocks, both instantiations, three gains, and a
    peak exactly on the limit and one step under it"""
    fs, n, p, g, below = case
    params = lc.PARAMS[p]
    x16 = lc.c_signal(oracle_mod, case)
    with Stage(fs, params, [n]) as st:
        assert (4 - (st.job.halo_frames & 3)) & 3 == lc.C_WINDOW[fs]
        _both_paths(oracle_mod, st, [x16], [lc.GAINS[g]], fs, params, lc.c_id(case))


BATCH = (4100, 4097, 3 * 2048 + 5)


@pytest.mark.parametrize("fs", lc.C_RATES[:5], ids=["C-batch-%d-r%d" % (fs, lc.C_WINDOW[fs]) for fs in lc.C_RATES[:5]])
def test_idle_path_batch_offsets(gpu, oracle_mod, fs):
    """three tracks in one launch: the offsets 0 and 4100 are multiples of 4, 8197 is not (its
    interior blocks must take the edge form).  All idle, by both paths; then idle and general
    tracks mixed through the decision words, both ways round"""
    params = lc.PARAMS["ref"]
    lo, hi = lc.allowed_range(oracle_mod, params)
    q = [lc.quiet(n, fs, lo, hi, seed=10 + t) for t, n in enumerate(BATCH)]
    loud = [lc.signal("bursts", n, fs, params, seed=20 + t) for t, n in enumerate(BATCH)]
    with Stage(fs, params, BATCH, LS=1000, W=0) as st:
        offs = [int(st.job.plan.span(t).out_offset) for t in range(3)]
        assert any(o % 4 == 0 for o in offs[1:]) and any(o % 4 for o in offs), offs
        _both_paths(oracle_mod, st, q, [-1.0] * 3, fs, params, "batch %d" % fs)
        for ctl in ((CTL_IDLE, CTL_GENERAL, CTL_IDLE), (CTL_GENERAL, CTL_IDLE, CTL_GENERAL)):
            tracks = [q[t] if ctl[t] == CTL_IDLE else loud[t] for t in range(3)]
            y, _ = st.run(tracks, [-1.0] * 3, fast=None, ctl=ctl)
            for t in range(3):
                ref, att = lc.reference(oracle_mod, tracks[t], fs, params)
                assert (att != 1.0).any() == (ctl[t] == CTL_GENERAL)
                _cmp(y[t], ref, "batch %d ctl %r track %d" % (fs, ctl, t))


# ------------------------------------------------------------------------------ group D
_d_cache = {}


def _d_setup(O, fs, p):
    """the signal, the oracle's one-shot output and trace, and the cut points, once"""
    if (fs, p) not in _d_cache:
        x16 = lc.d_signal(fs, p)
        ref, att = lc.reference(O, x16, fs, lc.PARAMS[p])
        ref.setflags(write=False)
        att.setflags(write=False)
        _d_cache[(fs, p)] = (x16, ref, att, lc.d_points(att, lc.ring_frames(fs, lc.PARAMS[p])))
    return _d_cache[(fs, p)]


def _halo(x16, cut, h):
    """the h frames before `cut`; frames before the track are silence"""
    out = np.zeros((h, 2), np.int16)
    k = min(h, cut)
    if k:
        out[h - k:] = x16[cut - k:cut]
    return out


def _run_spans(x16, fs, params, cuts, fast, LS=0, W=-1, trace=False):
    """one job per span; the state a span leaves enters the next (general path)"""
    N = x16.shape[0]
    edges = [0] + list(cuts) + [N]
    ys, atts, state = [], [], None
    for a, b in zip(edges[:-1], edges[1:]):
        with Stage(fs, params, [b - a], LS=LS, W=W, frame0=[a], total=[N], trace=trace) as st:
            y, att = st.run([x16[a:b]], fast=fast, halos=[_halo(x16, a, st.job.halo_frames)], state=state)
            state = st.job.lim_state.clone()
        ys.append(y[0])
        if trace:
            atts.append(att[0])
    return np.concatenate(ys), (np.concatenate(atts) if trace else None)


@pytest.mark.parametrize("LS,W", [(0, -1), (256, 0)], ids=["one-segment", "LS256-W0"])
@pytest.mark.parametrize("name", lc.D_CUTS)
@pytest.mark.parametrize("fs,p", lc.D_SETUPS, ids=["D-%d-%s" % s for s in lc.D_SETUPS])
def test_spans_carried_state(gpu, oracle_mod, fs, p, name, LS, W):
    """a track cut into 2, 3 or 4 spans (inside an active stretch, at rest, first spans shorter
    than the halo, cuts under a ring apart), each its own job with the halo and the state the
    span before left: the pieces are the oracle's one-shot output and trace"""
    x16, ref, att, pts = _d_setup(oracle_mod, fs, p)
    cuts = lc.d_cuts(name, pts, lc.ring_frames(fs, lc.PARAMS[p]))
    y, a = _run_spans(x16, fs, lc.PARAMS[p], cuts, fast=False, LS=LS, W=W, trace=True)
    _cmp(y, ref, "spans %s" % cuts)
    _cmp_att(a, att, "spans %s" % cuts)


@pytest.mark.parametrize("name", lc.D_CUTS)
@pytest.mark.parametrize("fs,p", lc.D_SETUPS, ids=["D-%d-%s" % s for s in lc.D_SETUPS])
def test_spans_idle_signal_both_paths(gpu, oracle_mod, fs, p, name):
    """the same cuts on a signal that never reaches the limit: the idle path (halo only) and
    the general path (carried state) both give the oracle's one-shot output"""
    params = lc.PARAMS[p]
    lo, hi = lc.allowed_range(oracle_mod, params)
    x16 = lc.quiet(lc.D_FRAMES, fs, lo, hi, seed=30)
    ref, att = lc.reference(oracle_mod, x16, fs, params)
    assert (att == 1.0).all()
    cuts = lc.d_cuts(name, _d_setup(oracle_mod, fs, p)[3], lc.ring_frames(fs, params))
    _cmp(_run_spans(x16, fs, params, cuts, fast=True)[0], ref, "idle spans %s" % cuts)
    _cmp(_run_spans(x16, fs, params, cuts, fast=False)[0], ref, "general spans %s" % cuts)


@pytest.mark.parametrize("stale", [False, True], ids=["zero-state", "stale-state"])
@pytest.mark.parametrize("fs,p", lc.D_SETUPS, ids=["D-%d-%s" % s for s in lc.D_SETUPS])
def test_span_from_rest(gpu, oracle_mod, fs, p, stale):
    """from_rest: a span cut where the limiter rests and the halo is under the limit starts
    from its halo alone, equal to the oracle run from the halo's first frame; a state left
    in the buffer (here: the end state of another span, marked valid) is not read"""
    params = lc.PARAMS[p]
    x16, ref, att, pts = _d_setup(oracle_mod, fs, p)
    cut, N = pts["rest"], x16.shape[0]
    with Stage(fs, params, [N - cut], LS=1000, frame0=[cut], total=[N], trace=True) as st:
        h = st.job.halo_frames
        want, want_att = lc.reference(oracle_mod, x16[cut - h:], fs, params)
        state = None
        if stale:
            st.run([lc.signal("square", N - cut, fs, params)], fast=False, halos=[_halo(x16, 0, h)])
            state = st.job.lim_state.clone()
            assert float(state[0, 5]) == 1.0 and float(state[0, 0]) != 1.0     # valid, mid-attenuation
        y, a = st.run([x16[cut:]], fast=False, halos=[_halo(x16, cut, h)], state=state, from_rest=True)
    _cmp(y[0], want[h:], "from_rest")
    _cmp_att(a[0], want_att[h:], "from_rest")
    _cmp(y[0], ref[cut:], "from_rest vs one shot")


# ------------------------------------------------------------------------------ group E
def test_rerun_rearmed_counter_nothing_stale(gpu, oracle_mod):
    """one job, three runs, new signals and new decision words per track each time (general,
    idle, general and the reverse): each output is the oracle's on that input alone.  With no
    warm-up every active boundary needs the walker, which only runs if the run before re-armed
    the finished-block counter; old segment records and trace values must not show"""
    fs, params = 48000, lc.PARAMS["ref"]
    lengths = (9000, 5003, 12001)
    lo, hi = lc.allowed_range(oracle_mod, params)
    with Stage(fs, params, lengths, LS=256, W=0, trace=True) as st:
        for run in range(3):
            ctl = [CTL_GENERAL if (run + t) % 2 == 0 else CTL_IDLE for t in range(3)]
            tracks = [lc.signal(("bursts", "am", "square")[(run + t) % 3], n, fs, params, seed=40 + run) if c == CTL_GENERAL
                      else lc.quiet(n, fs, lo, hi, seed=50 + run + t) for t, (n, c) in enumerate(zip(lengths, ctl))]
            y, a = st.run(tracks, fast=None, ctl=ctl)
            for t in range(3):
                ref, att = lc.reference(oracle_mod, tracks[t], fs, params)
                assert (att != 1.0).any() == (ctl[t] == CTL_GENERAL)
                _cmp(y[t], ref, "run %d track %d" % (run, t))
                if ctl[t] == CTL_GENERAL:
                    _cmp_att(a[t], att, "run %d track %d" % (run, t))
