"""GPU: every EQ stage combination and shelf sign through every front of the chunk chain.

The four EQ gains pick, at plan time, which kernel instantiations a master runs.  The
non-zero stages form a mask (bit 0 bass shelf, 1 mid peak, 2 presence peak, 3 treble shelf)
and the mask fixes the state dimension D = 2 per shelf + 8 per peak.  launch_front1 and
launch_scan switch over the nine D, launch_front2 over the sixteen masks, and eq_tile /
eq_state_load / eq_chain (amx_dev.hpp) hold mask-dependent code: the two peaks' shared
loop body, the lone presence stage's state slot, the running coefficient offset, and the
negative shelf's  x g + (y - x g)  whose first product is float32 only on the first
active stage.  So the matrix is 36 (mask, bass sign, treble sign) cases times the fronts:

  variant  input            analog  width  multiband  seg   first kernel(s)            cases
  A        int16 stereo     off     1.3    on         128   k_front1<D,1,false>        36
  A192     the same at 192 kHz (the scan's longest window)                             masks 6 7 14
  B        float32 stereo   40      off    off        128   k_analog_h + k_gemv16<D>   36
  C        int16 mono       70      0.7    on         256   k_front1<D,1,true>         16 masks
  D        float32 stereo   off     off    off        128   k_front1s<D,false>         16 masks
  E        float32, AMX_F1=2  100   off    off        128   k_front1s<D,true>          one mask per D
  MC       int16, 3 channels  off   -      off / on   128   the stream (SC) chain      16 masks x 2

Every stereo case is three uneven chunks of more than 2048 frames (two scan blocks each),
every 3-channel case two chunks; the oracle runs per chunk.  The comparison is the
multi-chunk one of test_gpu_parity.py (3 LSB, 0.9999 exact).

What a case must be able to show is asserted on the ORACLE ALONE, before any GPU result
is looked at (``_reference``; ``test_preconditions_on_the_oracle`` runs that half without
a GPU): removing any one active EQ stage changes at least 10 % of the oracle's output
samples, and where the multiband compressor is on it changes at least 1 % of them.
"""
import functools
import itertools

import numpy as np
import pytest

from test_gpu_multichannel import _chain as _mc_chain
from test_gpu_parity import MB, _chunk_chain, _cmp

KEYS = ("bass_boost", "mid_cut", "presence_boost", "treble_boost")
GAIN = dict(bass_boost=3.0, mid_cut=4.0, presence_boost=2.5, treble_boost=2.0)
RATES = (44100, 48000, 96000)
STAGE_MIN = 0.10        # removing an active stage changes at least this share of samples
MB_MIN = 0.01           # so does the compressor, where it is on

# the 36 (mask, bass sign, treble sign) cases; a mask's first entry has every shelf positive
CASES36 = [(m,) + s for m in range(16)
           for s in itertools.product(*[(1, -1) if m & b else (0,) for b in (1, 8)])]
assert len(CASES36) == 36


def _dim(mask):
    return sum((2, 8, 8, 2)[b] for b in range(4) if mask >> b & 1)


def _signed(mask, sb, st):
    """one entry per mask: the signs given, on the shelves the mask has"""
    return mask, sb if mask & 1 else 0, st if mask & 8 else 0


VARIANTS = {
    "A": dict(inp="s16", seg=128, extra=dict(width=1.3, **MB), cases=CASES36),
    "B": dict(inp="f32", seg=128, extra=dict(analog_character=40.0), cases=CASES36),
    # C and D: shelf signs that A does not take first (a lone shelf negative)
    "C": dict(inp="mono", seg=256, extra=dict(analog_character=70.0, width=0.7, **MB),
              cases=[_signed(m, -1, 1) if m & 1 and m & 8 else _signed(m, -1, -1) for m in range(16)]),
    "D": dict(inp="f32", seg=128, extra={},
              cases=[_signed(m, 1, -1) if m & 1 and m & 8 else _signed(m, -1, -1) for m in range(16)]),
    "E": dict(inp="f32", seg=128, extra=dict(analog_character=100.0), env={"AMX_F1": "2"},
              cases=[_signed(m, -1, -1) for m in (0, 1, 9, 2, 3, 13, 6, 7, 15)]),
    # 192 kHz: D 16 / 18 with more window powers than the down sweep stages in LDS
    "A192": dict(inp="s16", seg=128, extra=dict(width=1.3, **MB), fs=192000, first=36,
                 cases=[_signed(m, -1, -1) for m in (6, 7, 14)]),
    "MC": dict(inp="mc", seg=128, extra={}, cases=[_signed(m, 1, -1) for m in range(16)]),
    "MCmb": dict(inp="mc", seg=128, extra=dict(MB), first=16,
                 cases=[_signed(m, -1, 1) for m in range(16)]),
}


def _params(v):
    V = VARIANTS[v]
    out = []
    for k, (mask, sb, st) in enumerate(V["cases"]):
        i = V.get("first", 0) + k
        fs = V.get("fs", RATES[i % 3])
        out.append(pytest.param(v, i, mask, sb, st, fs,
                                id="%s-m%02d-b%s-t%s-%d" % (v, mask, "0+-"[sb], "0+-"[st], fs)))
    return out


def _settings(mask, sb, st, extra):
    s = {k: GAIN[k] for b, k in enumerate(KEYS) if mask >> b & 1}
    if sb < 0:
        s["bass_boost"] = -s["bass_boost"]
    if st < 0:
        s["treble_boost"] = -s["treble_boost"]
    s.update(extra)
    return s


def _oracle_chunks(O, mc, x16, fs, settings, chunks):
    return [(O.chunk_mc if mc else O.chunk)(x16[s:s + m], fs, settings) for s, m in chunks]


def _changed(a, b):
    """share of differing samples over the chunks' common frames (the compressor's overlay
    rounds a chunk's length to whole milliseconds)"""
    diff = size = 0
    for p, q in zip(a, b):
        k = min(p.shape[0], q.shape[0])
        diff += int((p[:k] != q[:k]).sum())
        size += p[:k].size
    return diff / size


@functools.lru_cache(maxsize=None)
def _reference(v, i, mask, sb, st, fs):
    """the case's input, chunks, settings and oracle output -- made once, shared by the
    precondition test and the GPU test, and not modified by either.  Asserts, on the oracle
    alone, that the case can tell a skipped or misrouted stage from a right one."""
    import oracle as O
    from amx import synth
    V = VARIANTS[v]
    mc = V["inp"] == "mc"
    settings = _settings(mask, sb, st, V["extra"])
    seed = 1000 * (1 + sorted(VARIANTS).index(v)) + i
    if mc:
        n = 3100 + 37 * i
        cuts = [0, n // 2 + 3, n]
        assert min(np.diff(cuts)) >= 1500
    else:
        n = 7001 + 113 * i
        cuts = [0, n // 3 + 17, 2 * n // 3 - 5, n]
        assert min(np.diff(cuts)) > 2048
    chunks = [(cuts[k], cuts[k + 1] - cuts[k]) for k in range(len(cuts) - 1)]
    ch = 3 if mc else 1 if V["inp"] == "mono" else 2
    x16 = synth.to_s16(synth.music_like(n, fs, ch, seed=seed, peak_dbfs=-3.0))
    ref = _oracle_chunks(O, mc, x16, fs, settings, chunks)
    what = "%s mask %d bass %+d treble %+d fs %d" % (v, mask, sb, st, fs)
    for b, k in enumerate(KEYS):
        if mask >> b & 1:
            less = {a: g for a, g in settings.items() if a != k}
            f = _changed(ref, _oracle_chunks(O, mc, x16, fs, less, chunks))
            assert f >= STAGE_MIN, "%s: without %s only %.4f of the samples change" % (what, k, f)
    if settings.get("multiband"):
        f = _changed(ref, _oracle_chunks(O, mc, x16, fs, dict(settings, multiband=False), chunks))
        assert f >= MB_MIN, "%s: the compressor changes only %.4f of the samples" % (what, f)
    ref = np.concatenate(ref)
    ref.setflags(write=False)
    return x16, chunks, settings, ref


def test_matrix_reaches_every_mask_and_dimension():
    """each row of the table launches every state dimension, and every mask where the
    row's dispatch goes by mask (k_front2's, in all but E)"""
    dims = {0, 2, 4, 8, 10, 12, 16, 18, 20}
    for v, V in VARIANTS.items():
        masks = [m for m, _, _ in V["cases"]]
        if v == "A192":
            assert sorted(masks) == [6, 7, 14] and {_dim(m) for m in masks} == {16, 18}
            continue
        assert {_dim(m) for m in masks} == dims, v
        if v != "E":
            assert sorted(set(masks)) == list(range(16)), v
        assert all((sb != 0) == bool(m & 1) and (st != 0) == bool(m & 8) for m, sb, st in V["cases"])
    for v in ("A", "B"):
        assert set(VARIANTS[v]["cases"]) == set(CASES36)
    # C and D do not repeat the signs A takes first (every shelf positive)
    first = {m: (sb, st) for m, sb, st in reversed(CASES36)}
    for v in ("C", "D"):
        assert all((sb, st) != first[m] for m, sb, st in VARIANTS[v]["cases"] if m & 9)


@pytest.mark.parametrize("v", sorted(VARIANTS))
def test_preconditions_on_the_oracle(oracle_mod, v):
    """the oracle half of every case of a row (no GPU): its preconditions hold"""
    for p in _params(v):
        _reference(*p.values)


def _run_f32(x16, fs, settings, chunks, seg_frames):
    import torch
    from amx.engine import MasteringJob
    # float32 input x16 / 32768: ffmpeg's quantisation gives x16 back exactly
    xf = np.ascontiguousarray(x16.astype(np.float32) / np.float32(32768.0))
    job = MasteringJob(fs, 2, settings, [x16.shape[0]], chunks=[(0, s, m) for s, m in chunks],
                       seg_frames=seg_frames)
    job.run_chunks(torch.from_numpy(xf).cuda())
    torch.cuda.synchronize()
    return job.out[:job.info.out_frames].cpu().numpy()


def _check(gpu, monkeypatch, v, i, mask, sb, st, fs):
    x16, chunks, settings, ref = _reference(v, i, mask, sb, st, fs)
    V = VARIANTS[v]
    for k, e in V.get("env", {}).items():
        monkeypatch.setenv(k, e)
    if V["inp"] == "mc":
        out = _mc_chain(x16, fs, settings, chunks, seg_frames=V["seg"])
    elif V["inp"] == "f32":
        out = _run_f32(x16, fs, settings, chunks, V["seg"])
    else:
        out, _ = _chunk_chain(x16, fs, settings, chunks, seg_frames=V["seg"])
    what = "eq mask %d (D %d) bass %+d treble %+d, %s fs=%d" % (mask, _dim(mask), sb, st, v, fs)
    if out.shape == ref.shape:
        d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
        print("EQMASK %s max|diff| %d differing %d of %d" % (what, d.max(), int((d != 0).sum()), d.size))
    _cmp(out, ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("v,i,mask,sb,st,fs", _params("A") + _params("A192"))
def test_eq_masks_int16_width_multiband(gpu, oracle_mod, monkeypatch, v, i, mask, sb, st, fs):
    """A: k_front1<D,1,false>, k_scan_blk<D>, k_front2<M, multiband> on all 36 cases, and D 16 /
    18 at 192 kHz"""
    _check(gpu, monkeypatch, v, i, mask, sb, st, fs)


@pytest.mark.gpu
@pytest.mark.parametrize("v,i,mask,sb,st,fs", _params("B"))
def test_eq_masks_float32_analog(gpu, oracle_mod, monkeypatch, v, i, mask, sb, st, fs):
    """B: k_analog_h + k_gemv16<D>, k_front2<M, plain> on all 36 cases"""
    _check(gpu, monkeypatch, v, i, mask, sb, st, fs)


@pytest.mark.gpu
@pytest.mark.parametrize("v,i,mask,sb,st,fs", _params("C"))
def test_eq_masks_mono_analog_multiband(gpu, oracle_mod, monkeypatch, v, i, mask, sb, st, fs):
    """C: k_front1<D,1,true> at seg_frames 256 on the 16 masks"""
    _check(gpu, monkeypatch, v, i, mask, sb, st, fs)


@pytest.mark.gpu
@pytest.mark.parametrize("v,i,mask,sb,st,fs", _params("D"))
def test_eq_masks_float32_plain(gpu, oracle_mod, monkeypatch, v, i, mask, sb, st, fs):
    """D: k_front1s<D,false> on the 16 masks"""
    _check(gpu, monkeypatch, v, i, mask, sb, st, fs)


@pytest.mark.gpu
@pytest.mark.parametrize("v,i,mask,sb,st,fs", _params("E"))
def test_eq_masks_float32_full_table(gpu, oracle_mod, monkeypatch, v, i, mask, sb, st, fs):
    """E: k_front1s<D,true> (AMX_F1 = 2) on one mask per state dimension"""
    _check(gpu, monkeypatch, v, i, mask, sb, st, fs)


@pytest.mark.gpu
@pytest.mark.parametrize("v,i,mask,sb,st,fs", _params("MC") + _params("MCmb"))
def test_eq_masks_three_channels(gpu, oracle_mod, monkeypatch, v, i, mask, sb, st, fs):
    """the stream chain (MultiChannelJob.run_chunks) at C = 3 on the 16 masks, without and
    with the multiband compressor, against oracle.chunk_mc"""
    _check(gpu, monkeypatch, v, i, mask, sb, st, fs)
