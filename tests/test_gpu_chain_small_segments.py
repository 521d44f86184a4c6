"""GPU: the segment kernels of the chunk chain on a full, a partial and a one-frame segment,
bit for bit against the C oracle.

k_front2, k_xover2 and k_gemv16 (amx_chain.hip) hold one lane per (128-frame segment,
channel); their frame loops carry the forms checked on the host by
tests/test_chain_identities.py (the two peak stages as two bodies, the lane-signed width,
the int16 sample fed to the GEMVs as an int against rows scaled by 2^-15).  Here the whole
chain runs them on stereo 48 kHz float32 input with the analog stage (k_analog_h, k_gemv16,
k_front2, and k_xover2 where the compressor is on) over two chunks of 3 * 128 + 37 and
128 + 1 frames: three full segments and a 37-frame one, then a full segment and a one-frame
one.  Settings: EQ masks 15, 6, 1 with a negative bass shelf (the float32 first product),
8 with a negative treble shelf, and 0, each with width off / 1.3 and the multiband
compressor off / on; and one case with loudness normalisation and no compressor, where
k_front2 also accumulates the K-weighting rows and the sample peak (its KW form).

The comparison is exact (every sample equal).  These inputs are far too short for a
start-state rounding flip to be likely; the oracle's own determinism on them is asserted
first, without a GPU (``test_oracle_is_deterministic_on_these_inputs``).
"""
import functools
import itertools

import numpy as np
import pytest

from test_gpu_parity import MB

FS = 48000
CHUNKS = ((0, 3 * 128 + 37), (3 * 128 + 37, 128 + 1))
N = CHUNKS[-1][0] + CHUNKS[-1][1]
EQ = {
    "m15": dict(bass_boost=3.0, mid_cut=4.0, presence_boost=2.5, treble_boost=2.0),
    "m06": dict(mid_cut=4.0, presence_boost=2.5),
    "m01neg": dict(bass_boost=-3.0),
    "m08neg": dict(treble_boost=-2.0),
    "m00": dict(),
}
CASES = [pytest.param(e, w, mb, False, id="%s-w%s-mb%d" % (e, "1.3" if w else "off", mb))
         for e, w, mb in itertools.product(EQ, (False, True), (False, True))]
CASES.append(pytest.param("m15", True, False, True, id="m15-w1.3-loudnorm"))


def _settings(eq, width, mb, lufs):
    s = dict(EQ[eq], analog_character=40.0)
    if width:
        s["width"] = 1.3
    if mb:
        s.update(MB)
    if lufs:
        s["lufs"] = -14.0
    return s


@functools.lru_cache(maxsize=None)
def _input():
    from amx import synth
    import oracle as O
    x16 = O.quantize(synth.music_like(N, FS, 2, seed=4242, peak_dbfs=-1.0))
    x16.setflags(write=False)
    return x16


@functools.lru_cache(maxsize=None)
def _reference(eq, width, mb, lufs):
    import oracle as O
    x16 = _input()
    s = _settings(eq, width, mb, lufs)
    ref = np.concatenate([O.chunk(x16[a:a + m], FS, s) for a, m in CHUNKS])
    ref.setflags(write=False)
    return ref


def test_oracle_is_deterministic_on_these_inputs(oracle_mod):
    x16 = _input()
    assert x16.shape == (N, 2) and np.abs(x16.astype(np.int32)).max() > 20000
    for p in CASES:
        eq, width, mb, lufs = p.values
        s = _settings(eq, width, mb, lufs)
        again = np.concatenate([oracle_mod.chunk(x16[a:a + m], FS, s) for a, m in CHUNKS])
        np.testing.assert_array_equal(again, _reference(eq, width, mb, lufs))
    # and the cases differ from one another where a stage is switched (the matrix can tell
    # a skipped stage from a right one)
    base = _reference("m15", True, True, False)
    assert (base[:400] != _reference("m15", False, True, False)[:400]).mean() > 0.1
    assert (base[:400] != _reference("m06", True, True, False)[:400]).mean() > 0.1
    assert (_reference("m15", True, False, False)[:400] != base[:400]).mean() > 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("eq,width,mb,lufs", CASES)
def test_small_segments_bit_exact(gpu, oracle_mod, eq, width, mb, lufs):
    import torch
    from amx.engine import MasteringJob
    x16 = _input()
    ref = _reference(eq, width, mb, lufs)
    # float32 input x16 / 32768: the chain's quantisation gives x16 back exactly
    xf = np.ascontiguousarray(x16.astype(np.float32) / np.float32(32768.0))
    job = MasteringJob(FS, 2, _settings(eq, width, mb, lufs), [N], chunks=[(0, a, m) for a, m in CHUNKS],
                       seg_frames=128)
    job.run_chunks(torch.from_numpy(xf).cuda())
    torch.cuda.synchronize()
    out = job.out[:job.info.out_frames].cpu().numpy()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    print("SMALLSEG %s width %s mb %s lufs %s: max|diff| %d differing %d of %d"
          % (eq, width, mb, lufs, d.max(), int((d != 0).sum()), d.size))
    np.testing.assert_array_equal(out, ref)
