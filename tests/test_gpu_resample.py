"""GPU: the output resampler (csrc/amx_resample.hip, amx/resample.py, the settings key
output_rate) against the oracle's restatement of libswresample's float resampler
(oracle/amx_oracle.c orc_upsample) and ffmpeg's f32 -> s16 conversion, sample for sample
(parity with an ffmpeg binary is unpinned, like every ffmpeg stage: DESIGN.md 3.12).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [(192000, 48000), (192000, 44100), (96000, 44100), (48000, 44100), (44100, 48000), (48000, 96000)]
CHANNELS = [1, 2, 3, 6, 8]
LENGTHS = [1, 2, 7, 131, 4097, 20011]

_refs = {}


def _want(oracle_mod, x16, fi, fo):
    """the oracle's float stream through ffmpeg's f32 -> s16 conversion"""
    u = oracle_mod.upsample(x16, fi, fo).astype(np.float32) * np.float32(32768)
    return np.clip(np.rint(u), -32768, 32767).astype(np.int16)


def _tile_lengths(oracle_mod, fi, fo):
    """input lengths whose output is T - 1, T, T + 1 and 3 T + 1 frames for the kernel's tile
    T -- or, where an upsampling ratio skips that count, the next count it reaches"""
    from amx.resample import TILE
    L, M = oracle_mod.swr_geometry(fi, fo)
    return sorted({(target - 1) * M // L + 1 for target in (TILE - 1, TILE, TILE + 1, 3 * TILE + 1)})


def _gpu(x16, fi, fo):
    import torch
    from amx.resample import resample_s16
    return resample_s16(torch.from_numpy(x16).cuda(), fi, fo).cpu().numpy()


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("fi,fo", PAIRS)
def test_exact_against_oracle(gpu, oracle_mod, fi, fo, C):
    """random full-range int16 of every length: inputs shorter than the filter (1, 2, 7
    frames: the mirror applied more than once), the period wrap of the phase, tile seams,
    odd channel counts"""
    from amx.resample import TILE
    L, M = oracle_mod.swr_geometry(fi, fo)
    tiles = _tile_lengths(oracle_mod, fi, fo)
    outs = [-(-n * L // M) for n in tiles]
    assert TILE in outs and (TILE + 1 in outs or TILE + 2 in outs) and 3 * TILE < outs[-1] <= 3 * TILE + 2, outs
    if L <= M:
        assert outs == [TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
    rng = np.random.default_rng(fi // 100 + fo + C)
    for n in LENGTHS + tiles:
        x = rng.integers(-32768, 32768, (n, C)).astype(np.int16)
        want = _want(oracle_mod, x, fi, fo)
        got = _gpu(x, fi, fo)
        assert got.shape == want.shape == (-(-n * L // M), C), (n, got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (n, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("fi,fo", [(192000, 48000), (44100, 48000)])
def test_clipping(gpu, oracle_mod, fi, fo):
    """a full-scale square wave overshoots past full scale in the filter: the quantiser's
    clip at both rails is reached, in the oracle first"""
    n = 4000
    x = np.where((np.arange(n) // 400) % 2 == 0, 32767, -32768).astype(np.int16)
    x = np.stack([x, -x - 1], axis=1).astype(np.int16)
    want = _want(oracle_mod, x, fi, fo)
    u = oracle_mod.upsample(x, fi, fo)
    assert u.max() > 1.0 and u.min() < -1.0, (u.max(), u.min())
    assert (want == 32767).any() and (want == -32768).any()
    np.testing.assert_array_equal(_gpu(x, fi, fo), want)


@pytest.mark.parametrize("fi,fo,C,n", [(192000, 44100, 2, 5000), (48000, 96000, 3, 700), (192000, 48000, 1, 3)])
def test_bounds_and_determinism(gpu, oracle_mod, fi, fo, C, n):
    """64 guard samples on each side of the output stay as they were; a second run over
    other bytes gives the same output; a capacity one frame short is refused unwritten"""
    import torch
    from amx import capi
    from amx.resample import Resampler
    rng = np.random.default_rng(n)
    x = rng.integers(-32768, 32768, (n, C)).astype(np.int16)
    want = _want(oracle_mod, x, fi, fo)
    n_out = want.shape[0]
    rs = Resampler(fi, fo, C)
    assert rs.out_frames(n) == n_out
    y = torch.from_numpy(x).cuda()
    runs = []
    for fill in (-23131, 0x1234):
        buf = torch.full((64 + n_out * C + 64,), fill, dtype=torch.int16, device="cuda")
        assert rs.run(y, buf[64:64 + n_out * C], n_out) == capi.AMX_OK
        got = buf.cpu().numpy()
        assert (got[:64] == fill).all() and (got[-64:] == fill).all()
        runs.append(got[64:-64].reshape(n_out, C))
    np.testing.assert_array_equal(runs[0], runs[1])
    np.testing.assert_array_equal(runs[0], want)
    buf = torch.full((64 + n_out * C + 64,), 77, dtype=torch.int16, device="cuda")
    assert rs.run(y, buf[64:64 + n_out * C], n_out - 1) == capi.AMX_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 77).all()
    # no frames: nothing launched, nothing written; NULL handles and pointers are refused
    assert rs.run(y[:0], buf[64:], 0) == capi.AMX_OK
    lib = capi.load()
    assert lib.amx_resampler_run(None, capi.ptr(y), n, capi.ptr(buf), n_out, None) == capi.AMX_EINVAL
    assert lib.amx_resampler_run(rs.h, None, n, capi.ptr(buf), n_out, None) == capi.AMX_EINVAL
    assert lib.amx_resampler_run(rs.h, capi.ptr(y), n, None, n_out, None) == capi.AMX_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 77).all()
    rs.close()
    lib.amx_resampler_free(None)


def _dynamic_signal(seconds, fs, seed):
    """tests/test_gpu_dynamic.py's: a quiet programme with sparse full-scale transients, so
    that TP + offset > -1.5 dBTP and loudnorm leaves its linear mode"""
    from amx import synth
    n = int(fs * seconds)
    x = synth.mix_like(n, fs, 2, seed=seed) * 0.12
    rng = np.random.default_rng(seed)
    for k in rng.integers(0, n - 200, max(2, int(seconds * 2))):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, 2))
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def _master(x, fs, settings):
    from amx import engine
    y, rep = engine.master_array(x, fs, settings)
    y = y.cpu().numpy()
    rep["job"].close()
    return y, rep


def _linear_ref():
    """one keyless master_array run of the linear case, shared by the tests that need it"""
    if "linear" not in _refs:
        from amx import synth
        fs = 48000
        x = synth.mix_like(int(fs * LINEAR_SECONDS), fs, 2, seed=5).astype(np.float32)
        settings = dict(bass_boost=1.0, lufs=-14.0)
        y, rep = _master(x, fs, settings)
        print("keyless master: mode %s at %d Hz, %d frames" % (rep["modes"], rep["sample_rate"], y.shape[0]))
        y.setflags(write=False)
        _refs["linear"] = (x, fs, settings, y, rep)
    return _refs["linear"]


# 1.5 s of synth.mix_like with lufs = -14 never takes loudnorm's linear mode: below 3 s no
# short-term block exists, LRA measures 0.00 and pass 2 runs dynamic (its < 3 s fallback, at
# 192 kHz) -- tests/test_gpu_flac_encode.py notes the same of a 3 s track.  Measured here: 1.5
# and 3.5 s are dynamic, 4 s is the shortest linear one.  So the linear case runs on 4 s and
# the 1.5 s signal keeps a test of its own (test_master_array_short).
LINEAR_SECONDS = 4.0


def test_master_array_linear(gpu, oracle_mod):
    """a master at the input's rate: output_rate 44100 is the oracle's resampling of the
    keyless call's output; 48000 and "input" change nothing"""
    x, fs, settings, y0, rep0 = _linear_ref()
    assert "resampled_from" not in rep0
    assert rep0["modes"] == ["linear"] and rep0["sample_rate"] == fs, (rep0["modes"], rep0["sample_rate"])
    y, rep = _master(x, fs, dict(settings, output_rate=44100))
    assert rep["sample_rate"] == 44100 and rep["resampled_from"] == fs
    np.testing.assert_array_equal(y, _want(oracle_mod, y0, fs, 44100))
    for same in (48000, "input"):
        y, rep = _master(x, fs, dict(settings, output_rate=same))
        assert rep["sample_rate"] == fs and "resampled_from" not in rep
        assert y.tobytes() == y0.tobytes()


def test_master_array_short(gpu, oracle_mod):
    """1.5 s of synth.mix_like at 48 kHz with lufs = -14: too short for the linear mode, the
    master is at 192 kHz.  44100, 48000 and "input" are each the oracle's resampling of the
    keyless output from that rate; 192000 changes nothing"""
    from amx import synth
    fs = 48000
    x = synth.mix_like(int(fs * 1.5), fs, 2, seed=5).astype(np.float32)
    settings = dict(bass_boost=1.0, lufs=-14.0)
    y0, rep0 = _master(x, fs, settings)
    assert rep0["sample_rate"] == 192000 and "resampled_from" not in rep0
    for key, rate in ((44100, 44100), (48000, 48000), ("input", 48000)):
        y, rep = _master(x, fs, dict(settings, output_rate=key))
        assert rep["sample_rate"] == rate and rep["resampled_from"] == 192000
        np.testing.assert_array_equal(y, _want(oracle_mod, y0, 192000, rate))
    y, rep = _master(x, fs, dict(settings, output_rate=192000))
    assert rep["sample_rate"] == 192000 and "resampled_from" not in rep and y.tobytes() == y0.tobytes()


def test_master_array_dynamic(gpu, oracle_mod):
    """loudnorm's dynamic mode leaves the master at 192 kHz: output_rate "input" brings it
    back to the input's 48 kHz, the oracle's resampling of the keyless call's own output
    (so dynamic mode's own tolerance stays out of the comparison)"""
    fs = 48000
    x = _dynamic_signal(6.0, fs, 32)
    settings = dict(bass_boost=1.0, lufs=-14.0)
    y0, rep0 = _master(x, fs, settings)
    assert rep0["modes"] == ["dynamic"] and rep0["sample_rate"] == 192000 and "resampled_from" not in rep0
    y, rep = _master(x, fs, dict(settings, output_rate="input"))
    assert rep["modes"] == ["dynamic"] and rep["sample_rate"] == 48000 and rep["resampled_from"] == 192000
    np.testing.assert_array_equal(y, _want(oracle_mod, y0, 192000, 48000))
    assert y.shape[0] == -(-y0.shape[0] // 4)


def test_master_array_refuses_before_running(gpu):
    from amx import engine
    x = np.zeros((4800, 2), np.float32)
    with pytest.raises(ValueError, match="output_rate"):
        engine.master_array(x, 48000, {"output_rate": True})
    with pytest.raises(ValueError, match="192000.*22050"):
        engine.master_array(x, 48000, {"output_rate": 22050, "lufs": -14.0})


@pytest.mark.parametrize("C", [2, 3])
def test_master_audio_files(gpu, oracle_mod, tmp_path, C):
    """master_audio with output_rate 44100 to x.wav and x.flac (C = 3: through
    _master_multichannel): the header's rate, the frame count, and the samples of
    master_array with the same key"""
    import audio_mastering_engine as ame
    from amx import flacio, synth, wavio
    fs = 48000
    x = synth.mix_like(fs // 2 + 77, fs, C, seed=90 + C)
    x16 = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
    settings = dict(bass_boost=1.5, treble_boost=-1.0, lufs=None, output_rate=44100)
    src = str(tmp_path / "in.wav")
    wavio.write_wav_pcm(src, x16, fs, "s16")
    want, rep = _master(x16, fs, settings)
    assert rep["sample_rate"] == 44100 and rep["resampled_from"] == fs
    keyless, _ = _master(x16, fs, dict(settings, output_rate=None))
    n_out = -(-keyless.shape[0] * 147 // 160)
    assert want.shape == (n_out, max(C, 2))
    np.testing.assert_array_equal(want, _want(oracle_mod, keyless, fs, 44100))
    wav, flac = str(tmp_path / "x.wav"), str(tmp_path / "x.flac")
    for dst in (wav, flac):
        assert ame.master_audio(dict(settings, input_file=src, output_file=dst)) == dst
    y, info = wavio.read_wav_native(wav)
    assert info.sample_rate == 44100 and info.channels == want.shape[1]
    np.testing.assert_array_equal(y.reshape(want.shape), want)
    data = open(flac, "rb").read()
    got, finfo = flacio.decode_flac(data)
    assert finfo.sample_rate == 44100 and finfo.channels == want.shape[1] and finfo.total_frames == n_out
    np.testing.assert_array_equal(got.reshape(want.shape), want.astype(np.int32) << 16)
