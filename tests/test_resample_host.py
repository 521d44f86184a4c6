"""CPU: the host side of the output resampler (include/amx.h amx_resample_size, the
settings key output_rate) -- the geometry against the oracle's restatement of
libswresample (oracle/amx_oracle.c orc_swr_*), the pairs it refuses, the key's values and
that master_audio rejects a bad key before it opens the input.  The kernel is pinned on
the GPU (tests/test_gpu_resample.py).
"""
import ctypes

import pytest

PAIRS = [(192000, 48000), (192000, 44100), (192000, 96000), (96000, 44100), (48000, 44100), (44100, 48000),
         (48000, 96000), (192000, 32000)]


def _size(in_rate, out_rate, frames):
    from amx import capi
    n, t, al, ph = ctypes.c_int64(-1), ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = capi.load().amx_resample_size(in_rate, out_rate, frames, ctypes.byref(n), ctypes.byref(t),
                                       ctypes.byref(al), ctypes.byref(ph))
    return rc, n.value, t.value, al.value, ph.value


@pytest.mark.parametrize("in_rate,out_rate", PAIRS)
def test_geometry_matches_oracle(oracle_mod, in_rate, out_rate):
    L, M = oracle_mod.swr_geometry(in_rate, out_rate)
    taps, alloc, _ = oracle_mod.swr_filter(in_rate, out_rate)
    phases = oracle_mod.swr_phases(in_rate, out_rate)
    assert phases == L <= 1024
    for frames in (0, 1, 7, 4097):
        want = int(oracle_mod.lib().orc_swr_out_frames(ctypes.c_int64(frames), ctypes.c_int(in_rate),
                                                       ctypes.c_int(out_rate)))
        assert want == -(-frames * L // M)
        assert _size(in_rate, out_rate, frames) == (0, want, taps, alloc, phases)


def test_geometry_known_values():
    """the filters the issue lists: 132 taps and one phase for 192 -> 48 kHz, 144 taps and 147
    phases for 192 -> 44.1 kHz, 36 taps in rows of 40 for 48 -> 44.1 kHz, 32 taps and 160
    phases for 44.1 -> 48 kHz"""
    assert _size(192000, 48000, 8)[1:] == (2, 132, 136, 1)
    assert _size(192000, 44100, 640)[1:] == (147, 144, 144, 147)
    assert _size(48000, 44100, 160)[1:] == (147, 36, 40, 147)
    assert _size(44100, 48000, 147)[1:] == (160, 32, 32, 160)


def test_null_outputs_are_optional():
    from amx import capi
    assert capi.load().amx_resample_size(192000, 48000, 5, None, None, None, None) == capi.AMX_OK


def test_refusals(oracle_mod):
    from amx import capi, resample
    # more than 256 taps; more than 1024 phases with a filter longer than 32 taps: the
    # oracle has no filter for either
    for pair in ((192000, 22050), (44100, 44056)):
        with pytest.raises(ValueError):
            oracle_mod.swr_phases(*pair)
        assert _size(*pair, 100)[0] == capi.AMX_ERANGE
        with pytest.raises(ValueError) as e:
            resample.check_pair(*pair)
        assert str(pair[0]) in str(e.value) and str(pair[1]) in str(e.value)
    # more than 1024 phases with the 32-tap filter: the interpolating path, not wanted here
    assert oracle_mod.swr_phases(22050, 192000) == 1024
    assert _size(22050, 192000, 100)[0] == capi.AMX_ERANGE
    assert _size(0, 48000, 100)[0] == capi.AMX_EINVAL
    assert _size(48000, -1, 100)[0] == capi.AMX_EINVAL
    assert _size(48000, 44100, -1)[0] == capi.AMX_EINVAL
    assert _size(48000, 48000, 100)[0] == capi.AMX_EINVAL
    assert b"48000" in capi.load().amx_last_error()
    resample.check_pair(48000, 48000)          # equal rates: no resampler runs


def test_the_measurement_resampler_keeps_its_limit():
    """the loudness plan's own resampler rows stay at 144 taps: a pair the output resampler
    takes (192 -> 32 kHz, rows of 200) is still one the measurement's filter refuses"""
    import os
    import re
    from amx import build
    text = open(os.path.join(build.CSRC, "amx_tables.hpp")).read()
    assert re.search(r"#define AMX_SWR_MAX_ALLOC 144\b", text) and re.search(r"#define AMX_RS_MAX_ALLOC 256\b", text)
    assert _size(192000, 32000, 0)[3] == 200


def test_tile_constant_matches_the_kernel():
    import os
    import re
    from amx import build, resample
    text = open(os.path.join(build.CSRC, "amx_tables.hpp")).read()
    assert int(re.search(r"#define AMX_RS_TILE (\d+)", text).group(1)) == resample.TILE


def test_output_rate_values():
    from amx.settings import output_rate
    assert output_rate({}, 48000) is None
    assert output_rate(None, 48000) is None
    assert output_rate({"output_rate": None}, 48000) is None
    assert output_rate({"output_rate": 44100}, 48000) == 44100
    assert output_rate({"output_rate": "input"}, 48000) == 48000
    for bad in (0, -1, "cd", 44100.5, True):
        with pytest.raises(ValueError):
            output_rate({"output_rate": bad}, 48000)


@pytest.mark.parametrize("bad", [0, "cd", True, 44100.5])
def test_master_audio_checks_the_key_before_the_input(tmp_path, bad):
    """a path that does not exist: the ValueError of the key, not the file error"""
    import audio_mastering_engine as ame
    settings = dict(input_file=str(tmp_path / "missing.wav"), output_file=str(tmp_path / "out.wav"),
                    output_rate=bad)
    with pytest.raises(ValueError, match="output_rate"):
        ame.master_audio(settings)
    assert not (tmp_path / "out.wav").exists()


def test_master_audio_refuses_an_unsupported_pair_before_any_kernel(tmp_path):
    """a 192 kHz input asked for at 22.05 kHz: the ValueError names both rates, and it
    comes before anything goes to the device (this test runs without one)"""
    import numpy as np
    import audio_mastering_engine as ame
    from amx import wavio
    src = str(tmp_path / "in.wav")
    wavio.write_wav_s16(src, np.zeros((64, 2), np.int16), 192000)
    with pytest.raises(ValueError, match="192000.*22050"):
        ame.master_audio(dict(input_file=src, output_file=str(tmp_path / "out.wav"), output_rate=22050))
    # with lufs set a 48 kHz input can end at 192 kHz (loudnorm's dynamic mode): refused too
    wavio.write_wav_s16(src, np.zeros((64, 2), np.int16), 48000)
    with pytest.raises(ValueError, match="192000.*22050"):
        ame.master_audio(dict(input_file=src, output_file=str(tmp_path / "out.wav"), output_rate=22050, lufs=-14.0))
    assert not (tmp_path / "out.wav").exists()
