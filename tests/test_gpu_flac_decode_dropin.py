"""master_audio with the settings key flac_decode: "device" decodes a *.flac input on the
device (amx.flacio.decode_flac_device) and must write, byte for byte, the file the default
path (the host decoder and an upload) writes; a value that is neither "host" nor "device"
is refused before any file is read."""
import os

import numpy as np
import pytest


def _master_both(tmp_path, channels, settings):
    import audio_mastering_engine as ame
    from amx import flacio, synth
    fs = 48000
    x = synth.mix_like(fs * 2, fs, channels if channels <= 2 else 2, seed=40 + channels)
    if channels > 2:
        x = np.concatenate([x * g for g in (1.0, 0.7, 0.5)], axis=1)[:, :channels]
    x16 = np.clip(np.round(x * 30000.0), -32768, 32767).astype(np.int16)
    src = os.path.join(str(tmp_path), "in%d.flac" % channels)
    flacio.write_flac(src, x16, fs, block=1152, lpc_order=8 if channels == 2 else 0)   # (the device encoder: quick)
    out = {}
    for ext in ("wav", "flac"):
        for mode in (None, "host", "device"):
            dst = os.path.join(str(tmp_path), "m%d_%s.%s" % (channels, mode, ext))
            extra = {} if mode is None else dict(flac_decode=mode)
            assert ame.master_audio(dict(settings, input_file=src, output_file=dst, **extra)) == dst
            with open(dst, "rb") as f:
                out[ext, mode] = f.read()
        assert len(out[ext, None]) > 1000
        assert out[ext, "device"] == out[ext, None] == out[ext, "host"]
    assert out["wav", None] != out["flac", None]


@pytest.mark.gpu
def test_stereo_flac_input_decoded_on_the_device(gpu, tmp_path):
    _master_both(tmp_path, 2, dict(bass_boost=1.0, presence_boost=1.5, width=1.2, lufs=-14.0))


@pytest.mark.gpu
def test_six_channel_flac_input_decoded_on_the_device(gpu, tmp_path):
    _master_both(tmp_path, 6, dict(bass_boost=1.0, treble_boost=0.5))


def test_bad_flac_decode_value_is_refused_before_any_file_is_read(tmp_path):
    import audio_mastering_engine as ame
    from amx import settings
    missing = os.path.join(str(tmp_path), "not_there.flac")
    with pytest.raises(ValueError, match="flac_decode"):
        ame.master_audio(dict(input_file=missing, output_file=os.path.join(str(tmp_path), "o.wav"),
                              flac_decode="gpu?"))
    with pytest.raises(ValueError, match="flac_decode"):
        ame._device_input(missing, dict(flac_decode="gpu?"))
    assert settings.flac_decode_mode({}) == settings.flac_decode_mode(None) == "host"
    assert settings.flac_decode_mode(dict(flac_decode="device")) == "device"
    for bad in ("Device", "", None, 1, True):
        with pytest.raises(ValueError):
            settings.flac_decode_mode(dict(flac_decode=bad))
