"""CPU: the settings key multichannel_dynamic (loudnorm's dynamic mode on 3..8-channel
tracks) -- its schema, and the delivery-rate check it widens."""
import pytest


def test_key_schema():
    from amx.settings import multichannel_dynamic
    assert multichannel_dynamic(None) is False
    assert multichannel_dynamic({}) is False
    assert multichannel_dynamic({"lufs": -14.0}) is False
    assert multichannel_dynamic({"multichannel_dynamic": False}) is False
    assert multichannel_dynamic({"multichannel_dynamic": True}) is True
    for bad in (1, 0, "yes", "True", None, 1.0):
        with pytest.raises(ValueError, match="multichannel_dynamic"):
            multichannel_dynamic({"multichannel_dynamic": bad})


def test_bad_key_refused_before_any_file_is_read(tmp_path):
    """as for flac_decode: the input file does not even exist"""
    import audio_mastering_engine as ame
    s = dict(input_file=str(tmp_path / "missing.wav"), output_file=str(tmp_path / "out.wav"))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="multichannel_dynamic"):
            ame.master_audio(dict(s, multichannel_dynamic=bad))


def test_delivery_rate_checks_192k_for_multichannel_only_with_the_key():
    """22050 Hz cannot be reached from 192 kHz (amx_resample_size refuses the pair) but can
    from 44.1 kHz: a C > 2 call meets the 192 kHz master only with the key"""
    from amx.engine import delivery_rate
    s = {"lufs": -14.0, "output_rate": 22050}
    with pytest.raises(ValueError, match="192000.*22050"):
        delivery_rate(s, 44100, 2)
    for C in (3, 6, 8):
        assert delivery_rate(s, 44100, C) == 22050
        assert delivery_rate(dict(s, multichannel_dynamic=False), 44100, C) == 22050
        with pytest.raises(ValueError, match="192000.*22050"):
            delivery_rate(dict(s, multichannel_dynamic=True), 44100, C)
        # without lufs no dynamic mode: the key changes nothing
        assert delivery_rate(dict(s, lufs=None, multichannel_dynamic=True), 44100, C) == 22050
    with pytest.raises(ValueError, match="multichannel_dynamic"):
        delivery_rate(dict(s, multichannel_dynamic="yes"), 44100, 6)
    assert delivery_rate({"lufs": -14.0, "multichannel_dynamic": True}, 44100, 6) is None


def test_exports_declared():
    """the two new entry points are in the header and in capi's table"""
    import os
    from amx import capi
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "amx.h")).read()
    for sym in ("amx_mc_loudnorm_192k_size", "amx_mc_loudnorm_192k"):
        assert sym in capi.EXPORTS and ("AMX_API int %s(" % sym) in hdr
