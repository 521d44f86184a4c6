"""CPU: amx.flacio.flac_container, the 42 bytes the host puts in front of the device
encoder's frame stream ('fLaC' + one STREAMINFO block marked last).

The frames come from the test-side encoder (tests/flac_enc.py): its stream's own metadata
blocks are skipped by their 4-byte headers, the frame lengths follow from the decoder's
packet list, and the rebuilt file must decode to the same samples with STREAMINFO's fields
reading back through amx_flac_info.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import flac_enc


def _frames_of(stream):
    """(the frame bytes of a FLAC stream, offset of the first frame)"""
    assert stream[:4] == b"fLaC"
    pos = 4
    while True:
        last, length = stream[pos] >> 7, int.from_bytes(stream[pos + 1:pos + 4], "big")
        pos += 4 + length
        if last:
            break
    return stream[pos:], pos


def _frame_lengths(payload, blocks):
    """every frame's length in bytes, from the decoder's packet list (one entry per frame)
    and the stream length: frame k starts at the next sync whose header codes frame number
    k with a good CRC-8 (a fixed-blocksize stream), the last frame ends with the stream"""
    starts = []
    want = 0
    pos = 0
    while want < len(blocks):
        pos = payload.index(b"\xff\xf8", pos)
        # fixed-blocksize stream: byte 4.. holds the frame number UTF-8 style
        num = _utf8_value(payload, pos + 4)
        hdr_ok = num == want and _header_crc_ok(payload, pos)
        if hdr_ok:
            starts.append(pos)
            want += 1
            pos += 6
        else:
            pos += 1
    starts.append(len(payload))
    return np.diff(np.asarray(starts, np.int64))


def _utf8_value(b, i):
    b0 = b[i]
    if b0 < 0x80:
        return b0
    nb = 8 - int(b0 ^ 0xFF).bit_length()
    if nb < 2 or nb > 7 or i + nb > len(b):
        return -1
    v = b0 & ((1 << (7 - nb)) - 1) if nb < 7 else 0
    for k in range(1, nb):
        if (b[i + k] & 0xC0) != 0x80:
            return -1
        v = (v << 6) | (b[i + k] & 0x3F)
    return v


def _header_crc_ok(b, pos):
    bs, sr = b[pos + 2] >> 4, b[pos + 2] & 15
    i = pos + 4
    b0 = b[i]
    i += 1 if b0 < 0x80 else 8 - int(b0 ^ 0xFF).bit_length()
    i += {6: 1, 7: 2}.get(bs, 0) + {12: 1, 13: 2, 14: 2}.get(sr, 0)
    return i < len(b) and flac_enc.crc8(b[pos:i]) == b[i]


@pytest.mark.parametrize("channels,fs,frames,block", [(2, 44100, 3 * 1024 + 100, 1024), (1, 48000, 700, 4096),
                                                      (6, 192000, 2 * 576, 576), (2, 768000, 5000, 1000)])
def test_container_round_trip(channels, fs, frames, block):
    from amx import capi, flacio
    rng = np.random.default_rng(channels * 1000 + block)
    x = rng.integers(-3000, 3000, (frames, channels)).astype(np.int64)
    src = flac_enc.encode(x, fs, 16, seed=block, block=block, kinds=["verbatim", "fixed1", "fixed2", "constant"])
    ref, info, blocks = flacio.decode_flac(src, with_blocks=True)
    payload, first = _frames_of(src)
    assert first > 42                                   # the source carries extra metadata blocks
    fb = _frame_lengths(payload, blocks)
    assert fb.sum() == len(payload) and len(fb) == len(blocks) == -(-frames // block)
    md5 = hashlib.md5(x.astype("<i2").tobytes()).digest()
    out = flacio.flac_container(payload, fb, fs, channels, frames, block, md5)
    assert len(out) == 42 + fb.sum() and out[:4] == b"fLaC" and out[4] == 0x80
    assert out[42:] == payload and out[26:42] == md5
    got, ginfo = flacio.decode_flac(out)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, (x << 16).astype(np.int32))
    L = capi.load()
    fi = capi.FlacInfo()
    raw = np.frombuffer(out, np.uint8)
    assert L.amx_flac_info(ctypes.c_void_p(raw.ctypes.data), raw.size, ctypes.byref(fi)) == capi.AMX_OK
    assert (fi.sample_rate, fi.channels, fi.bits_per_sample, fi.total_frames) == (fs, channels, 16, frames)
    assert fi.max_block == (block if len(fb) > 1 else frames)
    # STREAMINFO's other fields, read straight from the block
    si = int.from_bytes(out[8:26], "big")
    assert si >> 128 == (block if len(fb) > 1 else frames)                  # min block size
    assert (si >> 88) & 0xFFFFFF == fb.min() and (si >> 64) & 0xFFFFFF == fb.max()
    zero = flacio.flac_container(payload, fb, fs, channels, frames, block, None)
    assert zero[26:42] == bytes(16) and zero[:26] == out[:26] and zero[42:] == out[42:]


def test_container_of_no_frames():
    from amx import capi, flacio
    out = flacio.flac_container(b"", [], 48000, 2, 0, 4096, None)
    assert len(out) == 4 + 38 and out[:4] == b"fLaC"
    L = capi.load()
    fi = capi.FlacInfo()
    raw = np.frombuffer(out, np.uint8)
    assert L.amx_flac_info(ctypes.c_void_p(raw.ctypes.data), raw.size, ctypes.byref(fi)) == capi.AMX_OK
    assert (fi.sample_rate, fi.channels, fi.bits_per_sample, fi.total_frames) == (48000, 2, 16, 0)
    got, _ = flacio.decode_flac(out)
    assert got.shape == (0, 2)


def test_container_rejects_a_wrong_frame_count():
    from amx import flacio
    with pytest.raises(ValueError):
        flacio.flac_container(b"", [10, 10], 48000, 2, 4096, 4096, None)
