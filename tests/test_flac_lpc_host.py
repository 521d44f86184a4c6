"""CPU: the host side of the FLAC encoder's LPC level -- the LPC-aware reader
(tests/flac_verify_lpc.py) against the in-tree decoder, the streams it must refuse, the
_ex entry points' argument checks, the Python argument check and the numpy model's
(tests/flac_lpc_model.py) own consistency.  The encoder itself is pinned on the GPU
(tests/test_gpu_flac_lpc.py).
"""
import ctypes

import numpy as np
import pytest

import flac_enc
import flac_lpc_model as model
import flac_verify
import flac_verify_lpc


def _music16(frames, C, seed):
    from amx import synth
    x = synth.mix_like(max(frames, 64), 48000, C, seed=seed)[:frames]
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int64)


def _quiet(frames, C, seed):
    """a smooth signal of small amplitude: the generator's LPC residuals stay below 2^13,
    where it may pick 4-bit Rice parameters (what the reader takes without any_rice)"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None]
    x = 900.0 * np.sin(2 * np.pi * t * (0.003 + 0.002 * np.arange(C)[None, :])) + rng.normal(0, 20, (frames, C))
    return np.round(x).astype(np.int64)


# ------------------------------------------------------------------ the reader against the host decoder
@pytest.mark.parametrize("kinds", [["lpc"], ["lpc", "fixed2", "verbatim"]])
@pytest.mark.parametrize("C,block", [(1, 192), (2, 192), (1, 4096), (2, 4096)])
def test_reader_matches_host_decoder(C, block, kinds):
    """tests/flac_enc.py streams with LPC subframes (random order 1..12, precision, shift,
    wasted bits, all four stereo assignments): what the reader decodes equals what
    amx_flac_decode decodes.  The generator draws 5-bit Rice parameters and escapes at
    random, which flac_verify's residual reader refuses by rule, hence any_rice."""
    from amx import flacio
    frames = 3 * block + 50 if block == 192 else block + 100
    lpc_subframes = 0
    for seed in range(3):
        x = _music16(frames, C, seed)
        data = flac_enc.encode(x, 48000, 16, seed=seed, block=block, kinds=kinds)
        want, _ = flacio.decode_flac(data)
        np.testing.assert_array_equal(want >> 16, x)
        got, rep = flac_verify_lpc.verify(data, profile=False, any_rice=True)
        np.testing.assert_array_equal(got, want.astype(np.int64) >> 16)
        for fr in flac_verify_lpc.records(rep):
            for sub in fr:
                if sub["type"] >= 32:
                    lpc_subframes += 1
                    assert sub["order"] == sub["type"] - 31 == len(sub["coefficients"]) and sub["shift"] >= 0
    assert lpc_subframes >= (3 if kinds == ["lpc"] else 1)


# ------------------------------------------------------------------ corrupted streams
def _lpc_stream():
    """(data, report) of a one-frame mono stream whose subframe is LPC, read in full"""
    for seed in range(64):
        x = _quiet(192, 1, seed)
        data = flac_enc.encode(x, 48000, 16, seed=seed, block=192, kinds=["lpc"], metadata=False)
        try:
            _, rep = flac_verify_lpc.verify(data, profile=False)
        except flac_verify.FlacFormatError:
            continue
        if rep["frames"][0]["subframes"][0]["wasted"] == 0:
            return data, rep
    raise AssertionError("no seed gives a readable LPC stream")


def _patched(data, rep, bit, value, nbits):
    """the stream with nbits at `bit` of frame 0 replaced by value, the CRC-16 recomputed
    with the generator's crc16 (the header and its CRC-8 are untouched)"""
    fr = rep["frames"][0]
    off, n = fr["offset"], fr["length"]
    body = int.from_bytes(data[off:off + n - 2], "big")
    total = 8 * (n - 2)
    sh = total - bit - nbits
    body = (body & ~(((1 << nbits) - 1) << sh)) | (value << sh)
    raw = body.to_bytes(n - 2, "big")
    assert flac_enc.crc8(raw[:fr["header_bytes"] - 1]) == raw[fr["header_bytes"] - 1]
    return data[:off] + raw + flac_enc.crc16(raw).to_bytes(2, "big") + data[off + n:]


def test_corrupted_lpc_fields_are_refused():
    data, rep = _lpc_stream()
    sub = rep["frames"][0]["subframes"][0]
    field = sub["start_bit"] + 8 + 16 * sub["order"]            # after the warm-up samples
    same = _patched(data, rep, field, sub["precision"] - 1, 4)
    assert same == data                                          # the patch finds the field
    with pytest.raises(flac_verify.FlacFormatError) as e:
        flac_verify_lpc.verify(_patched(data, rep, field, 15, 4), profile=False)
    assert e.value.rule == "lpc_precision_invalid"
    with pytest.raises(flac_verify.FlacFormatError) as e:
        flac_verify_lpc.verify(_patched(data, rep, field + 4, 0b10011, 5), profile=False)
    assert e.value.rule == "lpc_shift_negative"
    # the reader without LPC still refuses the stream by name, and is itself again afterwards
    with pytest.raises(flac_verify.FlacFormatError) as e:
        flac_verify.verify(data)
    assert e.value.rule == "subframe_lpc"


# ------------------------------------------------------------------ ABI
def test_encode_size_ex():
    from amx import capi
    L = capi.load()
    assert capi.ABI_VERSION == 6 == L.amx_abi_version()
    a = [ctypes.c_int64() for _ in range(3)]
    b = [ctypes.c_int64() for _ in range(3)]
    for frames, C, block in ((1, 1, 16), (4097, 2, 4096), (15, 3, 1152), (3 * 4096 + 1000, 6, 1000),
                             (4613, 8, 4608)):
        assert L.amx_flac_encode_size(frames, C, block, *map(ctypes.byref, a)) == capi.AMX_OK
        assert L.amx_flac_encode_size_ex(frames, C, block, 0, *map(ctypes.byref, b)) == capi.AMX_OK
        assert [v.value for v in a] == [v.value for v in b]
        assert L.amx_flac_encode_size_ex(frames, C, block, 8, *map(ctypes.byref, b)) == capi.AMX_OK
        assert (a[0].value, a[1].value) == (b[0].value, b[1].value) and b[2].value > a[2].value
    for bad in (-1, 9):
        assert L.amx_flac_encode_size_ex(4096, 2, 4096, bad, *map(ctypes.byref, b)) == capi.AMX_ERANGE


# ------------------------------------------------------------------ Python
@pytest.mark.parametrize("bad", [9, -1, 2.0, "8", None, True])
def test_write_flac_refuses_a_bad_order(tmp_path, bad):
    from amx import flacio
    path = tmp_path / "x.flac"
    with pytest.raises(ValueError):
        flacio.write_flac(str(path), np.zeros((16, 2), np.int16), 48000, lpc_order=bad)
    assert not path.exists()


# ------------------------------------------------------------------ the model's own consistency
def test_model_self_check():
    from amx import synth
    x = synth.mix_like(4 * 4096, 48000, 2, seed=7)
    x = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)[:4096, 0].astype(np.int64)
    cands = model.lpc_candidates(x, 16, 8)
    assert cands
    order = min(cands, key=lambda o: cands[o][0])
    bits, shift, q = cands[order]
    assert 1 <= order <= 8 and len(q) == order and 0 <= shift <= 15 and all(-2048 <= c <= 2047 for c in q)
    assert bits == model.subframe_bits(x, 16, 8) < model.subframe_bits(x, 16, 0)
    res = model.lpc_residual(x, q, shift)
    xs = [int(v) for v in x]
    mine = [xs[i] - (sum(q[j] * xs[i - 1 - j] for j in range(order)) >> shift) for i in range(order, len(xs))]
    assert mine == [int(v) for v in res]
    # the window and the autocorrelation in plain Python integers
    n = len(xs)
    W = [(255 * 4 * (i + 1) * (n - i)) // ((n + 1) ** 2) for i in range(n)]
    assert W == [int(v) for v in model.window(n)] and max(W) <= 255 and min(W) >= 0
    xw = [a * b for a, b in zip(xs, W)]
    assert model.autocorr(x, 8) == [sum(xw[i] * xw[i - l] for i in range(l, n)) for l in range(9)]
