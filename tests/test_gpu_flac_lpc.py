"""GPU: the device FLAC encoder with LPC prediction (lpc_order 1..8, k_flac_lpc in
csrc/amx_flacenc.hip; DESIGN.md 3.10 "LPC").

The search space is the specification, LPC included: the predictor's derivation is fixed
down to the operation order, so tests/flac_lpc_model.py recomputes the encoder's
coefficients bit for bit and every subframe's size must EQUAL the model's minimum.  Every
stream goes through the in-tree decoder and through tests/flac_verify_lpc.py (the strict
RFC 9639 reader plus LPC subframes) with profile=True.  lpc_order 0 must stay what
amx_flac_encode writes, byte for byte.
"""
import ctypes
import hashlib
import os
import tempfile

import numpy as np
import pytest

import flac_lpc_model as model
import flac_verify_lpc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _encode(x16, fs, block, lpc_order=0):
    """(file bytes with MD5, frame_bytes, sub_bits [n_frames, C]) of an int16 array"""
    import torch
    from amx import flacio
    d = torch.from_numpy(np.ascontiguousarray(x16)).cuda()
    payload, fb, sb = flacio.encode_flac_device(d, fs, block, sub_bits=True, lpc_order=lpc_order)
    fb, sb = fb.cpu().numpy(), sb.cpu().numpy()
    md5 = hashlib.md5(np.ascontiguousarray(x16, "<i2").tobytes()).digest()
    data = flacio.flac_container(payload.cpu().numpy().tobytes(), fb, fs, x16.shape[1], x16.shape[0], block, md5)
    return data, fb, sb


def _candidate(seg, assign, c):
    """(samples, width) of the subframe of channel c under the frame's channel assignment"""
    if assign < 8:
        return seg[:, c], 16
    l, r = seg[:, 0], seg[:, 1]
    kind = {8: ("l", "s"), 9: ("s", "r"), 10: ("m", "s")}[assign][c]
    return {"l": (l, 16), "r": (r, 16), "m": ((l + r) >> 1, 16), "s": (l - r, 17)}[kind]


def _check(x16, fs, block, M, data, fb, sb):
    """round trip, the reader with the profile, the exact optimum, the coefficients; returns
    the number of LPC subframes the stream holds"""
    from amx import flacio
    frames, C = x16.shape
    got, _ = flacio.decode_flac(data)
    np.testing.assert_array_equal(got, x16.astype(np.int32) << 16)
    dec, rep = flac_verify_lpc.verify(data, profile=True, frame_bytes=fb, lpc_order=M)
    np.testing.assert_array_equal(dec, x16.astype(np.int64))
    assert rep["md5_checked"]
    nf = -(-frames // block)
    assert len(fb) == nf and len(data) == 42 + int(fb.sum())
    want = model.frame_minima(x16, block, M)
    x = x16.astype(np.int64)
    n_lpc = 0
    for k in range(nf):
        if C == 2:
            assert int(sb[k].sum()) == want[k], (k, sb[k], want[k])
        else:
            assert [int(v) for v in sb[k]] == want[k], (k, sb[k], want[k])
        seg = x[k * block:(k + 1) * block]
        fr = rep["frames"][k]
        for c, sub in enumerate(fr["subframes"]):
            assert sub["bits"] == int(sb[k, c])
            if sub["type"] < 32:
                continue
            n_lpc += 1
            s, w = _candidate(seg, fr["assignment"], c)
            o = sub["order"]
            assert 1 <= o <= min(M, len(s) - 1)
            bits, shift, q = model.lpc_candidates(s, w, M)[o]
            assert (sub["shift"], sub["coefficients"], sub["bits"]) == (shift, q, bits), (k, c, o)
    return n_lpc


def _music(frames, C, fs, seed):
    from amx import synth
    x = synth.mix_like(max(frames, 64), fs, C, seed=seed)[:frames]
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def _ar2(frames, seed=3):
    """AR(2) noise, poles of radius 0.97 at fs / 4 (y[n] = -0.97^2 y[n - 2] + e[n]), peak 20000"""
    rng = np.random.default_rng(seed)
    e = rng.normal(0, 1, (frames + 200, 2))
    y = np.zeros_like(e)
    for i in range(2, len(e)):
        y[i] = e[i] - 0.97 ** 2 * y[i - 2]
    y = y[200:]
    return np.round(y * (20000.0 / np.abs(y).max())).astype(np.int16)


# ------------------------------------------------------------------ 1: exact optimum and round trip
SHAPES = [(1, 48000, 4096, 4096, 8), (2, 44100, 3 * 4096 + 1000, 4096, 8), (2, 48000, 4097, 4096, 8),
          (3, 48000, 15, 1152, 8), (2, 48000, 41, 16, 8), (8, 192000, 4613, 4608, 8), (6, 96000, 2000, 1000, 4),
          (2, 48000, 8192, 4096, 1)]


@pytest.mark.parametrize("C,fs,frames,block,M", SHAPES)
def test_exact_optimum_and_round_trip(gpu, C, fs, frames, block, M):
    x = _music(frames, C, fs, seed=C * 100 + block + M)
    data, fb, sb = _encode(x, fs, block, M)
    n_lpc = _check(x, fs, block, M, data, fb, sb)
    if M == 8 and block == 4096:
        assert n_lpc > 0                      # music in blocks of 4096: LPC is chosen somewhere


# ------------------------------------------------------------------ 2: signals
def _signals(frames):
    rng = np.random.default_rng(1234)
    t = np.arange(frames)
    z = np.zeros((frames, 2), np.int16)
    two = lambda v: np.stack([v, v], axis=1).astype(np.int16)   # noqa: E731
    alt = np.where(t % 2 == 0, 32767, -32768)
    sig = {"ar2": _ar2(frames), "noise": np.clip(np.round(rng.normal(0, 3000, (frames, 2))), -32768, 32767).astype(np.int16),
           "silence": z.copy(), "dc": np.full((frames, 2), 1234, np.int16), "alternating": two(alt),
           "square14": two(np.where(t % 14 < 7, 32767, -32768)),
           "sine1k": two(np.round(32767.0 * np.sin(2 * np.pi * 1000.0 * t / 48000.0))),
           "opposed": np.stack([alt, -1 - alt], axis=1).astype(np.int16)}
    imp = z.copy()
    imp[0] = 32767
    sig["impulse"] = imp
    return sig


SIGNALS = ["ar2", "noise", "silence", "dc", "alternating", "square14", "sine1k", "opposed", "impulse"]


@pytest.mark.parametrize("block", [4096, 1000])
@pytest.mark.parametrize("name", SIGNALS)
def test_signals(gpu, name, block):
    frames, fs = 2 * 4096, 48000
    if name == "impulse":
        # one impulse at sample 0 of every block, the rest silent: in a block of 4096 the
        # window zeroes it (R[0] == 0); in one of 1000 W[0] is 1 and every R[l > 0] is 0, so
        # all coefficients are 0 -- no LPC candidate either way
        x = np.zeros((frames, 2), np.int16)
        x[::block] = 32767
        assert (model.autocorr(x[:block, 0], 8)[0] == 0) == (block == 4096)
        assert not model.predictors(x[:block, 0], 8)
    else:
        x = _signals(frames)[name]
    data, fb, sb = _encode(x, fs, block, 8)
    n_lpc = _check(x, fs, block, 8, data, fb, sb)
    if name == "noise":
        np.testing.assert_array_equal(sb, _encode(x, fs, block, 0)[2])
    if name in ("silence", "dc", "impulse"):
        assert n_lpc == 0


# ------------------------------------------------------------------ 3: it pays
@pytest.mark.parametrize("name", ["mix_like", "ar2"])
def test_it_pays_and_is_monotonic(gpu, name):
    x = _music(4 * 4096, 2, 48000, seed=7) if name == "mix_like" else _ar2(4 * 4096)
    sums = [_encode(x, 48000, 4096, m)[2].astype(np.int64).sum(axis=1) for m in range(9)]
    print("sub_bits totals by lpc_order:", [int(s.sum()) for s in sums])
    assert sums[8].sum() <= 0.95 * sums[0].sum()
    for m in range(1, 9):
        assert (sums[m] <= sums[m - 1]).all(), m


# ------------------------------------------------------------------ 4-5: the C ABI
SENTINEL = 0xA5


class _Raw:
    """an encode through the C ABI on buffers the test owns, every one pre-filled with 0xA5:
    d_out of the asked capacity with 64 spare bytes behind (and out_shift before), the
    workspace with 64 spare bytes behind"""

    def __init__(self, frames, C, block, lpc_order, entry="ex", out_shift=0):
        import torch
        from amx import capi
        self.L, self.capi, self.torch = capi.load(), capi, torch
        self.args, self.M, self.entry, self.shift = (frames, C, block), lpc_order, entry, out_shift
        nf, cap, wsb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        refs = [ctypes.byref(v) for v in (nf, cap, wsb)]
        rc = (self.L.amx_flac_encode_size_ex(frames, C, block, lpc_order, *refs) if entry == "ex"
              else self.L.amx_flac_encode_size(frames, C, block, *refs))
        assert rc == capi.AMX_OK
        self.nf, self.cap, self.wsb = nf.value, cap.value, (wsb.value + 7) // 8 * 8
        fill = lambda n, dt: torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda").view(dt)   # noqa: E731
        self.store = fill(out_shift + self.cap + 64, torch.uint8)
        self.ws = fill(self.wsb + 64, torch.uint8)
        self.fb = fill(4 * self.nf, torch.int32)
        self.sb = fill(4 * self.nf * C, torch.int32)
        self.total = fill(8, torch.int64)

    def encode(self, x16, fs):
        torch, capi = self.torch, self.capi
        frames, C, block = self.args
        d = torch.from_numpy(np.ascontiguousarray(x16)).cuda()
        head = (capi.ptr(d), frames, C, fs, block)
        tail = (capi.ptr(self.store[self.shift:]), self.cap, capi.ptr(self.fb), capi.ptr(self.sb),
                capi.ptr(self.total), capi.ptr(self.ws), self.wsb, capi.ptr_stream())
        rc = (self.L.amx_flac_encode_ex(*head, self.M, *tail) if self.entry == "ex"
              else self.L.amx_flac_encode(*head, *tail))
        torch.cuda.synchronize()
        assert rc == capi.AMX_OK
        n = int(self.total.item())
        assert 0 < n <= self.cap
        store, ws = self.store.cpu().numpy(), self.ws.cpu().numpy()
        assert (store[:self.shift] == SENTINEL).all() and (store[self.shift + n:] == SENTINEL).all()
        assert (ws[self.wsb:] == SENTINEL).all()
        return (store[self.shift:self.shift + n].tobytes(), self.fb.cpu().numpy().copy(),
                self.sb.cpu().numpy().reshape(self.nf, C).copy())


@pytest.mark.parametrize("C,fs,frames,block", [(2, 48000, 3 * 4096 + 1000, 4096), (1, 44100, 4097, 1152),
                                               (6, 96000, 2000, 1000)])
def test_level_0_is_untouched(gpu, C, fs, frames, block):
    """lpc_order 0, by the Python default and by amx_flac_encode_ex: the payload, the frame
    lengths and the subframe sizes of amx_flac_encode, byte for byte"""
    import torch
    from amx import flacio
    x = _music(frames, C, fs, seed=frames + C)
    want = _Raw(frames, C, block, 0, entry="old").encode(x, fs)
    ex = _Raw(frames, C, block, 0, entry="ex").encode(x, fs)
    payload, fb, sb = flacio.encode_flac_device(torch.from_numpy(x).cuda(), fs, block, sub_bits=True)
    py = (payload.cpu().numpy().tobytes(), fb.cpu().numpy(), sb.cpu().numpy())
    for got in (ex, py):
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])


def test_deterministic_and_within_its_buffers(gpu):
    """lpc_order 8 twice from the Python side; then through the C ABI into buffers pre-filled
    with 0xA5 (_Raw checks the bytes after the stream and after the workspace), and with the
    output pointer moved by one byte: the same stream every time"""
    frames, block, fs = 3 * 4096 + 1000, 4096, 48000
    x = _music(frames, 2, fs, seed=91)
    a, b = _encode(x, fs, block, 8), _encode(x, fs, block, 8)
    assert a[0] == b[0]
    raw = _Raw(frames, 2, block, 8).encode(x, fs)
    moved = _Raw(frames, 2, block, 8, out_shift=1).encode(x, fs)
    assert raw[0] == moved[0] == a[0][42:]
    np.testing.assert_array_equal(raw[1], a[1])
    np.testing.assert_array_equal(raw[2], a[2])


# ------------------------------------------------------------------ 6: master_audio
def test_master_audio_flac_lpc_order(gpu):
    import audio_mastering_engine as ame
    from amx import flacio, synth, wavio
    fs = 48000
    src_x = synth.mix_like(fs * 2, fs, 2, seed=73).astype(np.float32)
    settings = dict(bass_boost=1.0, presence_boost=1.5, width=1.2)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in.wav")
        wavio.write_wav_pcm(src, src_x, fs, "f32")
        out = {}
        for name, extra in (("m.wav", dict(flac_lpc_order=8)), ("m.flac", dict(flac_lpc_order=8)), ("m0.flac", {})):
            dst = os.path.join(d, name)
            assert ame.master_audio(dict(settings, input_file=src, output_file=dst, **extra)) == dst
            out[name] = open(dst, "rb").read()
        y, info = wavio.read_wav_native(os.path.join(d, "m.wav"))
    y = np.asarray(y).reshape(-1, info.channels)
    dec, rep = flac_verify_lpc.verify(out["m.flac"], profile=True, lpc_order=8)
    np.testing.assert_array_equal(dec, y.astype(np.int64))
    assert rep["md5_checked"] and any(s["type"] >= 32 for fr in rep["frames"] for s in fr["subframes"])
    assert len(out["m.flac"]) <= len(out["m0.flac"])
    assert out["m0.flac"] == flacio.flac_bytes(y.astype(np.int16), info.sample_rate, lpc_order=0)
