"""GPU: the device FLAC encoder (amx_flac_encode, csrc/amx_flacenc.hip) and the *.flac
ending of master_audio.

The encoder is pinned three ways: the in-tree decoder (amx_flac_decode, itself pinned by
tests/flac_enc.py) must give the samples back bit for bit; every subframe's size must
EQUAL the minimum a brute-force numpy search finds over the encoder's search space
(the search space is the specification, so this is an equality); and the
container's sizes, MD5 and argument errors are checked directly.

Every stream also goes through tests/flac_verify.py, a strict reader written from RFC 9639
alone that shares no code with the in-tree decoder, with profile=True (the encoder's own
promises): that pins what amx_flac_decode skips or accepts either way -- the
coded frame number and its shortest coding, the rate, sample-size and block-size codes and
their extra bytes against STREAMINFO, the blocking strategy, the reserved and padding bits,
STREAMINFO's block and frame sizes, and that each frame starts where the lengths the encoder
reports say (the placement scan over more than 1024 frames, 3- and 4-byte frame numbers).
The direct C ABI tests hold the encoder to its buffers: canaries behind the stream and the
arrays, buffers reused without clearing, an output pointer at any alignment.  What is still
not pinned: no third-party FLAC implementation is involved, so the reader and the encoder
share one person's reading of the RFC.
"""
import ctypes
import hashlib
import os
import tempfile

import numpy as np
import pytest

import flac_verify

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ brute force
def _fixed_bits(x, w, o):
    """smallest FIXED(o) subframe of samples x (int64) at w bits: 8 + o w + 6 + min over the
    partition order of sum over partitions of (4 + min over k of [n (k + 1) + sum(u >> k)])"""
    n = len(x)
    r = x.copy()
    for _ in range(o):
        r = np.diff(r)
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    u = np.concatenate([np.zeros(o, np.int64), u])        # warm-up samples: no code
    tz = (n & -n).bit_length() - 1
    best = None
    for p in range(0, min(6, tz) + 1):
        plen = n >> p
        if plen < o:
            continue
        cnt = np.full(1 << p, plen, np.int64)
        cnt[0] -= o
        per_k = np.stack([cnt * (k + 1) + (u >> k).reshape(1 << p, plen).sum(axis=1) for k in range(15)])
        total = int((4 + per_k.min(axis=0)).sum())
        best = total if best is None else min(best, total)
    return 8 + o * w + 6 + best


def _subframe_bits(x, w):
    x = np.asarray(x, np.int64)
    n = len(x)
    cands = [8 + n * w]
    if np.all(x == x[0]):
        cands.append(8 + w)
    for o in range(0, min(4, n) + 1):
        cands.append(_fixed_bits(x, w, o))
    return min(cands)


def _brute_force(x16, block):
    """per frame: the subframe minima per channel (C != 2), or for stereo the minimum of the
    four assignments' sums; returns a list of ints (C == 2) or of per-channel lists"""
    x = np.asarray(x16, np.int64)
    out = []
    for s in range(0, len(x), block):
        seg = x[s:s + block]
        if seg.shape[1] != 2:
            out.append([_subframe_bits(seg[:, c], 16) for c in range(seg.shape[1])])
            continue
        l, r = seg[:, 0], seg[:, 1]
        bl, br = _subframe_bits(l, 16), _subframe_bits(r, 16)
        bm, bs = _subframe_bits((l + r) >> 1, 16), _subframe_bits(l - r, 17)
        out.append(min(bl + br, bl + bs, bs + br, bm + bs))
    return out


# ------------------------------------------------------------------ helpers
def _encode(x16, fs, block):
    """(file bytes with MD5, frame_bytes, sub_bits [n_frames, C]) of an int16 array"""
    import torch
    from amx import flacio
    d = torch.from_numpy(np.ascontiguousarray(x16)).cuda()
    payload, fb, sb = flacio.encode_flac_device(d, fs, block, sub_bits=True)
    fb, sb = fb.cpu().numpy(), sb.cpu().numpy()
    md5 = hashlib.md5(np.ascontiguousarray(x16, "<i2").tobytes()).digest()
    data = flacio.flac_container(payload.cpu().numpy().tobytes(), fb, fs, x16.shape[1], x16.shape[0], block, md5)
    return data, fb, sb


def _info(data):
    from amx import capi
    fi = capi.FlacInfo()
    raw = np.frombuffer(data, np.uint8)
    assert capi.load().amx_flac_info(ctypes.c_void_p(raw.ctypes.data), raw.size, ctypes.byref(fi)) == capi.AMX_OK
    return fi


def _check_format(x16, data, fb, frames=None):
    """the independent reader on one encode: the stream keeps RFC 9639 and the encoder's
    profile, every frame starts where the reported lengths say, and the samples are the
    input's (frames: decode only these frames fully, tests/flac_verify.py)"""
    got, rep = flac_verify.verify(data, profile=True, frames=frames, frame_bytes=fb)
    if frames is None:
        np.testing.assert_array_equal(got, x16.astype(np.int64))
        assert rep["md5_checked"]
    assert [f["number"] for f in rep["frames"]] == list(range(len(fb)))
    assert [f["length"] for f in rep["frames"]] == [int(v) for v in fb]
    return got, rep


def _check_stream(x16, fs, block, data, fb, sb):
    """round trip, sizes and the exact optimum of one encode"""
    from amx import flacio
    frames, C = x16.shape
    got, _ = flacio.decode_flac(data)
    np.testing.assert_array_equal(got, x16.astype(np.int32) << 16)
    _check_format(x16, data, fb)
    fi = _info(data)
    assert (fi.sample_rate, fi.channels, fi.bits_per_sample, fi.total_frames) == (fs, C, 16, frames)
    # sizes
    nf = -(-frames // block)
    assert len(fb) == nf and len(data) == 42 + int(fb.sum())
    si = int.from_bytes(data[8:26], "big")
    assert (si >> 88) & 0xFFFFFF == fb.min() and (si >> 64) & 0xFFFFFF == fb.max()
    for k in range(nf):
        n = min(block, frames - k * block)
        assert fb[k] <= 16 + -(-(C * (8 + 17 * n)) // 8) + 2, (k, fb[k])
    # the exact optimum
    want = _brute_force(x16, block)
    for k in range(nf):
        if C == 2:
            assert int(sb[k].sum()) == want[k], (k, sb[k], want[k])
        else:
            assert [int(v) for v in sb[k]] == want[k], (k, sb[k], want[k])


def _music(frames, C, fs, seed):
    from amx import synth
    x = synth.mix_like(max(frames, 64), fs, C, seed=seed)[:frames]
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------ 1, 3, 4: shapes
# every C in {1, 2, 3, 6, 8}, rate in {11025, 44100, 48000, 192000, 768000}, length in
# {1, 3, 15, 4095, 4096, 4097, 3 * 4096 + 1000} and block in {16, 1000, 1152, 4096, 4608}
SHAPES = [(1, 11025, 1, 16), (2, 44100, 3, 1000), (3, 48000, 15, 1152), (6, 192000, 4095, 4096),
          (8, 768000, 4096, 4608), (2, 48000, 4097, 4096), (2, 44100, 3 * 4096 + 1000, 1000),
          (1, 48000, 4097, 16), (8, 48000, 4097, 4608), (3, 192000, 3 * 4096 + 1000, 1152),
          (2, 48000, 3 * 4096 + 1000, 4096)]


@pytest.mark.parametrize("C,fs,frames,block", SHAPES)
def test_round_trip_sizes_and_optimum(gpu, C, fs, frames, block):
    x = _music(frames, C, min(fs, 192000), seed=C * 100 + block)
    data, fb, sb = _encode(x, fs, block)
    _check_stream(x, fs, block, data, fb, sb)


# ------------------------------------------------------------------ 2: signals
def _signals(frames):
    rng = np.random.default_rng(1234)
    t = np.arange(frames)
    z = np.zeros((frames, 2), np.int16)
    sig = {}
    sig["silence"] = z.copy()
    sig["dc"] = np.full((frames, 2), 1234, np.int16)
    sig["noise"] = rng.integers(-32768, 32768, (frames, 2)).astype(np.int16)
    alt = np.where(t % 2 == 0, 32767, -32768).astype(np.int16)
    sig["alternating"] = np.stack([alt, alt], axis=1)
    ramp = (t * 2 - 12000).astype(np.int16)
    sig["ramp"] = np.stack([ramp, ramp], axis=1)
    sp = z.copy()
    sp[::997] = 3000
    sig["sparse"] = sp
    m = _music(frames, 2, 48000, seed=5)
    sig["l_eq_r"] = np.stack([m[:, 0], m[:, 0]], axis=1)
    neg = np.clip(-m[:, 0].astype(np.int32), -32768, 32767).astype(np.int16)
    sig["l_eq_minus_r"] = np.stack([m[:, 0], neg], axis=1)
    sig["two_noises"] = np.stack([rng.integers(-20000, 20000, frames), rng.integers(-40, 40, frames)],
                                 axis=1).astype(np.int16)
    return sig


SIGNALS = ["silence", "dc", "noise", "alternating", "ramp", "sparse", "l_eq_r", "l_eq_minus_r", "two_noises"]


@pytest.mark.parametrize("name", SIGNALS)
def test_signals(gpu, name):
    frames, block, fs = 2 * 4096 + 1000, 4096, 48000
    x = _signals(frames)[name]
    data, fb, sb = _encode(x, fs, block)
    _check_stream(x, fs, block, data, fb, sb)
    sizes = [min(block, frames - k * block) for k in range(len(fb))]
    if name in ("silence", "dc"):
        assert all(int(sb[k, c]) == 8 + 16 for k in range(len(fb)) for c in range(2))      # CONSTANT
    if name == "noise":
        assert all(int(sb[k, c]) == 8 + 16 * n for k, n in enumerate(sizes) for c in range(2))  # VERBATIM
    if name == "ramp":
        # an order-2 residual of zeros at k = 0: 8 + 2 * 16 + 6 + 4 + (n - 2); the other
        # subframe is the constant side
        assert all(int(sb[k].max()) == 48 + n and int(sb[k].min()) == 8 + 17 for k, n in enumerate(sizes))
    if name == "l_eq_r":
        assert all(int(sb[k].min()) == 8 + 17 for k in range(len(fb)))                      # side == 0
    # the same signal in mono (independent channels only) and in a block no power of two divides far
    xm = np.ascontiguousarray(x[:3000, :1])
    data, fb, sb = _encode(xm, fs, 1000)
    _check_stream(xm, fs, 1000, data, fb, sb)


# ------------------------------------------------------------------ 5: MD5
def test_md5(gpu):
    from amx import flacio
    x = _music(5000, 2, 48000, seed=9)
    with tempfile.TemporaryDirectory() as d:
        a, b, c = (os.path.join(d, n) for n in ("a.flac", "b.flac", "c.flac"))
        import torch
        flacio.write_flac(a, torch.from_numpy(x).cuda(), 48000)
        flacio.write_flac(b, x, 48000, md5=False)
        flacio.write_flac(c, np.zeros((0, 2), np.int16), 48000)
        da, db, dc = (open(p, "rb").read() for p in (a, b, c))
    assert da[26:42] == hashlib.md5(x.astype("<i2").tobytes()).digest()
    assert db[26:42] == bytes(16) and db[:26] == da[:26] and db[42:] == da[42:]
    np.testing.assert_array_equal(flacio.decode_flac(da)[0], x.astype(np.int32) << 16)
    assert len(dc) == 42 and _info(dc).total_frames == 0


# ------------------------------------------------------------------ 6: determinism
def test_deterministic_and_block_independent(gpu):
    from amx import flacio
    x = _music(3 * 4096 + 1000, 2, 48000, seed=10)
    a = _encode(x, 48000, 4096)[0]
    b = _encode(x, 48000, 4096)[0]
    assert a == b
    for block in (1152, 4608):
        c = _encode(x, 48000, block)[0]
        np.testing.assert_array_equal(flacio.decode_flac(c)[0], x.astype(np.int32) << 16)


# ------------------------------------------------------------------ 7: argument errors
def test_argument_errors(gpu):
    import torch
    from amx import capi
    L = capi.load()
    x = torch.zeros((4096, 2), dtype=torch.int16, device="cuda")
    nf, cap, wsb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert L.amx_flac_encode_size(4096, 2, 4096, ctypes.byref(nf), ctypes.byref(cap), ctypes.byref(wsb)) == capi.AMX_OK
    assert nf.value == 1 and cap.value >= 16 + 2 * (8 + 17 * 4096) // 8 + 2 and wsb.value > 0
    out = torch.full((cap.value,), 0x55, dtype=torch.uint8, device="cuda")
    fb = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    total = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros((wsb.value + 7) // 8, dtype=torch.int64, device="cuda")

    def call(frames=4096, channels=2, fs=48000, block=4096, capacity=None, pcm=x):
        return L.amx_flac_encode(capi.ptr(pcm), frames, channels, fs, block, capi.ptr(out),
                                 cap.value if capacity is None else capacity, capi.ptr(fb), None,
                                 capi.ptr(total), capi.ptr(ws), ws.numel() * 8, capi.ptr_stream())

    assert call(channels=0) == capi.AMX_EINVAL
    assert call(channels=9) == capi.AMX_EINVAL
    assert call(frames=0) == capi.AMX_EINVAL
    assert call(pcm=None) == capi.AMX_EINVAL
    assert call(block=8) == capi.AMX_ERANGE
    assert call(block=5000) == capi.AMX_ERANGE
    assert call(fs=0) == capi.AMX_ERANGE
    assert call(fs=1 << 20) == capi.AMX_ERANGE
    assert call(capacity=cap.value - 1) == capi.AMX_ERANGE
    for bad in ((0, 2, 4096), (4096, 0, 4096), (4096, 9, 4096)):
        assert L.amx_flac_encode_size(*bad, ctypes.byref(nf), ctypes.byref(cap), ctypes.byref(wsb)) == capi.AMX_EINVAL
    for bad in ((4096, 2, 8), (4096, 2, 5000)):
        assert L.amx_flac_encode_size(*bad, ctypes.byref(nf), ctypes.byref(cap), ctypes.byref(wsb)) == capi.AMX_ERANGE
    # none of these launched anything: the outputs are untouched
    torch.cuda.synchronize()
    assert int(total.item()) == -7 and bool((fb == -7).all()) and bool((out == 0x55).all())
    assert call() == capi.AMX_OK
    torch.cuda.synchronize()
    assert int(total.item()) == int(fb[0].item()) > 0


# ------------------------------------------------------------------ 8: master_audio
C3 = dict(bass_boost=-1.0, mid_cut=2.0, presence_boost=2.5, treble_boost=1.0, lufs=-14.0, width=1.3,
          analog_character=40.0, multiband=True, low_thresh=-25.0, low_ratio=6.0, mid_thresh=-20.0,
          mid_ratio=3.0, high_thresh=-15.0, high_ratio=4.0)


def _dynamic_signal(seconds, fs, seed):
    """quiet program with sparse full-scale transients (tests/test_gpu_dynamic.py's loud
    input): TP + offset > -1.5 dBTP, so loudnorm takes dynamic mode"""
    from amx import synth
    n = int(fs * seconds)
    x = synth.mix_like(n, fs, 2, seed=seed) * 0.12
    rng = np.random.default_rng(seed)
    for k in rng.integers(0, n - 200, max(2, int(seconds * 2))):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, 2))
    return np.clip(x, -1.0, 1.0).astype(np.float32)


@pytest.mark.parametrize("kind,flac_name,out_fs", [("stereo", "out.flac", None), ("stereo_linear", "out.flac", 48000),
                                                   ("six", "OUT.FLAC", 48000), ("dynamic", "out.flac", 192000)])
def test_master_audio_writes_flac(gpu, kind, flac_name, out_fs):
    """master_audio to out.wav and to a *.flac name: the same samples, rate, channels, status
    and progress sequences; the DSP is pinned elsewhere, this holds the container.  (A 3 s
    C3 track is too short for loudnorm's linear mode, so "stereo" ends in the 192 kHz
    output like "dynamic"; "stereo_linear" is C3 without lufs, the 48 kHz stereo ending.)"""
    import audio_mastering_engine as ame
    from amx import flacio, synth, wavio
    fs = 48000
    if kind in ("stereo", "stereo_linear"):
        src_x, code = synth.mix_like(fs * 3, fs, 2, seed=71).astype(np.float32), "f32"
        settings = dict(C3) if kind == "stereo" else dict(C3, lufs=None)
    elif kind == "six":
        x = synth.mix_like(fs * 2, fs, 6, seed=72)
        src_x, code = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16), "s16"
        # (no lufs: a track this short measures LRA 0, loudnorm's dynamic mode, which a
        # 3-8-channel file refuses -- tests/test_gpu_multichannel.py pins that)
        settings = dict(C3, lufs=None)
    else:
        src_x, code, settings = _dynamic_signal(2.0, fs, 11), "f32", dict(bass_boost=1.0, lufs=-14.0)
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in.wav")
        wavio.write_wav_pcm(src, src_x, fs, code)
        runs = {}
        for name in ("out.wav", flac_name):
            st, pr = [], []
            dst = os.path.join(d, name)
            assert ame.master_audio(dict(settings, input_file=src, output_file=dst), st.append,
                                    lambda a, b: pr.append((a, b))) == dst
            runs[name] = (st, pr, open(dst, "rb").read())
        y, info = wavio.read_wav_native(os.path.join(d, "out.wav"))
        again = os.path.join(d, "again.wav")
        wavio.write_wav_s16(again, y, info.sample_rate)
        assert open(again, "rb").read() == runs["out.wav"][2]
    assert runs["out.wav"][0] == runs[flac_name][0] and runs["out.wav"][1] == runs[flac_name][1]
    data = runs[flac_name][2]
    assert data[:4] == b"fLaC"
    got, _ = flacio.decode_flac(data)
    fi = _info(data)
    assert out_fs is None or info.sample_rate == out_fs
    assert (fi.sample_rate, fi.channels, fi.bits_per_sample) == (info.sample_rate, info.channels, 16)
    assert fi.total_frames == y.shape[0] > 0
    np.testing.assert_array_equal(got, y.astype(np.int32).reshape(got.shape) << 16)
    assert data[26:42] == hashlib.md5(np.ascontiguousarray(y, "<i2").tobytes()).digest()


# ------------------------------------------------------------------ 9: the placement scan's passes
@pytest.mark.parametrize("C,nf,tail", [(2, 1023, 0), (2, 1024, 0), (2, 1025, 0), (2, 2049, 0), (1, 1025, 0),
                                       (8, 1025, 5)])
def test_placement_passes(gpu, C, nf, tail):
    """k_flac_place scans 1024 frame lengths at a time and carries the sum: frame counts
    around one and two passes, music so that the lengths vary and the offsets land on every
    alignment.  tail: the last of the nf frames holds 5 samples."""
    from amx import flacio
    block = 16
    frames = block * nf if not tail else block * (nf - 1) + tail
    x = _music(frames, C, 48000, seed=nf + C)
    data, fb, sb = _encode(x, 48000, block)
    assert len(fb) == nf and int(fb.astype(np.int64).sum()) == len(data) - 42
    assert len(set(int(v) for v in fb)) > 1
    offs = 42 + np.concatenate([[0], np.cumsum(fb.astype(np.int64))[:-1]])
    assert set(int(o) & 3 for o in offs) == {0, 1, 2, 3}
    assert all(data[o] == 0xFF and data[o + 1] == 0xF8 for o in offs)
    _check_format(x, data, fb)
    got, _ = flacio.decode_flac(data)
    np.testing.assert_array_equal(got, x.astype(np.int32) << 16)


# ------------------------------------------------------------------ 10: 3- and 4-byte frame numbers
def test_long_numbering(gpu):
    """65 537 frames (mono, block 16, a last frame of 5 samples): frame numbers of 1 to 4
    bytes and 65 passes of the placement scan.  The reader checks every header and steps by
    the reported lengths; it decodes the frames around each change of the number's length."""
    from amx import flacio
    block, frames = 16, 16 * 65536 + 5
    m = _music(65536, 1, 48000, seed=21)
    x = np.ascontiguousarray(np.concatenate([m] * 16 + [m[:5]]))
    assert x.shape == (frames, 1)
    data, fb, sb = _encode(x, 48000, block)
    assert len(fb) == 65537 and int(fb.astype(np.int64).sum()) == len(data) - 42
    got, _ = flacio.decode_flac(data)
    np.testing.assert_array_equal(got, x.astype(np.int32) << 16)
    full = sorted(set(k + d for k in (0, 127, 128, 2047, 2048, 65535, 65536) for d in (-1, 0, 1)
                      if 0 <= k + d <= 65536))
    part, rep = _check_format(x, data, fb, frames=full)
    for k in full:
        assert rep["frames"][k]["decoded"]
        np.testing.assert_array_equal(part[k * block:(k + 1) * block], x[k * block:(k + 1) * block].astype(np.int64))
    assert [rep["frames"][k]["number_bytes"] for k in (0, 127, 128, 2047, 2048, 65535, 65536)] == [1, 1, 2, 2, 3, 3, 4]
    assert rep["frames"][65536]["block"] == 5


# ------------------------------------------------------------------ 11: sample-rate codes
RATE_CODES = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 88200: 1, 176400: 2, 352800: 14, 384000: 14,
              655350: 0, 65535: 13, 65536: 0, 1048575: 0}


@pytest.mark.parametrize("fs", list(RATE_CODES))
def test_rate_codes(gpu, fs):
    """table rates, Hz in 16 bits (up to 65 535), tens of Hz in 16 bits (below 655 350), and
    the rates only STREAMINFO can hold (code 0)"""
    block, frames = 1152, 3 * 1152 + 100
    x = _music(frames, 2, 48000, seed=31)
    data, fb, sb = _encode(x, fs, block)
    _check_stream(x, fs, block, data, fb, sb)
    rep = flac_verify.verify(data, profile=True)[1]
    assert rep["sample_rate"] == fs and [f["rate_code"] for f in rep["frames"]] == [RATE_CODES[fs]] * 4


# ------------------------------------------------------------------ 12: block-size codes
BLOCK_CODES = {192: 1, 576: 2, 2304: 4, 256: 8, 512: 9, 2048: 11, 255: 6, 257: 7, 4607: 7}


@pytest.mark.parametrize("block", list(BLOCK_CODES))
def test_block_size_codes(gpu, block):
    tail = 37
    x = _music(block + tail, 1, 48000, seed=41)
    data, fb, sb = _encode(x, 48000, block)
    _check_stream(x, 48000, block, data, fb, sb)
    rep = flac_verify.verify(data, profile=True)[1]
    assert [(f["block"], f["block_code"]) for f in rep["frames"]] == [(block, BLOCK_CODES[block]), (tail, 6)]


# ------------------------------------------------------------------ 13: the side channel's extremes
def _extremes(n):
    t = np.arange(n)
    hi, lo = np.full(n, 32767, np.int16), np.full(n, -32768, np.int16)
    alt = np.where(t % 2 == 0, 32767, -32768).astype(np.int16)
    neg = np.where(t % 2 == 0, -32768, 32767).astype(np.int16)
    return {"side_max": np.stack([hi, lo], axis=1), "side_min": np.stack([lo, hi], axis=1),
            "alternating_opposed": np.stack([alt, neg], axis=1), "both_min": np.stack([lo, lo], axis=1)}


@pytest.mark.parametrize("block", [4096, 1000])
@pytest.mark.parametrize("name", ["side_max", "side_min", "alternating_opposed", "both_min"])
def test_side_channel_extremes(gpu, name, block):
    """one block of L - R = +-65535 (17 bits), of L and R alternating between the extremes in
    opposition (the order-4 residual of the side channel at its largest), of L = R = -32768"""
    x = np.ascontiguousarray(_extremes(block)[name])
    data, fb, sb = _encode(x, 48000, block)
    _check_stream(x, 48000, block, data, fb, sb)


# ------------------------------------------------------------------ 14-17: the C ABI's buffers
SENTINEL = -7


class _Raw:
    """amx_flac_encode through the C ABI on buffers the test owns: d_out of the asked
    capacity inside an allocation with `spare` bytes of 0x55 behind it (and out_shift bytes
    before it), d_frame_bytes and d_sub_bits with 8 spare entries of SENTINEL"""

    def __init__(self, frames, C, block, spare=64, out_shift=0):
        import torch
        from amx import capi
        self.L, self.capi, self.torch = capi.load(), capi, torch
        nf, cap, wsb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert self.L.amx_flac_encode_size(frames, C, block, ctypes.byref(nf), ctypes.byref(cap),
                                           ctypes.byref(wsb)) == capi.AMX_OK
        self.frames, self.C, self.block, self.nf, self.cap, self.shift = frames, C, block, nf.value, cap.value, out_shift
        self.store = torch.full((out_shift + cap.value + spare,), 0x55, dtype=torch.uint8, device="cuda")
        self.fb = torch.full((nf.value + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        self.sb = torch.full((nf.value * C + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        self.total = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
        self.ws = torch.full(((wsb.value + 7) // 8 + 1,), SENTINEL, dtype=torch.int64, device="cuda")

    def encode(self, x16, fs, ws_shift=0):
        """(rc, stream bytes up to total or None)"""
        torch, capi = self.torch, self.capi
        d = torch.from_numpy(np.ascontiguousarray(x16)).cuda()
        assert d.shape == (self.frames, self.C)
        ws = ctypes.c_void_p(self.ws.data_ptr() + ws_shift)
        rc = self.L.amx_flac_encode(capi.ptr(d), self.frames, self.C, fs, self.block, capi.ptr(self.store[self.shift:]),
                                    self.cap, capi.ptr(self.fb), capi.ptr(self.sb), capi.ptr(self.total), ws,
                                    self.ws.numel() * 8 - 8, capi.ptr_stream())
        torch.cuda.synchronize()
        if rc != capi.AMX_OK:
            return rc, None
        n = int(self.total.item())
        assert 0 < n <= self.cap
        return rc, self.store[self.shift:self.shift + n].cpu().numpy().tobytes()

    def untouched_beyond(self, n):
        """every byte of the allocation before d_out and from d_out + n on, and every spare
        entry, is as it was filled"""
        store = self.store.cpu().numpy()
        assert (store[:self.shift] == 0x55).all() and (store[self.shift + n:] == 0x55).all()
        assert bool((self.fb[self.nf:] == SENTINEL).all()) and bool((self.sb[self.nf * self.C:] == SENTINEL).all())

    def file(self, x16, fs, payload):
        from amx import flacio
        md5 = hashlib.md5(np.ascontiguousarray(x16, "<i2").tobytes()).digest()
        fb = self.fb[:self.nf].cpu().numpy()
        return flacio.flac_container(payload, fb, fs, self.C, self.frames, self.block, md5), fb


FRAMES_ABI, BLOCK_ABI = 3 * 4096 + 1000, 4096


def test_canaries(gpu):
    """a successful encode writes d_out[0, total), d_frame_bytes[0, n_frames) and
    d_sub_bits[0, n_frames * channels) and nothing else"""
    x = _music(FRAMES_ABI, 2, 48000, seed=51)
    raw = _Raw(FRAMES_ABI, 2, BLOCK_ABI)
    rc, payload = raw.encode(x, 48000)
    assert rc == raw.capi.AMX_OK
    raw.untouched_beyond(len(payload))
    data, fb = raw.file(x, 48000, payload)
    assert int(fb.astype(np.int64).sum()) == len(payload)
    _check_format(x, data, fb)
    sb = raw.sb[:raw.nf * 2].cpu().numpy().reshape(raw.nf, 2)
    _check_stream(x, 48000, BLOCK_ABI, data, fb, sb)


def test_reuse_without_clearing(gpu):
    """the same d_out, workspace, d_frame_bytes and d_total_bytes for full-scale noise (the
    largest frames), silence (the smallest) and music, nothing cleared in between: each
    stream is the input's (the reader) and equals the one encoded into fresh buffers"""
    rng = np.random.default_rng(61)
    inputs = [rng.integers(-32768, 32768, (FRAMES_ABI, 2)).astype(np.int16), np.zeros((FRAMES_ABI, 2), np.int16),
              _music(FRAMES_ABI, 2, 48000, seed=62)]
    used = _Raw(FRAMES_ABI, 2, BLOCK_ABI)
    sizes = []
    for x in inputs:
        rc, payload = used.encode(x, 48000)
        assert rc == used.capi.AMX_OK
        data, fb = used.file(x, 48000, payload)
        _check_format(x, data, fb)
        fresh = _Raw(FRAMES_ABI, 2, BLOCK_ABI)
        rc, want = fresh.encode(x, 48000)
        assert rc == used.capi.AMX_OK and payload == want
        np.testing.assert_array_equal(fb, fresh.fb[:fresh.nf].cpu().numpy())
        np.testing.assert_array_equal(used.sb.cpu().numpy(), fresh.sb.cpu().numpy())
        sizes.append(len(payload))
    assert sizes[0] > sizes[2] > sizes[1]
    used.untouched_beyond(sizes[0])            # the largest of the three reached this far, none further


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_output_pointer_at_any_alignment(gpu, shift):
    """d_out + shift inside a larger allocation: the same stream as at an aligned address,
    and not a byte before d_out or from d_out + total on"""
    x = _music(FRAMES_ABI, 2, 48000, seed=71)
    aligned, moved = _Raw(FRAMES_ABI, 2, BLOCK_ABI), _Raw(FRAMES_ABI, 2, BLOCK_ABI, out_shift=shift)
    assert moved.store.data_ptr() % 4 == 0
    rc, want = aligned.encode(x, 48000)
    assert rc == aligned.capi.AMX_OK
    rc, payload = moved.encode(x, 48000)
    assert rc == moved.capi.AMX_OK and payload == want
    moved.untouched_beyond(len(payload))
    data, fb = moved.file(x, 48000, payload)
    _check_format(x, data, fb)


def test_misaligned_workspace_is_refused(gpu):
    """the workspace starts with the frames' int64 offsets: workspace + 4 is AMX_EINVAL,
    refused on the host before anything is launched"""
    x = _music(FRAMES_ABI, 2, 48000, seed=81)
    raw = _Raw(FRAMES_ABI, 2, BLOCK_ABI)
    rc, payload = raw.encode(x, 48000, ws_shift=4)
    assert rc == raw.capi.AMX_EINVAL and payload is None
    raw.untouched_beyond(0)
    assert int(raw.total.item()) == SENTINEL and bool((raw.fb == SENTINEL).all()) and bool((raw.sb == SENTINEL).all())
    assert bool((raw.ws == SENTINEL).all())
    rc, payload = raw.encode(x, 48000)
    assert rc == raw.capi.AMX_OK
    _check_format(x, *raw.file(x, 48000, payload))
