"""The FLAC streams the device decoder's tests share (test infrastructure): the matrix of
test_flac_decode_core.py (the decoder's core on the CPU) and test_gpu_flac_decode.py (the
kernels), written by the test-side encoder flac_enc.py, seeded."""
import numpy as np

import flac_enc

KINDS = ["constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4", "lpc"]


def signal(n, ch, bps, seed, kind="music"):
    rng = np.random.default_rng(seed)
    hi = (1 << (bps - 1)) - 1
    if kind == "noise":
        return rng.integers(-hi - 1, hi + 1, size=(n, ch), dtype=np.int64)
    t = np.arange(n) / 48000.0
    x = np.zeros((n, ch))
    for c in range(ch):
        f = 220.0 * (1 + c) * rng.uniform(0.9, 1.1)
        x[:, c] = 0.6 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 3.1 * f * t)
        x[:, c] += 0.05 * rng.standard_normal(n)
    x[n // 3: n // 3 + 600] = 0.0                         # a silent stretch (constant subframes)
    return np.clip(np.round(x * hi), -hi - 1, hi).astype(np.int64)


def false_sync_stream():
    """(bytes, frames): 24-bit stereo noise in verbatim subframes whose payload spells whole
    frame headers (sync code FF F8, valid fields, matching CRC-8): false frame starts the
    scan must list and the chain must pass over"""
    x = signal(6000, 2, 24, seed=31, kind="noise")
    x[:, 0] |= 1                                          # no wasted bits: the samples stay byte-aligned
    head = bytes([0xFF, 0xF8, 0x10, 0x10, 0x00])          # block 192, 2 independent channels, frame 0
    head += bytes([flac_enc.crc8(head)])
    a, b = int.from_bytes(head[:3], "big"), int.from_bytes(head[3:], "big")
    for at in (100, 1500, 2900, 4400, 5800):
        x[at, 0] = a - (1 << 24) if a >= 1 << 23 else a
        x[at + 1, 0] = b - (1 << 24) if b >= 1 << 23 else b
    return flac_enc.encode(x, 48000, 24, seed=4, kinds=["verbatim"], assigns=[0], block=1024), (6000 + 1023) // 1024


def matrix():
    """[(name, FLAC bytes)]: every stream is valid and decodes on the host"""
    out = []

    def add(name, x, bps, **kw):
        out.append((name, flac_enc.encode(x, kw.pop("fs", 48000), bps, **kw)))

    for bps in (8, 12, 16, 20, 24):
        for ch in (1, 2):
            add("depth%d_ch%d" % (bps, ch), signal(2000 + 37 * bps, ch, bps, seed=bps * 10 + ch), bps,
                seed=bps + ch, block=512)
    for ki, kind in enumerate(KINDS):
        for assign in (0, 8, 9, 10):
            for block in (192, 576):
                add("%s_a%d_b%d" % (kind, assign, block), signal(2000 + block, 2, 16, seed=assign * 7 + ki), 16,
                    seed=assign + block, kinds=[kind], assigns=[assign], block=block)
    add("block16x200", signal(3200, 2, 16, seed=1), 16, seed=1, block=16)
    add("block17", signal(17 * 130 + 5, 2, 16, seed=2), 16, seed=2, block=17)
    for tail in (1, 7, 15):
        add("tail%d" % tail, signal(192 * 11 + tail, 2, 16, seed=tail), 16, seed=tail, block=192)
    add("variable", signal(20000, 2, 16, seed=3), 16, seed=3, block=1024, variable=True)
    add("variable24", signal(9000, 2, 24, seed=4), 24, seed=4, block=700, variable=True)
    for ch in (3, 6, 8):
        add("ch%d" % ch, signal(3000, ch, 16, seed=ch), 16, seed=ch, block=1152)
    add("mono65535", signal(65535, 1, 16, seed=5), 16, seed=5, block=65535)
    out.append(("false_syncs", false_sync_stream()[0]))
    id3 = b"ID3\x04\x00\x00" + bytes([0, 0, 0, 20]) + bytes(20)
    out.append(("id3", id3 + flac_enc.encode(signal(5000, 2, 16, seed=6), 44100, 16, seed=6)))
    return out
