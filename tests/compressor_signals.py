"""Crafted int16 inputs for the compressor tests (tests/test_gpu_compressor.py, and the
reference pin test_compressor_edges_match_pydub_restatement in tests/test_oracle.py).

Each signal puts the detector or the gain somewhere music does not: the top of the
detector's range, r = 0 stretches, energy at a chunk's first frame, a few-LSB floor, one
silent channel, bands that saturate the overlay's adds.  ``edge_signal`` builds the signal
chunk by chunk (``lengths``), since ``step`` depends on where a chunk starts.
"""
import numpy as np

SIGNALS = ("dc", "alt", "impulses", "step", "noise_lo", "am", "one_ch", "sq110+sq5k")
# no +-2 LSB noise where saturation (or exact zeros between the impulses) is the point
NOISELESS = ("alt", "impulses", "sq110+sq5k")

# (threshold dB, ratio) pairs: the GUI's corners (-40..0 dB, 1..10), thresholds above 0 dBFS
# and far below the sliders, a ratio below 1 and a negative one (both give the reference a
# negative or growing attenuation), a ratio a hair over 1 (attenuations ~1e-6..1e-2 dB), a
# threshold that is a power of two in amplitude, the default low band, a threshold one
# count under full scale
PAIRS = ((-40.0, 10.0), (-40.0, 1.0), (0.0, 10.0), (3.0, 4.0), (-60.0, 10.0), (-90.0, 10.0),
         (-20.0, 0.5), (-20.0, -2.0), (-12.34, 1.0001), (20.0 * np.log10(0.5), 2.0), (-25.0, 6.0),
         (-0.001, 10.0))


def _sq(n, fs, freq, t0=0):
    t = (np.arange(n) + t0) / float(fs)
    return np.where(np.sin(2 * np.pi * freq * t) >= 0, 1.0, -1.0)


def _one(name, n, fs, rng, index, channels):
    C = channels
    if name == "dc":
        x = np.full((n, C), -30000.0)
    elif name == "alt":
        x = np.where(np.arange(n) % 2 == 0, 32767.0, -32768.0)[:, None].repeat(C, 1)
    elif name == "impulses":
        x = np.zeros((n, C))
        x[::97] = 32767.0
    elif name == "step":
        # zero, 20000 for a third of the chunk, zero; every second chunk starts ON the step
        x = np.zeros((n, C))
        a = 0 if index % 2 else n // 3
        x[a:a + n // 3] = 20000.0 + rng.integers(-2, 3, (n // 3, C))
    elif name == "noise_lo":
        x = rng.integers(-3, 4, (n, C)).astype(np.float64)
    elif name == "am":
        x = rng.normal(0.0, 9000.0, (n, C)) * np.abs(np.sin(np.arange(n) / 150.0))[:, None]
    elif name == "one_ch":
        x = np.zeros((n, C))
        x[:, 0::2] = 32767.0
    elif name == "sq110+sq5k":
        s = 0.8 * _sq(n, fs, 110.0) + 0.6 * _sq(n, fs, 5000.0)
        x = (np.clip(s, -1.0, 1.0) * 32767.0)[:, None].repeat(C, 1)
        if C > 2:
            x = x * (1.0 - 2.0 * (np.arange(C) % 3 == 2))       # every third channel inverted
    else:
        raise KeyError(name)
    if name not in NOISELESS and name not in ("step", "noise_lo"):
        x = x + rng.integers(-2, 3, (n, C))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def edge_signal(name, lengths, fs, seed, channels=2):
    """int16 [sum(lengths), channels]: the named signal, built per chunk"""
    rng = np.random.default_rng([seed, SIGNALS.index(name), fs])
    return np.concatenate([_one(name, int(n), fs, rng, k, channels) for k, n in enumerate(lengths)])
