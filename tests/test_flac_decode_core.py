"""The device FLAC decoder's core (csrc/amx_flacdec_core.hpp) on the CPU, before it runs on
a GPU: tests/flacdec_host_main.cpp decodes every candidate frame with the text the kernels
compile, chains and emits the frames as the kernels do, and is built with ASan + UBSan
(-fno-sanitize-recover: the first report ends the run with a failure).  It runs as a
subprocess; nothing is loaded into Python.

* equality: over the fixture matrix (flac_fixtures.matrix) its samples and block list equal
  the host decoder's (amx.flacio.decode_flac, csrc/amx_flac.cpp, which shares no decoding
  code with the core);
* robustness: single-byte corruptions, truncations, a valid header followed by random bytes
  or by runs of 0x00 / 0xFF.  Every run ends with exit status 0 (decoded), 2 (corrupt) or 3
  (left to the host path) within its time limit, never with a sanitizer report; where the
  host decoder accepts a mutated stream the outputs are equal, unless the core refused a
  frame for a width rule (include/amx.h: stricter than the host on invalid streams).
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import flac_fixtures

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "audio-mastering-engine_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
TIMEOUT = 10

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert os.path.exists(os.path.join(CSRC, "amx_flacdec_core.hpp"))
    out = str(tmp_path_factory.mktemp("flacdec") / "flacdec_host_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-pthread", os.path.join(HERE, "flacdec_host_main.cpp"),
                        os.path.join(CSRC, "amx_flac.cpp"), "-o", out], capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for the host compiler: %s" % r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def streams():
    return flac_fixtures.matrix()


def _run(args, allowed=(0,)):
    r = subprocess.run(args, capture_output=True, text=True, env=ENV, timeout=TIMEOUT)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert r.returncode in allowed, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return r


def _strip_id3(data):
    from amx import flacio
    return data[flacio._skip_id3(data[:10]):]


def test_core_equals_host_decoder(exe, streams, tmp_path):
    from amx import flacio
    d = str(tmp_path)
    for name, data in streams:
        want, info, blocks = flacio.decode_flac(data, with_blocks=True)
        src, pcm, blk = (os.path.join(d, name + e) for e in (".flac", ".i32", ".blocks"))
        with open(src, "wb") as f:
            f.write(_strip_id3(data))
        _run([exe, "decode", src, pcm, blk])
        got = np.fromfile(pcm, np.int32).reshape(-1, info.channels)
        assert got.tobytes() == want.tobytes(), name
        assert np.fromfile(blk, np.int32).tolist() == blocks.tolist(), name


def test_core_flips_and_cuts(exe, streams, tmp_path):
    """200 single-byte corruptions and 50 truncations of each of 20 streams, decoded by the
    core and by the host decoder inside the sanitized program, which compares them"""
    d = str(tmp_path)
    pick = [s for s in streams if len(s[1]) < 40000 and s[0] != "id3"]
    pick = pick[::max(1, len(pick) // 20)][:20]
    assert len(pick) >= 18
    equal = 0
    for i, (name, data) in enumerate(pick):
        src = os.path.join(d, name + ".flac")
        with open(src, "wb") as f:
            f.write(data)
        r = _run([exe, "fuzz", src, str(1000 + i), "200", "50"])
        assert r.stdout.startswith("250 cases:"), r.stdout
        equal += int(r.stdout.split(" equal")[0].split()[-1])
    assert equal > 0        # (a flip in the padding or the MD5 leaves a stream both decode)


def _first_header(data):
    """(offset of the first frame, length of its header with the CRC-8) from the host scan"""
    from amx import capi, flacio
    rc, sc, tab = flacio.flac_scan(data)
    assert rc == capi.AMX_OK
    c = ctypes.cast(tab.ctypes.data, ctypes.POINTER(capi.FlacCand))[0]
    return int(c.offset), int(c.data_byte)


def test_core_garbage_payloads(exe, streams, tmp_path):
    """a valid stream head and first frame header, then seeded random bytes, zeros or ones:
    unary runs and escape partitions of every length end at the read bound"""
    from amx import capi, flacio
    d = str(tmp_path)
    rng = np.random.default_rng(77)
    k = 0
    for name, data in streams[::6]:
        data = _strip_id3(data)
        off, hb = _first_header(data)
        head = data[:off + hb]
        n = max(64, len(data) - len(head))
        for fill in ("random", "random", "zeros", "ones", "short"):
            if fill == "random":
                body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            elif fill == "short":
                body = rng.integers(0, 256, int(rng.integers(0, 8)), dtype=np.uint8).tobytes()
            else:
                body = bytes([0x00 if fill == "zeros" else 0xFF]) * n
            src = os.path.join(d, "g%03d.flac" % k)
            k += 1
            with open(src, "wb") as f:
                f.write(head + body)
            r = _run([exe, "decode", src, src + ".i32", src + ".blocks"], allowed=(0, 2, 3))
            try:
                want = flacio.decode_flac(head + body)[0]
            except capi.AmxError:
                want = None
            if r.returncode == 0:
                assert want is not None
                assert np.fromfile(src + ".i32", np.int32).tobytes() == want.tobytes()
    assert k >= 40
