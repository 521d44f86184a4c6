"""master_files' host side (amx/files.py): the grouping, the header readers, the checks
that raise from the call itself, errors that stay with their job, the worker cap and the
staging bound.  No GPU."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from amx import aiffio, files, wavio
from amx.files import Header, plan_groups

DSP = dict(bass_boost=1.0, lufs=-14.0)


def _h(fs=48000, ch=2, code="s16", frames=48000):
    return Header(fs, ch, code, frames)


def test_group_key():
    """equal DSP settings, rate and chain input: one group whatever the delivery keys say"""
    heads = [_h(code="s16"), _h(code="s16"), _h(code="s24")]
    jobs = [dict(DSP, input_file="a.wav", output_file="a_out.wav"),
            dict(DSP, input_file="b.wav", output_file="b_out.flac", output_rate=44100, flac_lpc_order=4),
            dict(DSP, input_file="c.wav", output_file="c_out.FLAC", output_rate="input", create_mp3=True,
                 flac_decode="device", art_prompt="x", auto_generate_prompt=True)]
    assert plan_groups(heads, jobs) == [[0, 1, 2]]
    # a changed mid_cut: two groups
    jobs2 = [jobs[0], dict(jobs[1], mid_cut=1.0), jobs[2]]
    assert plan_groups(heads, jobs2) == [[0, 2], [1]]
    # lufs is a DSP key too
    assert plan_groups(heads, [jobs[0], dict(jobs[1], lufs=None), jobs[2]]) == [[0, 2], [1]]
    # f32 and s16: two
    assert plan_groups([_h(code="f32"), _h(code="s16")], jobs[:2]) == [[0], [1]]
    # f32 mono and f32 stereo: two; mono s16 joins stereo s16 (amx_pcm_to_s16 duplicates it)
    assert plan_groups([_h(code="f32", ch=1), _h(code="f32")], jobs[:2]) == [[0], [1]]
    assert plan_groups([_h(code="s16", ch=1), _h(code="s16")], jobs[:2]) == [[0, 1]]
    # big-endian float is converted like an integer format
    assert plan_groups([_h(code="f32be"), _h(code="s16")], jobs[:2]) == [[0, 1]]
    # 44.1 and 48 kHz: two
    assert plan_groups([_h(fs=44100), _h(fs=48000)], jobs[:2]) == [[0], [1]]
    # six channels: a group of its own, also next to another six-channel file
    assert plan_groups([_h(), _h(ch=6), _h(ch=6), _h()], [jobs[0]] * 4) == [[0, 3], [1], [2]]
    # an int where the other job has the float: the same setting
    assert plan_groups(heads[:2], [dict(jobs[0], mid_cut=2), dict(jobs[1], mid_cut=2.0)]) == [[0, 1]]
    # tables given as arrays cannot be compared: alone
    tab = [np.zeros(32769)] * 3
    assert plan_groups(heads[:2], [dict(jobs[0], _comp_m_table=tab), dict(jobs[1], _comp_m_table=tab)]) == [[0], [1]]
    # an empty file and a job without a header
    assert plan_groups([_h(), _h(frames=0), None, _h()], [jobs[0]] * 4) == [[0, 3], [1]]


def test_group_order_and_split():
    """job order inside groups, groups by their first job, the max_group_frames split"""
    a, b = dict(DSP), dict(DSP, mid_cut=3.0)
    heads = [_h(frames=100)] * 6
    jobs = [a, b, a, b, a, a]
    assert plan_groups(heads, jobs) == [[0, 2, 4, 5], [1, 3]]
    assert plan_groups(heads, jobs, 250) == [[0, 2], [1, 3], [4, 5]]
    assert plan_groups(heads, jobs, 200) == [[0, 2], [1, 3], [4, 5]]
    assert plan_groups(heads, jobs, 199) == [[0], [1], [2], [3], [4], [5]]
    # a file over the bound still gets its group
    assert plan_groups([_h(frames=1000), _h(frames=10), _h(frames=10)], [a, a, a], 50) == [[0], [1, 2]]


def test_group_2_31_bound():
    """a plan holds fewer than 2^31 frames whatever max_group_frames says"""
    n = 1 << 30
    heads = [_h(frames=n), _h(frames=n - 1), _h(frames=1), _h(frames=5)]
    jobs = [dict(DSP)] * 4
    assert plan_groups(heads, jobs) == [[0, 1], [2, 3]]             # 2^31 - 1 fits, 2^31 does not
    assert plan_groups(heads, jobs, 1 << 40) == [[0, 1], [2, 3]]
    assert files.default_group_frames(1 << 62) == (1 << 31) - 1
    assert files.default_group_frames(1 << 30) == (1 << 29) // files.DEVICE_BYTES_PER_FRAME


def test_jobs_argument():
    from audio_mastering_engine import master_files
    for bad in (None, {}, ({"input_file": "a"},), [{"input_file": "a"}, "b"]):
        with pytest.raises(TypeError):
            master_files(bad)
    assert master_files([]) == []


def test_duplicate_output(tmp_path):
    from audio_mastering_engine import master_files
    out = str(tmp_path / "m.wav")
    jobs = [dict(input_file="a.wav", output_file=str(tmp_path / "other.wav")),
            dict(input_file="b.wav", output_file=out),
            dict(input_file="c.wav"),
            dict(input_file="d.wav", output_file=str(tmp_path / "." / "m.wav"))]
    with pytest.raises(ValueError) as e:
        master_files(jobs)
    assert "1" in str(e.value) and "3" in str(e.value)
    assert not (tmp_path / "m.wav").exists()


def test_error_stays_with_job(tmp_path):
    """what master_audio raises before it touches a file or the GPU lands in the job's
    result, same type and same text"""
    from audio_mastering_engine import master_audio, master_files
    jobs = [dict(output_file=str(tmp_path / "a.wav"), lufs=-14.0),
            dict(input_file="x.wav"),
            dict(input_file="x.wav", output_file=str(tmp_path / "b.wav"), flac_decode="gpu?"),
            dict(input_file="x.wav", output_file=str(tmp_path / "c.wav"), output_rate=True),
            dict(input_file="x.wav", output_file=str(tmp_path / "d.wav"), multichannel_dynamic=1)]
    calls = []
    res = master_files(jobs, lambda i, m: calls.append((i, m)), lambda i, c, t: calls.append((i, c, t)))
    assert [r["index"] for r in res] == [0, 1, 2, 3, 4]
    assert calls == []                                  # master_audio raises these before its first callback
    assert len({r["group"] for r in res}) == 5
    for job, r in zip(jobs, res):
        with pytest.raises(Exception) as e:
            master_audio(job)
        assert type(r["error"]) is type(e.value) and str(r["error"]) == str(e.value)
        assert r["input_file"] == job.get("input_file") and r["output_file"] == job.get("output_file")
        assert r["sample_rate"] is None and r["mode"] is None and r["stats"] is None
    assert list(tmp_path.iterdir()) == []


def test_workers_cap():
    assert files.worker_count(None, 3) == 3
    assert files.worker_count(None, 100) == 8
    assert files.worker_count(64, 100) == 16
    assert files.worker_count(16, 1) == 16
    assert files.worker_count(0, 5) == 1
    assert files.worker_count(None, 0) == 1
    with pytest.raises(ValueError):
        files.worker_count("4", 5)
    from audio_mastering_engine import master_files
    with pytest.raises(ValueError):
        master_files([dict(input_file="a", output_file="b")], workers=2.5)


def test_staging_pool_bound():
    """a fake reader and small sizes: the pool never holds more than its capacity, a file
    larger than the pool is staged alone, and every read gets through in order"""
    cap = 1000
    sizes = [300, 300, 300, 300, 2500, 100, 900, 100, 50, 1000, 1]
    pool = files.StagingPool(cap, lambda n: np.zeros(n, np.uint8))
    seen, lock = [], threading.Lock()

    def reader(k):
        def fn(buf):
            with lock:
                seen.append((k, pool.used))
            buf[:] = k
            return k
        return fn
    with ThreadPoolExecutor(max_workers=4) as ex:
        reads = files.ReadAhead(pool, ex, [(n, reader(k)) for k, n in enumerate(sizes)])
        held = []

        def make_room():
            while held:
                reads.release(held.pop(0))
        for k in range(len(sizes)):
            assert reads.future(k, make_room).result() == k
            assert reads.leases[k].buf.size == sizes[k] and int(reads.leases[k].buf[0]) == k
            held.append(k)                               # (kept, as an upload in flight keeps it)
            assert pool.used <= max(cap, sizes[k])
        make_room()
    assert pool.used == 0
    assert sorted(k for k, _ in seen) == list(range(len(sizes)))
    for k, used in seen:
        assert used <= cap or used == sizes[k], (k, used)     # over the capacity only alone
    assert pool.peak == 2500


def test_released_staging_is_freed():
    """a released read gives its buffer back for real: nothing in ReadAhead (not the lease,
    not the finished future's result) keeps the memory until the call ends"""
    import gc
    import weakref
    bufs = []

    def alloc(n):
        b = np.zeros(n, np.uint8)
        bufs.append(weakref.ref(b))
        return b

    class Result:
        def __init__(self, raw):
            self.raw = raw                                # a view of the buffer, as Staged.raw is
    pool = files.StagingPool(128, alloc)
    with ThreadPoolExecutor(max_workers=2) as ex:
        reads = files.ReadAhead(pool, ex, [(64, lambda buf: Result(buf[:32]))] * 12)

        def no_room():
            raise AssertionError("every read was released before the next was asked for")
        for k in range(12):
            r = reads.future(k, no_room).result()
            assert r.raw.base is not None
            del r
            reads.release(k)
            gc.collect()
            # what is still alive: the reads started ahead, never more than the pool holds
            assert sum(64 for b in bufs[:k + 1] if b() is not None) == 0, k
            assert sum(64 for b in bufs if b() is not None) <= 128
        assert reads.futures == [None] * 12 and pool.used == 0
    gc.collect()
    assert all(b() is None for b in bufs)


def test_headers_match_readers(tmp_path):
    """read_header (no samples read) says what wavio / aiffio say with them"""
    rng = np.random.default_rng(1)
    cases = []
    for code, ch in (("s16", 2), ("s24", 2), ("u8", 1), ("f32", 1), ("f64", 2), ("s32", 6)):
        p = str(tmp_path / ("w_%s_%d.wav" % (code, ch)))
        x = rng.integers(-100, 100, (1001, ch))
        wavio.write_wav_pcm(p, x.astype(np.float64) / 128 if code[0] == "f" else x + (128 if code == "u8" else 0),
                            44100, code)
        cases.append(p)
    for code in ("s8", "s16be", "s24be", "f32be", "s16"):
        p = str(tmp_path / ("a_%s.aiff" % code))
        aiffio.write_aiff(p, rng.integers(-100, 100, (777, 2)), 48000, code)
        cases.append(p)
    for p in cases:
        raw, info, code = wavio.read_audio_raw(p)
        h = files.read_header(p)
        assert (h.sample_rate, h.channels, h.code, h.nbytes) == (info.sample_rate, info.channels, code, raw.size), p
        assert h.frames == raw.size // info.block_align
        buf = np.zeros(files.staging_bytes_for(h, "host"), np.uint8)
        st = files.read_staged(p, h, "host", buf)
        assert st.raw.tobytes() == raw.tobytes() and st.frames == h.frames and st.code == code
    # an odd-sized chunk before data, a truncated data chunk
    p = str(tmp_path / "odd.wav")
    wavio.write_wav_s16(p, rng.integers(-100, 100, (500, 2)), 8000)
    b = open(p, "rb").read()
    with open(p, "wb") as f:
        f.write(b[:12] + b"LIST" + (3).to_bytes(4, "little") + b"abc\0" + b[12:-7])
    raw, info, code = wavio.read_audio_raw(p)
    h = files.read_header(p)
    assert h.nbytes == raw.size and h.frames == 498
    st = files.read_staged(p, h, "host", np.zeros(h.nbytes, np.uint8))
    assert st.raw.tobytes() == raw.tobytes()


@pytest.mark.parametrize("content", [b"", b"RIFF", b"RIFF\0\0\0\0WAVEfmt \x10\0\0\0\x02\0\x02\0" + bytes(12) + b"data\0\0\0\0",
                                     b"RIFF\0\0\0\0WAVEdata\0\0\0\0", b"FORM\0\0\0\0AIFFCOMM\0\0\0\x02ab",
                                     b"RIFF\0\0\0\0WAVEfmt \x04\0\0\0abcd"])
def test_header_errors_match(tmp_path, content):
    """a file the readers refuse: read_header refuses it with the same exception"""
    p = str(tmp_path / "bad.wav")
    with open(p, "wb") as f:
        f.write(content)
    with pytest.raises(Exception) as want:
        wavio.read_audio_raw(p)
    with pytest.raises(Exception) as got:
        files.read_header(p)
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    missing = str(tmp_path / "nope.wav")
    with pytest.raises(FileNotFoundError) as want:
        wavio.read_audio_raw(missing)
    with pytest.raises(FileNotFoundError) as got:
        files.read_header(missing)
    assert str(got.value) == str(want.value)


def test_write_master_is_the_writers_file(tmp_path):
    """the WAV the write-behind stage writes from a buffer is write_wav_s16's file; a write
    that fails leaves nothing"""
    y = np.random.default_rng(2).integers(-32768, 32767, (999, 2)).astype(np.int16)
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    wavio.write_wav_s16(a, y, 22050)
    files.write_master(b, y.view(np.uint8).reshape(-1), 2, 22050)
    assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(OSError):
        files.write_master(str(tmp_path / "no_such_dir" / "c.wav"), y.view(np.uint8).reshape(-1), 2, 22050)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.wav", "b.wav"]
