"""master_files on the GPU: every output file must be, byte for byte, the file
master_audio writes for the same settings dict -- through batched plans (groups), the
read-ahead and write-behind threads, errors, a split group, a failing loudness stage --
with master_audio's callbacks per job, all on the calling thread."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MB = dict(multiband=True, low_thresh=-25.0, low_ratio=6.0, mid_thresh=-20.0, mid_ratio=3.0,
          high_thresh=-15.0, high_ratio=4.0)
C3 = dict(bass_boost=-1.0, mid_cut=2.0, presence_boost=2.5, treble_boost=1.0, lufs=-14.0,
          width=1.3, analog_character=40.0, **MB)


def _dynamic_signal(seconds, fs, seed, intro=0.0):
    """quiet program with sparse full-scale transients: TP + offset > -1.5 dBTP
    (tests/test_gpu_dynamic.py's)"""
    from amx import synth
    n = int(fs * seconds)
    x = synth.mix_like(n, fs, 2, seed=seed) * 0.12
    rng = np.random.default_rng(seed)
    for k in rng.integers(0, n - 200, max(2, int(seconds * 2))):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, 2))
    if intro:
        x[:int(fs * intro)] = 0.0
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def _s16(x):
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def _s24(x):
    return np.clip(np.round(x * 8388607.0), -8388608, 8388607).astype(np.int32)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _single(jobs, ref_dir, record=None):
    """master_audio over the dicts, writing into ref_dir: ([output path or None], [error or None])"""
    import audio_mastering_engine as ame
    paths, errors = [], []
    for i, job in enumerate(jobs):
        out = os.path.join(ref_dir, os.path.basename(job["output_file"]))
        st = pr = None
        if record is not None:
            record[i] = ([], [])
            st, pr = record[i][0].append, (lambda a, b, r=record[i][1]: r.append((a, b)))
        try:
            ame.master_audio(dict(job, output_file=out), st, pr)
            paths.append(out)
            errors.append(None)
        except Exception as e:   # noqa: BLE001 -- compared with master_files' stored error
            paths.append(None)
            errors.append(e)
            assert not os.path.exists(out)
    return paths, errors


def _same_files(jobs, results, ref_paths):
    for job, r, ref in zip(jobs, results, ref_paths):
        assert r["error"] is None, (r["index"], r["error"])
        got, want = _read(job["output_file"]), _read(ref)
        assert len(got) == len(want), (r["index"], len(got), len(want))
        assert got == want, "job %d: %s differs from master_audio's file" % (r["index"], job["output_file"])


def test_mixed_list(gpu, tmp_path):
    """seven files: two batched groups (f32 stereo with a dynamic track; s16 / s24 / FLAC as
    s16 stereo), a mono 44.1 kHz file and a six-channel file on their own"""
    import audio_mastering_engine as ame
    from amx import flacio, synth, wavio
    fs = 48000
    src, out, ref = tmp_path / "in", tmp_path / "out", tmp_path / "ref"
    for d in (src, out, ref):
        d.mkdir()
    p = lambda d, name: str(d / name)   # noqa: E731
    wavio.write_wav_f32(p(src, "a.wav"), synth.mix_like(480000, fs, 2, seed=21), fs)
    wavio.write_wav_f32(p(src, "b.wav"), _dynamic_signal(9.0, fs, 22), fs)
    wavio.write_wav_pcm(p(src, "c.wav"), _s16(synth.mix_like(fs * 6, fs, 2, seed=31)), fs, "s16")
    wavio.write_wav_pcm(p(src, "d.wav"), _s24(synth.mix_like(fs * 4, fs, 2, seed=32)), fs, "s24")
    flacio.write_flac(p(src, "e.flac"), _s16(synth.mix_like(fs * 5, fs, 2, seed=33)), fs)
    wavio.write_wav_pcm(p(src, "f.wav"), _s16(synth.mix_like(44100 * 5, 44100, 1, seed=34).reshape(-1)), 44100, "s16")
    wavio.write_wav_pcm(p(src, "g.wav"), _s16(synth.mix_like(fs * 4, fs, 6, seed=35)), fs, "s16")
    ab, cde = dict(mid_cut=2.0, lufs=-16.0), dict(bass_boost=1.0, lufs=-14.0)
    jobs = [dict(ab, input_file=p(src, "a.wav"), output_file=p(out, "a.wav")),
            dict(ab, input_file=p(src, "b.wav"), output_file=p(out, "b.flac"), output_rate="input"),
            dict(cde, input_file=p(src, "c.wav"), output_file=p(out, "c.wav")),
            dict(cde, input_file=p(src, "d.wav"), output_file=p(out, "d.flac"), flac_lpc_order=4),
            dict(cde, input_file=p(src, "e.flac"), output_file=p(out, "e.wav")),
            dict(C3, input_file=p(src, "f.wav"), output_file=p(out, "f.wav")),
            dict(bass_boost=1.0, lufs=None, input_file=p(src, "g.wav"), output_file=p(out, "g.wav"))]
    ref_paths, errors = _single(jobs, str(ref))
    assert errors == [None] * 7
    res = ame.master_files(jobs)
    assert [r["index"] for r in res] == list(range(7))
    _same_files(jobs, res, ref_paths)
    a, b, c, d, e, f, g = res
    # the batched path is what ran
    assert a["group"] == b["group"] and c["group"] == d["group"] == e["group"]
    assert len({a["group"], c["group"], f["group"], g["group"]}) == 4
    assert (a["mode"], b["mode"]) == ("linear", "dynamic")
    assert b["sample_rate"] == 48000 and a["sample_rate"] == 48000
    assert f["sample_rate"] == 44100 and g["sample_rate"] == 48000 and g["mode"] == "off" and g["stats"] is None
    assert set(b["stats"]) == {"input_i", "input_tp", "input_lra", "input_thresh"}
    for r, job in zip(res, jobs):
        assert r["input_file"] == job["input_file"] and r["output_file"] == job["output_file"]


def test_callbacks(gpu, tmp_path):
    """per index master_audio's status strings and progress pairs, on the calling thread"""
    import audio_mastering_engine as ame
    from amx import synth, wavio
    (tmp_path / "ref").mkdir()
    settings = dict(bass_boost=2.0, mid_cut=1.5, lufs=-14.0)
    fs = 22050
    wavio.write_wav_pcm(str(tmp_path / "two.wav"), _s16(synth.mix_like(fs * 31, fs, 2, seed=41)), fs, "s16")
    wavio.write_wav_pcm(str(tmp_path / "one.wav"), _s16(synth.mix_like(fs * 4, fs, 2, seed=42)), fs, "s16")
    jobs = [dict(settings, input_file=str(tmp_path / "two.wav"), output_file=str(tmp_path / "two_m.wav")),
            dict(settings, input_file=str(tmp_path / "one.wav"), output_file=str(tmp_path / "one_m.wav"))]
    want = {}
    ref_paths, errors = _single(jobs, str(tmp_path / "ref"), record=want)
    assert errors == [None, None]
    got = {0: ([], []), 1: ([], [])}
    threads = set()

    def status(i, msg):
        threads.add(threading.get_ident())
        got[i][0].append(msg)

    def progress(i, cur, total):
        threads.add(threading.get_ident())
        got[i][1].append((cur, total))
    res = ame.master_files(jobs, status, progress)
    _same_files(jobs, res, ref_paths)
    assert res[0]["group"] == res[1]["group"]
    assert want[0][0][2] == "Processing chunk 1 of 2..." and (2, 6) in want[0][1]      # a two-chunk file
    for i in (0, 1):
        assert got[i][0] == want[i][0], (i, got[i][0])
        assert got[i][1] == want[i][1], (i, got[i][1])
    assert threads == {threading.get_ident()}


def test_errors_stay_with_their_job(gpu, tmp_path):
    import audio_mastering_engine as ame
    from amx import synth, wavio
    (tmp_path / "ref").mkdir()
    fs = 48000
    for name, seed, seconds in (("g1.wav", 51, 5), ("g2.wav", 52, 5), ("rate.wav", 53, 3)):
        wavio.write_wav_pcm(str(tmp_path / name), _s16(synth.mix_like(fs * seconds, fs, 2, seed=seed)), fs, "s16")
    good = _read(str(tmp_path / "g1.wav"))
    with open(tmp_path / "adpcm.wav", "wb") as f:
        f.write(good[:20] + (2).to_bytes(2, "little") + good[22:])          # format tag 2
    s = dict(bass_boost=1.0, lufs=-14.0)
    j = lambda name, **kw: dict(s, input_file=str(tmp_path / name), output_file=str(tmp_path / ("m_" + name)), **kw)  # noqa: E731
    jobs = [j("g1.wav"), j("missing.wav"), j("adpcm.wav"), j("rate.wav", output_rate=22050), j("g2.wav")]
    want = {}
    ref_paths, errors = _single(jobs, str(tmp_path / "ref"), record=want)
    assert [e is None for e in errors] == [True, False, False, False, True]
    assert "22050" in str(errors[3]) and "192000" in str(errors[3])
    got = {i: ([], []) for i in range(5)}
    res = ame.master_files(jobs, lambda i, m: got[i][0].append(m), lambda i, c, t: got[i][1].append((c, t)))
    _same_files([jobs[0], jobs[4]], [res[0], res[4]], [ref_paths[0], ref_paths[4]])
    for i in (1, 2, 3):
        assert type(res[i]["error"]) is type(errors[i]) and str(res[i]["error"]) == str(errors[i]), res[i]["error"]
        assert not os.path.exists(jobs[i]["output_file"])
        assert res[i]["sample_rate"] is None and res[i]["mode"] is None
    for i in range(5):
        assert got[i][0] == want[i][0] and got[i][1] == want[i][1], (i, got[i], want[i])
    assert res[0]["group"] == res[4]["group"] and (res[0]["mode"], res[4]["mode"]) == ("linear", "linear")


def test_split_group(gpu, tmp_path):
    """three equal-key files, a bound two fit under: groups of two and one, the same bytes.
    The files are 4 s long, not 3 s: at exactly 3 s with lufs, loudnorm takes dynamic mode on
    one whole 192 kHz frame, where master_audio's own file is not the same from one run to
    the next, so there would be nothing to compare bytes with."""
    import audio_mastering_engine as ame
    from amx import synth, wavio
    (tmp_path / "ref").mkdir()
    fs, n = 48000, 48000 * 4
    s = dict(treble_boost=1.5, lufs=-14.0)
    jobs = []
    for k in range(3):
        wavio.write_wav_pcm(str(tmp_path / ("s%d.wav" % k)), _s16(synth.mix_like(n, fs, 2, seed=60 + k)), fs, "s16")
        jobs.append(dict(s, input_file=str(tmp_path / ("s%d.wav" % k)), output_file=str(tmp_path / ("m%d.wav" % k))))
    ref_paths, errors = _single(jobs, str(tmp_path / "ref"))
    # a small staging bound as well: the reads and writes queue behind it
    res = ame.master_files(jobs, max_group_frames=2 * n + 100, staging_bytes=n * 4 + 64, workers=2)
    print("split group modes", [r["mode"] for r in res])
    _same_files(jobs, res, ref_paths)
    assert res[0]["group"] == res[1]["group"] != res[2]["group"]
    assert all(r["mode"] in ("linear", "dynamic") and r["stats"] is not None for r in res)


def test_two_dynamic_tracks_in_a_group(gpu, tmp_path):
    """two files loudnorm sends to dynamic mode and a linear one in one plan: the dynamic
    tracks are finished side by side (MasteringJob.finish_dynamic) and still are
    master_audio's files"""
    import audio_mastering_engine as ame
    from amx import synth, wavio
    (tmp_path / "ref").mkdir()
    fs = 48000
    s = dict(bass_boost=1.0, lufs=-14.0)
    xs = [_dynamic_signal(6.0, fs, 51), synth.mix_like(fs * 5, fs, 2, seed=52), _dynamic_signal(7.5, fs, 53)]
    jobs = []
    for k, x in enumerate(xs):
        wavio.write_wav_f32(str(tmp_path / ("d%d.wav" % k)), x, fs)
        jobs.append(dict(s, input_file=str(tmp_path / ("d%d.wav" % k)), output_file=str(tmp_path / ("m%d.wav" % k))))
    ref_paths, errors = _single(jobs, str(tmp_path / "ref"))
    res = ame.master_files(jobs)
    assert [r["mode"] for r in res] == ["dynamic", "linear", "dynamic"] and len({r["group"] for r in res}) == 1
    assert [r["sample_rate"] for r in res] == [192000, 48000, 192000]
    _same_files(jobs, res, ref_paths)


def test_loudness_failure_inside_a_group(gpu, tmp_path, monkeypatch):
    """MasteringJob.histograms raises: the group is re-run one file at a time, and each
    file comes out as master_audio writes it under the same patch (its :243-246 fallback)"""
    import audio_mastering_engine as ame
    from amx import synth, wavio
    from amx.engine import MasteringJob
    (tmp_path / "ref").mkdir()
    fs = 48000
    s = dict(bass_boost=1.0, lufs=-14.0)
    jobs = []
    for k in range(2):
        wavio.write_wav_pcm(str(tmp_path / ("h%d.wav" % k)), _s16(synth.mix_like(fs * 3, fs, 2, seed=70 + k)), fs, "s16")
        jobs.append(dict(s, input_file=str(tmp_path / ("h%d.wav" % k)), output_file=str(tmp_path / ("m%d.wav" % k))))
    normal, _ = _single([jobs[0]], str(tmp_path / "ref"))
    unpatched = _read(normal[0])

    def boom(self, stream=None):
        raise RuntimeError("injected histogram failure")
    monkeypatch.setattr(MasteringJob, "histograms", boom)
    want = {}
    ref_paths, errors = _single(jobs, str(tmp_path / "ref"), record=want)
    assert errors == [None, None]
    assert _read(ref_paths[0]) != unpatched            # (the patch bites: no gain was applied)
    got = {0: ([], []), 1: ([], [])}
    res = ame.master_files(jobs, lambda i, m: got[i][0].append(m), lambda i, c, t: got[i][1].append((c, t)))
    _same_files(jobs, res, ref_paths)
    assert got == want
    assert [r["mode"] for r in res] == ["off", "off"] and res[0]["group"] == res[1]["group"]


def test_edges(gpu, tmp_path):
    """no job; one job: master_audio's file and callbacks"""
    import audio_mastering_engine as ame
    from amx import files, synth, wavio
    assert ame.master_files([]) == []
    (tmp_path / "ref").mkdir()
    fs = 44100
    wavio.write_wav_f32(str(tmp_path / "x.wav"), synth.mix_like(fs * 2, fs, 1, seed=80).reshape(-1), fs)
    jobs = [dict(mid_cut=1.0, lufs=-14.0, input_file=str(tmp_path / "x.wav"), output_file=str(tmp_path / "y.flac"))]
    want = {}
    ref_paths, errors = _single(jobs, str(tmp_path / "ref"), record=want)
    got = {0: ([], [])}
    res = ame.master_files(jobs, lambda i, m: got[i][0].append(m), lambda i, c, t: got[i][1].append((c, t)))
    _same_files(jobs, res, ref_paths)
    assert got == want and len(res) == 1 and res[0]["index"] == 0
    # (under 3 s with a loudness range of 0: dynamic mode's linear fallback, a 192 kHz master)
    assert res[0]["sample_rate"] == files.read_header(ref_paths[0]).sample_rate == 192000
    assert res[0]["mode"] == "dynamic"
