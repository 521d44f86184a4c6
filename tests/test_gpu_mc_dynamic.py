"""loudnorm's dynamic mode on 3..8-channel tracks (the settings key multichannel_dynamic):
k_ln_dyn<C> through amx_mc_loudnorm_192k, MultiChannelJob.dynamic and the drop-in,
against the oracle's restatement of af_loudnorm for any channel count (oracle/amx_oracle.c
orc_loudnorm; parity unpinned: no ffmpeg here).

The comparison is tests/test_gpu_dynamic.py's for this filter: max |diff| <= 3 LSB and at
least 99.9 % of the samples exact (the GPU statistics come from the 192 kHz hop energies,
rounding-level differences from libebur128's sequential sums).  Every case prints its
measured figures; DESIGN.md §3.9 carries them.  Signals are test_gpu_dynamic's
_dynamic_signal for C channels: synth.mix_like * 0.12 with 50-sample full-scale bursts."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGET = -14.0


@pytest.fixture(autouse=True)
def _no_garbage_with_plans():
    """a job dropped inside a reference cycle (a report that names its job, the traceback
    of an expected exception) frees its plans whenever the collector next runs; do that
    here, not in the middle of a later test's stream capture"""
    yield
    import gc
    gc.collect()


def _cmp(y, ref, what, tol=3, exact_min=0.999):
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    d = np.abs(y.astype(np.int32) - ref.astype(np.int32))
    exact = float((d == 0).mean()) if d.size else 1.0
    print("%s: max |diff| %d LSB, exact fraction %.7f" % (what, d.max() if d.size else 0, exact))
    assert (d.max() if d.size else 0) <= tol and exact >= exact_min, (what, int(d.max()), exact)


def _base(seconds, fs, C, seed):
    from amx import synth
    n = int(fs * seconds)
    return synth.mix_like(n, fs, C, seed=seed) * 0.12, np.random.default_rng(seed)


def _finish(x, fs, intro=0.0):
    if intro:
        x[:int(fs * intro)] = 0.0
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def mc_signal(seconds, fs, C, seed, intro=0.0):
    """_dynamic_signal for C channels: sparse bursts at random places, in all channels"""
    x, rng = _base(seconds, fs, C, seed)
    for k in rng.integers(0, x.shape[0] - 200, max(2, int(seconds * 2))):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, C))
    return _finish(x, fs, intro)


def single_channel_signal(seconds, fs, C, seed, channels):
    """a burst every 1.7 s from 0.4 s on, each in ONE channel, cycling through `channels`"""
    x, rng = _base(seconds, fs, C, seed)
    t, i = 0.4, 0
    while t < seconds - 0.1:
        k = int(t * fs)
        x[k:k + 50, channels[i % len(channels)]] += rng.uniform(-0.9, 0.9, 50)
        t += 1.7
        i += 1
    return _finish(x, fs)


def dense_signal(seconds, fs, C, seed):
    """bursts in all channels every 0.5 s: sustain, re-attack, the attack_length clamp"""
    x, rng = _base(seconds, fs, C, seed)
    for k in range(int(0.25 * fs), x.shape[0] - 200, fs // 2):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, C))
    return _finish(x, fs)


def edge_signal(seconds, fs, C, seed, where):
    """mc_signal plus one burst in the first 1 ms ("start": FIRST's max > ceiling branch)
    or 50 ms before the end ("end": the limiter active where FINAL re-bases the ring)"""
    x, rng = _base(seconds, fs, C, seed)
    for k in rng.integers(fs // 2, x.shape[0] - fs // 2, max(2, int(seconds * 2))):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, C))
    k = 0 if where == "start" else x.shape[0] - int(0.05 * fs)
    m = int(0.001 * fs) if where == "start" else 50
    x[k:k + m] += rng.uniform(-0.9, 0.9, (m, C))
    return _finish(x, fs)


class _Filter:
    """a MultiChannelJob whose concat buffer is the track itself (no chain), measured: what
    amx_mc_loudnorm_192k reads.  run(desc) -> the filter's int16 [n192, C]"""

    def __init__(self, oracle_mod, x, fs):
        import torch
        from amx.engine import MultiChannelJob
        self.x16 = oracle_mod.quantize(x)
        n, self.C = self.x16.shape
        self.fs = fs
        self.job = MultiChannelJob(fs, self.C, {"lufs": TARGET}, n, input_s16=True, chunks=[(0, 0, n)])
        self.job.out[:n].copy_(torch.from_numpy(self.x16))
        self.job.measure(lufs_on=True)
        self.stats = self.job.fetch_report(raise_dynamic=False)["stats"][0]

    def run(self, measured, offset, reuse=False):
        from amx import capi
        d = capi.LoudnormDesc(TARGET, 11.0, -1.5, 0.0, 0.0, 99.0, -70.0, offset)
        if measured:
            d.measured_i, d.measured_lra = float(measured["input_i"]), float(measured["input_lra"])
            d.measured_tp, d.measured_thresh = float(measured["input_tp"]), float(measured["input_thresh"])
        d.reuse_stream = 1 if reuse else 0
        self.job.dyn_filter(d)
        s = self.job._side192()
        return s.y192[:s.n192].cpu().numpy()

    def close(self):
        self.job.close()


def _both_passes(oracle_mod, x, fs, what, summary=None):
    """pass 1 (the measured_* defaults, offset 0) and pass 2 (the pass-1 strings, offset
    2.37, on pass 1's 192 kHz stream) against orc_loudnorm; returns pass 2's reference"""
    f = _Filter(oracle_mod, x, fs)
    try:
        st = oracle_mod.loudnorm_measure(f.x16, fs)
        assert f.stats == st, (f.stats, st)
        ref = None
        for measured, offset in ((None, 0.0), (st, 2.37)):
            y = f.run(measured, offset, reuse=measured is not None)
            ref, info = oracle_mod.loudnorm(f.x16, fs, TARGET, measured=measured, offset=offset)
            _cmp(y, ref, "%s %s" % (what, "pass 2" if measured else "pass 1"))
            if summary is not None:
                summary.append((info, f.job._side192().summ.cpu().numpy()))
        return ref, f.x16, st
    finally:
        f.close()


def _limited_frames(oracle_mod, ref, x16, fs, st):
    """on the oracle's output alone: the 100 ms frames its limiter changed, and left alone,
    in pass 2 -- against a run whose ceiling (target_tp 40 dB) nothing reaches"""
    free, _ = oracle_mod.loudnorm(x16, fs, TARGET, target_tp=40.0, measured=st, offset=2.37)
    nf = ref.shape[0] // 19200
    changed = (ref[:nf * 19200] != free[:nf * 19200]).reshape(nf, -1).any(axis=1)
    return int(changed.sum()), int((~changed).sum())


# ------------------------------------------------------------------ 1: the filter alone
@pytest.mark.parametrize("C,seconds,fs", [(3, 7.3, 48000), (5, 6.0, 44100), (6, 6.0, 48000), (8, 5.0, 96000),
                                          (4, 3.05, 48000)])
def test_filter_vs_oracle(gpu, oracle_mod, C, seconds, fs):
    """odd C and a partial last INNER frame; the polyphase upsampler (44.1 kHz); 6 and 8
    channels (unused channels in the loudness, 96 kHz); 3.05 s: one partial INNER frame,
    then FINAL"""
    _both_passes(oracle_mod, mc_signal(seconds, fs, C, 20 + C), fs, "mc filter C=%d %.2f s %d Hz" % (C, seconds, fs))


# ------------------------------------------------------------------ 2: single-channel peaks
@pytest.mark.parametrize("C,channels", [(3, [2, 0]), (6, [3, 5, 0]), (8, [7, 2, 6])])
def test_single_channel_peaks(gpu, oracle_mod, C, channels):
    """peaks in one channel at a time -- the last channel of an odd C (its pair partner is
    the measure plan's dummy), the LFE of 5.1 (weight 0 in the loudness, still limited),
    channel 7 of 8: the limiter's one gain per frame must follow the loudest channel.  The
    oracle's own output shows the limiter alternating between idle and engaged."""
    fs, seconds = 48000, 10.0
    x = single_channel_signal(seconds, fs, C, 60 + C, channels)
    ref, x16, st = _both_passes(oracle_mod, x, fs, "mc single-channel peaks C=%d" % C)
    limited, idle = _limited_frames(oracle_mod, ref, x16, fs, st)
    print("C=%d: %d frames limited, %d idle" % (C, limited, idle))
    assert limited >= 10 and idle >= 40, (limited, idle)


# ------------------------------------------------------------------ 3-5: limiter edges
def test_dense_bursts(gpu, oracle_mod):
    """bursts in all channels every 0.5 s keep the limiter busy: sustain, re-attack with
    attack_length = peak_delta, the <= 1 -> 2 clamp (the oracle's limiter changes at least
    every fourth frame)"""
    fs = 48000
    ref, x16, st = _both_passes(oracle_mod, dense_signal(6.0, fs, 4, 71), fs, "mc dense bursts C=4")
    limited, idle = _limited_frames(oracle_mod, ref, x16, fs, st)
    print("dense bursts: %d frames limited, %d idle" % (limited, idle))
    assert limited >= 15, (limited, idle)


@pytest.mark.parametrize("C,where", [(3, "start"), (6, "start"), (5, "end"), (8, "end")])
def test_burst_at_the_edges(gpu, oracle_mod, C, where):
    _both_passes(oracle_mod, edge_signal(5.0, 48000, C, 80 + C, where), 48000, "mc burst at the %s C=%d" % (where, C))


# ------------------------------------------------------------------ 6-7: quiet start, < 3 s
def test_quiet_start(gpu, oracle_mod):
    """a 4 s silent intro: above_threshold starts at 0, so r128_out -- the K filter per
    channel with libebur128's weights -- and the x 1.0058 growth steer the first frames"""
    summ = []
    _both_passes(oracle_mod, mc_signal(9.0, 48000, 6, 91, intro=4.0), 48000, "mc quiet start C=6", summ)
    assert all(s[1][7] > 0 for s in summ), "r128_out must have run (above_threshold 0)"


def test_under_3s_linear_fallback(gpu, oracle_mod):
    summ = []
    _both_passes(oracle_mod, mc_signal(2.0, 48000, 3, 93), 48000, "mc < 3 s C=3", summ)
    for info, s in summ:
        assert info["normalization_type"] == "linear" and s[0] == 1.0


# ------------------------------------------------------------------ 8: channel-count identity
def test_identity_with_stereo(gpu, oracle_mod):
    """a 4-channel track whose channels 2-3 are zero, fed the STEREO measurement's hop and
    peak arrays: channels 0-1 are amx_loudnorm_192k's output on the stereo track (within
    _cmp's limits; printed: whether bit-exact), channels 2-3 exactly 0"""
    import torch
    from amx import capi
    from amx.engine import MasteringJob
    fs = 48000
    x2 = mc_signal(7.3, fs, 2, 5)
    x16 = oracle_mod.quantize(x2)
    n = x16.shape[0]
    st = oracle_mod.loudnorm_measure(x16, fs)
    job = MasteringJob(fs, 2, {"lufs": TARGET}, [n], input_s16=True, chunks=[(0, 0, n)], measure_only=True)
    job.out[:n].copy_(torch.from_numpy(x16))
    job.loudness_pass1(tail=False)
    job.loudness_pass2(carry=False)
    job.histograms()
    job.decide()
    n192, job2, ws2, summ = job._job192(0)
    x4 = np.concatenate([x2, np.zeros_like(x2)], axis=1)
    f = _Filter(oracle_mod, x4, fs)
    try:
        s = f.job._side192()
        assert s.n192 == n192
        for measured, offset in ((None, 0.0), (st, 2.37)):
            d = capi.LoudnormDesc(TARGET, 11.0, -1.5, 0.0, 0.0, 99.0, -70.0, offset)
            if measured:
                d.measured_i, d.measured_lra = float(st["input_i"]), float(st["input_lra"])
                d.measured_tp, d.measured_thresh = float(st["input_tp"]), float(st["input_thresh"])
            job.loudnorm_192k(0, d, job2, ws2, summ)
            want = job2.out[:n192].cpu().numpy()
            capi.check(capi.load().amx_mc_loudnorm_192k(
                f.job.meas.plan.h, 4, ctypes.byref(d), capi.ptr(f.job.meas.out), capi.ptr(job.hops),
                int(job.max_hops), capi.ptr(job.peak), capi.ptr(s.y192), capi.ptr(s.summ), capi.ptr(s.ws),
                capi.ptr_stream()), "amx_mc_loudnorm_192k")
            y = s.y192[:n192].cpu().numpy()
            assert not y[:, 2:].any()
            what = "mc identity %s" % ("pass 2" if measured else "pass 1")
            print("%s: bit-exact with the stereo filter: %s" % (what, bool((y[:, :2] == want).all())))
            _cmp(y[:, :2], want, what)
    finally:
        f.close()
        job.close()


# ------------------------------------------------------------------ 9: the whole pipeline
_pipe = {}


def _pipeline_case(oracle_mod, C):
    """(x float32, x16, oracle's master at 192 kHz, info), once per C"""
    if C not in _pipe:
        from amx.chunking import chunk_bounds
        fs = 48000
        x = mc_signal(11.0, fs, C, 40 + C)
        x16 = oracle_mod.quantize(x)
        settings = dict(bass_boost=1.0, lufs=TARGET)
        ref, info = oracle_mod.pipeline(x16, fs, settings, chunk_bounds(x.shape[0], fs, 512))
        assert info["mode"] == "dynamic" and info["sample_rate"] == 192000, info.get("stats")
        assert (ref != info["normalized"]).any(), "the C-channel alimiter must engage"
        ref.setflags(write=False)
        _pipe[C] = (x, x16, settings, ref, info)
    return _pipe[C]


@pytest.mark.parametrize("C", [3, 6])
def test_master_array_dynamic(gpu, oracle_mod, C):
    import torch
    from amx.engine import master_array
    x, x16, settings, ref, info = _pipeline_case(oracle_mod, C)
    y, rep = master_array(torch.from_numpy(x), 48000, dict(settings, multichannel_dynamic=True), quantum=512)
    assert rep["modes"] == ["dynamic"] and rep["sample_rate"] == 192000
    assert rep["stats"][0] == info["stats"], (rep["stats"][0], info["stats"])
    assert rep["dynamic"]["target_offset"] == info["pass1"]["target_offset"]
    _cmp(y.cpu().numpy(), ref, "mc master_array dynamic C=%d" % C)
    rep["job"].close()


def _want_rate(oracle_mod, x16, fi, fo):
    """the oracle's resampling through ffmpeg's f32 -> s16 conversion (test_gpu_resample's)"""
    u = oracle_mod.upsample(x16, fi, fo).astype(np.float32) * np.float32(32768)
    return np.clip(np.rint(u), -32768, 32767).astype(np.int16)


def test_master_audio_dynamic_files(gpu, oracle_mod, tmp_path):
    """master_audio on a 6-channel WAV with the key: a 192 kHz .wav, and a .flac at
    output_rate 48000 -- the status / progress sequence of the linear multichannel test,
    the file's rate, frame count and samples against the oracle's master (delivered by the
    oracle's resampler)"""
    import audio_mastering_engine as ame
    from amx import flacio, wavio
    from amx.chunking import chunk_bounds, packet_frames
    fs, C = 48000, 6
    x, _, settings, _, _ = _pipeline_case(oracle_mod, C)
    src, wav, flac = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "out.flac")
    wavio.write_wav_pcm(src, x, fs, "f32")
    raw, winfo, _ = wavio.read_wav_raw(src)
    x16 = wavio.to_s16(wavio.read_wav_native(src)[0], winfo)
    bounds = chunk_bounds(x.shape[0], fs, packet_frames(winfo.block_align))
    ref, info = oracle_mod.pipeline(x16, fs, settings, bounds)
    assert info["mode"] == "dynamic"
    nb = len(bounds)
    for dst, extra in ((wav, {}), (flac, {"output_rate": 48000})):
        st, pr = [], []
        out = ame.master_audio(dict(settings, multichannel_dynamic=True, input_file=src, output_file=dst, **extra),
                               st.append, lambda a, b: pr.append((a, b)))
        assert out == dst
        assert st[:2] == ["Splitting audio into manageable chunks...", "Splitting complete."]
        assert "Normalizing final loudness..." in st and st[-1] == "Applying final limiting and exporting..."
        assert pr[0] == (0, 100) and pr[-1] == (nb + 4, nb + 4)
        assert [p for p in pr[1:]] == [(i + 1, nb + 4) for i in range(nb)] + [(nb + k, nb + 4) for k in (1, 2, 3, 4)]
    y, winfo2 = wavio.read_wav_native(wav)
    assert winfo2.sample_rate == 192000 and winfo2.channels == C and winfo2.bits == 16
    _cmp(y.reshape(-1, C), ref, "mc master_audio dynamic .wav")
    got, finfo = flacio.decode_flac(open(flac, "rb").read())
    want = _want_rate(oracle_mod, ref, 192000, 48000)
    assert finfo.sample_rate == 48000 and finfo.channels == C and finfo.total_frames == want.shape[0]
    assert want.shape[0] == -(-ref.shape[0] // 4)
    _cmp((got.reshape(want.shape) >> 16).astype(np.int16), want, "mc master_audio dynamic .flac at 48 kHz")


# ------------------------------------------------------------------ 10: the key absent
def test_key_absent_still_refuses(gpu):
    """the exact call of test_gpu_multichannel.test_multichannel_refuses_dynamic_mode; the
    key False likewise"""
    import torch
    from amx import synth
    from amx.engine import DynamicModeUnsupported, master_array
    fs = 48000
    n = fs * 12
    x = synth.mix_like(n, fs, 3, seed=5) * np.float32(0.12)
    rng = np.random.default_rng(5)
    for k in rng.integers(0, n - 200, 24):
        x[k:k + 50] += rng.uniform(-0.9, 0.9, (50, 3)).astype(np.float32)
    x = np.clip(x, -1.0, 1.0).astype(np.float32)
    with pytest.raises(DynamicModeUnsupported):
        master_array(torch.from_numpy(x), fs, dict(lufs=-14.0), quantum=512)
    with pytest.raises(DynamicModeUnsupported):
        master_array(torch.from_numpy(x), fs, dict(lufs=-14.0, multichannel_dynamic=False), quantum=512)


def test_linear_track_same_bytes_with_key(gpu):
    import torch
    from amx import synth
    from amx.engine import master_array
    fs = 48000
    x = synth.mix_like(fs * 6, fs, 5, seed=17)
    outs = []
    for extra in ({}, {"multichannel_dynamic": True}):
        y, rep = master_array(torch.from_numpy(x), fs, dict(bass_boost=1.0, lufs=-16.0, **extra), quantum=512)
        assert rep["modes"] == ["linear"] and rep["sample_rate"] == fs
        outs.append(y.cpu().numpy().tobytes())
        rep["job"].close()
    assert outs[0] == outs[1]


# ------------------------------------------------------------------ 11: the fallback
def test_loudness_error_falls_back(gpu, oracle_mod, tmp_path, monkeypatch):
    """:243-246 -- an error in the loudness stage is logged, and the track finalised without
    the gain: the oracle's pipeline with lufs removed"""
    import audio_mastering_engine as ame
    from amx import engine, wavio
    from amx.chunking import chunk_bounds, packet_frames
    fs, C = 48000, 3
    x = mc_signal(5.0, fs, C, 43)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    wavio.write_wav_pcm(src, x, fs, "f32")
    calls = []

    def boom(self, stats, stream=None):
        calls.append(stats)
        raise RuntimeError("the loudness stage fails")
    monkeypatch.setattr(engine.MultiChannelJob, "dynamic", boom)
    settings = dict(bass_boost=1.0, lufs=TARGET)
    assert ame.master_audio(dict(settings, multichannel_dynamic=True, input_file=src, output_file=dst)) == dst
    assert len(calls) == 1, "the track must have taken dynamic mode"
    y, info = wavio.read_wav_native(dst)
    raw, winfo, _ = wavio.read_wav_raw(src)
    x16 = wavio.to_s16(wavio.read_wav_native(src)[0], winfo)
    ref, _ = oracle_mod.pipeline(x16, fs, dict(settings, lufs=None),
                                 chunk_bounds(x.shape[0], fs, packet_frames(winfo.block_align)))
    assert info.sample_rate == fs and info.channels == C
    _cmp(y.reshape(-1, C), ref, "mc fallback without the gain", tol=3, exact_min=0.9999)


# ------------------------------------------------------------------ 12: ABI refusals
def test_abi_refusals(gpu, oracle_mod):
    """every bad argument is AMX_EINVAL before any launch: the output buffer, pre-filled
    with a pattern, is untouched"""
    import torch
    from amx import capi
    L = capi.load()
    fs, C = 48000, 3
    f = _Filter(oracle_mod, mc_signal(0.5, fs, C, 3), fs)
    try:
        job = f.job
        s = job._side192()
        d = capi.LoudnormDesc(TARGET, 11.0, -1.5, 0.0, 0.0, 99.0, -70.0, 0.0)
        s.y192.fill_(0x5A5A)
        good = dict(plan=job.meas.plan.h, channels=C, desc=ctypes.byref(d), pairs=capi.ptr(job.meas.out),
                    hops=capi.ptr(job.one.hops), max_hops=int(job.one.max_hops), peak=capi.ptr(job.one.peak),
                    y=capi.ptr(s.y192), summ=capi.ptr(s.summ), ws=capi.ptr(s.ws))

        def call(**bad):
            a = dict(good, **bad)
            return L.amx_mc_loudnorm_192k(a["plan"], a["channels"], a["desc"], a["pairs"], a["hops"], a["max_hops"],
                                          a["peak"], a["y"], a["summ"], a["ws"], capi.ptr_stream())
        cases = [dict(channels=2), dict(channels=9), dict(channels=6), dict(plan=None), dict(desc=None),
                 dict(pairs=None), dict(hops=None), dict(peak=None), dict(y=None), dict(summ=None), dict(ws=None),
                 dict(max_hops=s.n192 // 19200), dict(plan=job.one.plan.h)]
        for bad in cases:
            assert call(**bad) == capi.AMX_EINVAL, bad
        n, w = ctypes.c_int64(), ctypes.c_int64()
        for ch in (2, 9, 6):
            assert L.amx_mc_loudnorm_192k_size(job.meas.plan.h, ch, ctypes.byref(n), ctypes.byref(w)) == capi.AMX_EINVAL
        assert L.amx_mc_loudnorm_192k_size(job.meas.plan.h, C, None, ctypes.byref(w)) == capi.AMX_EINVAL
        torch.cuda.synchronize()
        assert bool((s.y192 == 0x5A5A).all()), "a refused call wrote to the output"
        assert call() == capi.AMX_OK                      # and the same arguments, all good, run
        torch.cuda.synchronize()
        assert not bool((s.y192[:s.n192] == 0x5A5A).all())
    finally:
        f.close()
