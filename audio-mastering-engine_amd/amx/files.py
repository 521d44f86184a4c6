"""Many files in one call: master_files' engine.

master_audio handles one file and does everything in series: read, upload from pageable
memory, plan, kernels, download, a second host copy, MD5, write.  Here a list of jobs goes
through three stages that overlap:

    read ahead   (thread pool)     container parse, payload -> pinned staging (readinto),
                                   host FLAC decode
    device       (calling thread)  H2D on a copy stream, ONE MasteringJob per group of files
                                   that can share a plan, per-track delivery and FLAC encode,
                                   D2H into pinned staging
    write behind (thread pool)     MD5, container, file write from the pinned buffer

Every torch.cuda call, every pinned allocation and every libamx device call stays on the
calling thread (libamx's last error is thread-local and plan creation synchronises the
device); the worker threads touch files and host memory only -- the one library call they
make is the host FLAC decoder, which takes no device and releases the GIL.

The contract is master_audio's: every output file is the file master_audio writes for the
same dict, byte for byte, every job's callbacks are master_audio's sequence, and an
exception master_audio would raise is stored in that job's result.
"""
import hashlib
import logging
import os
import struct
import threading
from concurrent.futures import FIRST_COMPLETED, ThreadPoolExecutor, wait

import numpy as np

from . import aiffio, wavio
from .chunking import bounds_for, plan_tracks
from .settings import output_rate
from .wavio import WavInfo

MAX_WORKERS = 16
DEFAULT_WORKERS = 8
DEFAULT_STAGING_BYTES = 2 << 30
MAX_PLAN_FRAMES = (1 << 31) - 1          # a plan holds fewer than 2^31 frames (AMX_ERANGE)
# device bytes budgeted per frame of a group when max_group_frames is not given: the input
# (<= 8), the chain's output and the master (4 + 4), the plan's workspace, and for a track
# that takes dynamic mode four times as many 192 kHz frames with their own buffers
DEVICE_BYTES_PER_FRAME = 512
DEVICE_MEMORY_SHARE = 0.5                # of the free device memory: the stated margin

# the settings keys the chunk chain (design.chain_desc), the loudness stage and the limiter
# read, with the defaults they read them with; every other key is a delivery key
DSP_KEYS = (("analog_character", 0), ("bass_boost", 0.0), ("mid_cut", 0.0), ("presence_boost", 0.0),
            ("treble_boost", 0.0), ("width", 1.0), ("multiband", None), ("low_thresh", None),
            ("low_ratio", None), ("mid_thresh", None), ("mid_ratio", None), ("high_thresh", None),
            ("high_ratio", None), ("lufs", None), ("_env_warm", -1), ("_env_rounds", -1),
            ("_comp_m_table", None))


def worker_count(workers, n_jobs):
    """the thread pool's size: `workers`, by default min(8, jobs), at least 1 and at most
    16 -- never derived from the machine's CPU count"""
    if workers is None:
        workers = min(DEFAULT_WORKERS, n_jobs)
    if isinstance(workers, bool) or not isinstance(workers, (int, np.integer)):
        raise ValueError("workers must be an int, not %r" % (workers,))
    return max(1, min(MAX_WORKERS, int(workers)))


# --------------------------------------------------------------------- headers (host)
class Header:
    """What a file's container says, without its samples: the rate, the channels, the PCM
    code amx_pcm_to_s16 takes (a FLAC file: "s32", the decoder's samples), the frames
    (a FLAC file without a length: 0), where the payload lies in the file, and the kind
    of container."""

    def __init__(self, sample_rate, channels, code, frames, kind="wav", info=None, offset=0, nbytes=0,
                 file_bytes=0):
        self.sample_rate, self.channels, self.code, self.frames = int(sample_rate), int(channels), code, int(frames)
        self.kind, self.offset, self.nbytes, self.file_bytes = kind, int(offset), int(nbytes), int(file_bytes)
        self.info = info

    @property
    def chain_input(self):
        """the chain input kind: ("f32", 1), ("f32", 2) or ("s16", 2); a file with 3..8
        channels: ("mc", channels)"""
        if self.channels > 2:
            return ("mc", self.channels)
        ch_in, s16, _ = wavio.chain_kind(self.channels, self.code)
        return ("s16" if s16 else "f32", ch_in)


def _wav_header(f, size, path):
    """wavio._parse + read_wav_raw on an open file, reading the chunk headers only (the
    same errors in the same order)"""
    f.seek(0)
    head = f.read(12)
    if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file: %s" % path)
    pos, fmt, data = 12, None, None
    while pos + 8 <= size:
        f.seek(pos)
        h = f.read(8)
        cid, csize = h[:4], struct.unpack("<I", h[4:8])[0]
        if cid == b"fmt ":
            body = f.read(min(csize, 40))
            tag, ch, fs, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and len(body) >= 26:
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = WavInfo(fs, ch, tag, bits)
        elif cid == b"data":
            data = (pos + 8, max(0, min(csize, size - pos - 8)))
        pos += 8 + csize + (csize & 1)
    if fmt is None or data is None:
        raise ValueError("WAV without fmt/data chunk: %s" % path)
    if fmt.block_align <= 0:
        raise ValueError("WAV with a zero block size: %s" % path)
    code = wavio.PCM_CODE.get((fmt.fmt_tag, fmt.bits))
    if code is None:
        raise ValueError("unsupported WAV format tag %d / %d bits" % (fmt.fmt_tag, fmt.bits))
    n = data[1] // fmt.block_align
    return Header(fmt.sample_rate, fmt.channels, code, n, "wav", fmt, data[0], n * fmt.block_align, size)


def _aiff_header(f, size, path):
    """aiffio._parse on an open file, reading the chunk headers, COMM and SSND's first
    bytes only (the same errors in the same order; the format decision is aiffio's own)"""
    f.seek(0)
    aifc = f.read(12)[8:12] == b"AIFC"
    pos, comm, ssnd = 12, None, None
    while pos + 8 <= size:
        f.seek(pos)
        h = f.read(8)
        cid, csize = h[:4], struct.unpack(">I", h[4:8])[0]
        have = max(0, min(csize, size - pos - 8))
        if cid == b"COMM":
            comm = aiffio._comm(f.read(min(have, 64)), aifc)
        elif cid == b"SSND":
            off = struct.unpack(">I", f.read(min(have, 4)))[0]
            ssnd = (pos + 16 + off, max(0, have - 8 - off))
        pos += 8 + csize + (csize & 1)
    if comm is None or ssnd is None:
        raise ValueError("AIFF without COMM/SSND chunk: %s" % path)
    info, code, frames = aiffio._format(comm, path)
    n = min(frames, ssnd[1] // info.block_align)
    return Header(info.sample_rate, info.channels, code, n, "aiff", info, ssnd[0], n * info.block_align, size)


def _flac_header(f, size, o):
    """STREAMINFO of a FLAC file (o: the offset past an ID3v2 tag): what the plan needs
    before the stream is decoded.  Anything unexpected gives a header without rate and
    length; the decoder then says what is wrong with the file."""
    f.seek(o)
    b = f.read(42)
    rate = ch = total = 0
    if len(b) == 42 and b[:4] == b"fLaC" and b[4] & 0x7F == 0:
        v = int.from_bytes(b[18:26], "big")
        rate, ch, total = v >> 44, ((v >> 41) & 7) + 1, v & ((1 << 36) - 1)
    return Header(rate, ch, "s32", total, "flac", None, o, size - o, size)


def read_header(path):
    """The Header of a WAV, AIFF / AIFF-C or FLAC file, chosen as wavio.read_audio_raw
    chooses; raises what it raises for a file it cannot take.  Host only, and the samples
    are not read."""
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if head[:4] == b"FORM" and head[8:12] in (b"AIFF", b"AIFC"):
            return _aiff_header(f, size, path)
        from .flacio import _skip_id3
        f.seek(0)
        o = _skip_id3(f.read(4096))
        f.seek(o)
        if f.read(4) == b"fLaC":
            return _flac_header(f, size, o)
        return _wav_header(f, size, path)


# --------------------------------------------------------------------- grouping (host)
def dsp_key(settings):
    """The settings that decide a plan's arithmetic, as a hashable key: two jobs with equal
    keys (and the same rate and chain input) can be tracks of one plan.  None for settings
    that cannot be compared (an unhashable value, tables given as arrays): such a job runs
    alone."""
    if settings.get("_comp_m_table") is not None:
        return None
    key = []
    for k, default in DSP_KEYS:
        v = settings.get(k, default)
        if k == "multiband":
            v = bool(v)
        try:
            hash(v)
        except TypeError:
            return None
        if isinstance(v, float) and v != v:
            return None                                   # NaN never equals itself
        key.append(v)
    return tuple(key)


def plan_groups(headers, jobs, max_group_frames=None):
    """Which jobs share a plan: a list of lists of job indices, the groups ordered by their
    first job and the jobs inside a group in job order.  headers[i]: job i's Header, or None
    for a job that takes no part (it failed before its header was read).

    One group: the same sample rate, the same chain input kind (f32 mono, f32 stereo, s16
    stereo -- every integer, float64, big-endian or FLAC format and every mono non-float
    file becomes s16 stereo through amx_pcm_to_s16), and equal dsp_key.  Delivery keys
    (input_file, output_file, output_rate, flac_lpc_order, flac_decode, create_mp3, the art
    and prompt keys) do not split a group.  A file with 3..8 channels, an empty file, a FLAC
    file whose header names no length and a job whose settings cannot be compared stand
    alone.  A group holds at most max_group_frames frames (None: no bound but the plan's)
    and fewer than 2^31; larger ones are split in job order (a single file over the bound
    still gets its group: the plan refuses it with its own error)."""
    cap = MAX_PLAN_FRAMES if max_group_frames is None else max(1, min(int(max_group_frames), MAX_PLAN_FRAMES))
    groups, open_group = [], {}
    for i, (h, job) in enumerate(zip(headers, jobs)):
        if h is None:
            continue
        key = dsp_key(job)
        if key is None or h.channels > 2 or h.frames <= 0 or h.sample_rate <= 0:
            groups.append([i])
            continue
        key = (h.sample_rate, h.chain_input, key)
        g = open_group.get(key)
        if g is None or g[1] + h.frames > cap:
            g = open_group[key] = [[], 0]
            groups.append(g[0])
        g[0].append(i)
        g[1] += h.frames
    return groups


def default_group_frames(free_bytes):
    """max_group_frames when the caller names none: the frames that fit in half of the
    free device memory at DEVICE_BYTES_PER_FRAME each"""
    return max(1, min(MAX_PLAN_FRAMES, int(free_bytes * DEVICE_MEMORY_SHARE) // DEVICE_BYTES_PER_FRAME))


# --------------------------------------------------------------------- staging
class Lease:
    def __init__(self, buf, nbytes):
        self.buf, self.nbytes = buf, nbytes


class StagingPool:
    """A bound on the staging memory in flight.  try_acquire(nbytes) gives a Lease (its buf
    from `alloc`) or None while the pool is full; an empty pool grants any size, so a file
    larger than the pool is staged alone.  peak: the most it ever held."""

    def __init__(self, capacity, alloc):
        self.capacity, self.alloc = max(1, int(capacity)), alloc
        self.used = self.peak = 0
        self._lock = threading.Lock()

    def try_acquire(self, nbytes):
        nbytes = int(nbytes)
        with self._lock:
            if self.used and self.used + nbytes > self.capacity:
                return None
            self.used += nbytes
            self.peak = max(self.peak, self.used)
        try:
            return Lease(self.alloc(max(1, nbytes)), nbytes)
        except BaseException:
            with self._lock:
                self.used -= nbytes
            raise

    def release(self, lease):
        if lease is not None and lease.buf is not None:
            lease.buf = None
            with self._lock:
                self.used -= lease.nbytes


class ReadAhead:
    """Reads in the order their results are used.  tasks[k] = (nbytes, fn): fn(buf) runs on
    the executor with a staging buffer of nbytes from the pool.  A read starts only once
    the pool has room for it and every earlier read has started, so the pool never holds
    more than its capacity, and what it holds is always what the consumer needs next: a
    full pool cannot keep the consumer from the read it waits for.  (The reader therefore
    never blocks inside a worker: it is not started before its buffer exists.  The buffers
    are allocated by the thread that calls pump(), the calling thread.)"""

    def __init__(self, pool, executor, tasks):
        self.pool, self.executor, self.tasks = pool, executor, tasks
        self.futures = [None] * len(tasks)
        self.leases = [None] * len(tasks)
        self.released = [False] * len(tasks)
        self.started = 0

    def pump(self):
        while self.started < len(self.tasks):
            nbytes, fn = self.tasks[self.started]
            lease = self.pool.try_acquire(nbytes)
            if lease is None:
                return
            k = self.started
            self.leases[k] = lease
            self.futures[k] = self.executor.submit(fn, lease.buf)
            self.started += 1

    def future(self, k, make_room):
        """task k's future; make_room() frees the staging of results already used when the
        pool is too full for k to start"""
        if self.released[k]:
            raise RuntimeError("amx.files: read %d was released" % k)
        self.pump()
        if self.futures[k] is None:
            make_room()
            self.pump()
        if self.futures[k] is None:
            raise RuntimeError("amx.files: read %d cannot start (staging pool holds %d bytes)" % (k, self.pool.used))
        return self.futures[k]

    def release(self, k):
        """read k's staging back to the pool.  The future goes too: its result holds a
        view of the buffer, which would keep the memory allocated until the call ends."""
        self.pool.release(self.leases[k])
        self.leases[k] = None
        self.futures[k] = None
        self.released[k] = True


def _readinto(f, view):
    """fill the memoryview from the file; a short file is an error"""
    got = 0
    while got < len(view):
        n = f.readinto(view[got:])
        if not n:
            raise OSError("unexpected end of file after %d of %d bytes" % (got, len(view)))
        got += n


class Staged:
    """One file's samples in host memory, ready for the device: raw (a uint8 array: the
    payload, the decoded FLAC samples, or with device=True the FLAC file's bytes), and --
    unless the device decodes -- the WavInfo, PCM code and frames master_audio sees."""

    def __init__(self, raw, info=None, code=None, frames=0, device=False):
        self.raw, self.info, self.code, self.frames, self.device = raw, info, code, frames, device


def staging_bytes_for(header, flac_mode):
    """the staging a file's read needs"""
    if header.kind != "flac":
        return header.nbytes
    if flac_mode == "device":
        return header.nbytes
    return header.frames * header.channels * 4


def read_staged(path, header, flac_mode, buf):
    """Worker: the file's samples into the staging buffer `buf` (a uint8 array of
    staging_bytes_for bytes).  WAV / AIFF: the payload, read in place.  FLAC: the file's
    bytes (flac_mode "device"), or the host decoder's samples, decoded into buf when
    STREAMINFO named their number."""
    from . import flacio
    with open(path, "rb") as f:
        if header.kind != "flac":
            f.seek(header.offset)
            _readinto(f, memoryview(buf)[:header.nbytes])
            return Staged(buf[:header.nbytes], header.info, header.code, header.frames)
        if flac_mode == "device":
            f.seek(header.offset)
            _readinto(f, memoryview(buf)[:header.nbytes])
            return Staged(buf[:header.nbytes], device=True)
        data = np.empty(header.file_bytes, np.uint8)
        _readinto(f, memoryview(data))

    def alloc(frames, channels):
        if frames * channels * 4 <= buf.size and frames > 0:
            return buf[:frames * channels * 4].view(np.int32).reshape(frames, channels)
        return np.empty((frames, channels), np.int32)
    x, finfo, blocks = flacio.decode_flac(data, with_blocks=True, alloc=alloc)
    info = WavInfo(finfo.sample_rate, finfo.channels, 1, 32)
    info.packet_starts = np.concatenate([[0], np.cumsum(blocks.astype(np.int64))[:-1]])
    return Staged(x.view(np.uint8).reshape(-1), info, "s32", x.shape[0])


# --------------------------------------------------------------------- write behind
def wav_header_s16(n_bytes, channels, fs):
    """wavio.write_wav_s16's 44 bytes"""
    hdr = b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVE"
    hdr += b"fmt " + struct.pack("<IHHIIHH", 16, 1, channels, fs, fs * channels * 2, channels * 2, 16)
    return hdr + b"data" + struct.pack("<I", n_bytes)


def write_master(path, samples, channels, fs, flac=None):
    """Worker: the output file from the staging buffer.  samples: the master's int16 frames
    as a uint8 array.  flac None: a 16-bit WAV.  Else (payload uint8 array, frame lengths
    int32 array, frames, block): flacio.flac_bytes' file -- the MD5 of the samples is taken
    here.  Nothing is copied: the file is written from the arrays.  A file this call began
    is removed if it cannot be finished.  Returns the seconds (MD5 and container, write)."""
    import time
    t0 = time.perf_counter()
    if flac is None:
        parts = [wav_header_s16(samples.size, channels, fs), samples]
        t1 = t0
    else:
        from . import flacio
        payload, fbytes, frames, block = flac
        head = flacio.flac_container(b"", fbytes, fs, channels, frames, block, hashlib.md5(samples).digest())
        parts = [head, payload]
        t1 = time.perf_counter()
    opened = False
    try:
        with open(path, "wb") as f:
            opened = True
            for p in parts:
                f.write(p)
    except BaseException:
        if opened:
            try:
                os.remove(path)
            except OSError:
                pass
        raise
    return t1 - t0, time.perf_counter() - t1


# --------------------------------------------------------------------- the run
class _Track:
    def __init__(self, index, settings):
        self.index, self.settings = index, settings
        self.result = {"index": index, "input_file": settings.get("input_file"),
                       "output_file": settings.get("output_file"), "error": None, "sample_rate": None,
                       "mode": None, "stats": None, "group": None}
        self.header = None
        self.flac_mode = "host"
        self.done = False            # failed, or its output is with the writers
        self.held = []               # callbacks held back until the file is written
        self.d_in = None

    def fail(self, exc):
        self.result["error"] = exc
        self.result["sample_rate"] = self.result["mode"] = self.result["stats"] = None
        self.done = True
        self.d_in = None


class FileBatch:
    """One master_files call.  Everything here runs on the calling thread but read_header,
    read_staged and write_master."""

    def __init__(self, engine, jobs, status_callback, progress_callback, workers, staging_bytes, max_group_frames):
        self._ame = engine           # the drop-in module's helpers (_check_settings, _chain_input, _master_device)
        self.jobs = jobs
        self.status_cb, self.progress_cb = status_callback, progress_callback
        self.n_workers = worker_count(workers, len(jobs))
        staging = DEFAULT_STAGING_BYTES if staging_bytes is None else int(staging_bytes)
        if staging <= 0:
            raise ValueError("staging_bytes must be positive, not %r" % (staging_bytes,))
        self.staging = staging
        self.max_group_frames = max_group_frames
        self.tracks = [_Track(i, job) for i, job in enumerate(jobs)]
        self.times = {}              # per-stage perf_counter sums (scripts/master_files_bench.py)
        self.device_events = []      # (start, end) HIP events around each group's device stage
        self.writes = []             # (future, track, lease, refs)
        self.handover = []           # (event, track, lease, args, refs): D2H enqueued, not yet with a writer
        self.uploads = []            # (event, read index): H2D enqueued from a staging buffer

    # ---------------------------------------------------------------- callbacks
    def status(self, t, msg):
        if self.status_cb is not None:
            self.status_cb(t.index, msg)

    def progress(self, t, cur, total):
        if self.progress_cb is not None:
            self.progress_cb(t.index, cur, total)

    def _emit_device_stage(self, t, num_chunks):
        """master_audio's callbacks between "Splitting complete." and the write, for a
        track of a batched group (whose device stage has succeeded)"""
        total = num_chunks + 4
        for i in range(num_chunks):
            self.status(t, f"Processing chunk {i+1} of {num_chunks}...")
            self.progress(t, i + 1, total)
        self.status(t, "Re-assembling processed chunks with concat filter...")
        self.progress(t, num_chunks + 1, total)
        self.status(t, "Concatenation complete.")
        if t.settings.get("lufs") is not None:
            self.status(t, "Normalizing final loudness...")
            self.progress(t, num_chunks + 2, total)
        self.status(t, "Applying final limiting and exporting...")
        self.progress(t, num_chunks + 3, total)

    # ---------------------------------------------------------------- the stages
    def run(self):
        from .engine import delivery_rate
        from .settings import flac_decode_mode
        ame, self._delivery_rate = self._ame, delivery_rate
        live = []
        for t in self.tracks:
            try:
                ame._check_settings(t.settings)
                t.flac_mode = flac_decode_mode(t.settings)
                live.append(t)
            except Exception as e:   # noqa: BLE001 -- the job's own error, as master_audio raises it
                t.fail(e)
        for t in live:
            self.status(t, "Splitting audio into manageable chunks...")
            self.progress(t, 0, 100)
        if live:
            with ThreadPoolExecutor(max_workers=self.n_workers, thread_name_prefix="amx-files") as ex:
                self.executor = ex
                try:
                    self._run_live(live)
                finally:
                    self._drain()
        gid = 1 + max((t.result["group"] for t in self.tracks if t.result["group"] is not None), default=-1)
        for t in self.tracks:
            if t.result["group"] is None:
                t.result["group"] = gid
                gid += 1
        return [t.result for t in self.tracks]

    def _run_live(self, live):
        import time
        import torch
        from . import capi
        capi.load()                                  # (before a worker's host FLAC decode needs it)
        # headers first: they decide the groups, and the groups the order of the reads
        t0 = time.perf_counter()
        futs = [self.executor.submit(read_header, t.settings["input_file"]) for t in live]
        for t, f in zip(live, futs):
            try:
                t.header = f.result()
                if t.header.kind != "flac":
                    self._check_header(t, t.header.sample_rate, t.header.channels)
            except Exception as e:   # noqa: BLE001
                t.fail(e)
        self.times["header"] = time.perf_counter() - t0
        headers = [None if t.done else t.header for t in self.tracks]
        mgf = self.max_group_frames
        if mgf is None and any(h is not None for h in headers):
            mgf = default_group_frames(torch.cuda.mem_get_info()[0])
        groups = plan_groups(headers, self.jobs, mgf)
        order = [i for g in groups for i in g]
        self.read_index = {i: k for k, i in enumerate(order)}
        half = max(1, self.staging // 2)             # one half reads ahead, one writes behind
        pin = lambda n: torch.empty(n, dtype=torch.uint8, pin_memory=True)   # noqa: E731
        self.pool_in, self.pool_out = StagingPool(half, pin), StagingPool(half, pin)
        tasks = []
        for i in order:
            t = self.tracks[i]
            tasks.append((staging_bytes_for(t.header, t.flac_mode), self._reader(t)))
        self.reads = ReadAhead(self.pool_in, self.executor, tasks)
        self.copy_in, self.copy_out = torch.cuda.Stream(), torch.cuda.Stream()
        for gid, g in enumerate(groups):
            members = [self.tracks[i] for i in g]
            for t in members:
                t.result["group"] = gid
            self._run_group(members)

    def _reader(self, t):
        path, header, mode = t.settings["input_file"], t.header, t.flac_mode

        def fn(buf):
            import time
            t0 = time.perf_counter()
            r = read_staged(path, header, mode, buf.numpy())
            r.seconds = time.perf_counter() - t0
            return r
        return fn

    def _add(self, stage, seconds):
        self.times[stage] = self.times.get(stage, 0.0) + seconds

    def _check_header(self, t, rate, channels):
        """master_audio's checks once the header is known (_device_input)"""
        if not 1 <= channels <= 8:
            raise ValueError("1 to 8 channels are supported (%d channels)" % channels)
        self._delivery_rate(t.settings, rate, channels)

    # ---------------------------------------------------------------- stage 2: device
    def _make_room(self):
        """the staging of every upload enqueued so far is free once its copy is done"""
        for ev, k in self.uploads:
            ev.synchronize()
            self.reads.release(k)
        self.uploads = []

    def _reap_uploads(self):
        keep = []
        for ev, k in self.uploads:
            if ev.query():
                self.reads.release(k)
            else:
                keep.append((ev, k))
        self.uploads = keep

    def _wait_read(self, k):
        """read k's result; meanwhile finished writes are reaped and further reads started"""
        fut = self.reads.future(k, self._make_room)
        while not fut.done():
            wait([fut] + [w[0] for w in self.writes], return_when=FIRST_COMPLETED)
            self._reap_writes()
            self._reap_uploads()
            self.reads.pump()
        return fut.result()

    def _upload(self, t, dst=None):
        """Track t's samples to the device as the chain reads them (t.d_in, frames, bounds);
        dst: its slice of the group's input (None: a tensor of its own).  The H2D runs on
        the copy stream from the pinned staging buffer; the launch stream waits for it."""
        import time
        k = self.read_index[t.index]
        try:
            st = self._wait_read(k)
            self._add("read", st.seconds)
            t0 = time.perf_counter()
            self._to_device(t, k, st, dst)
            self._add("stage", time.perf_counter() - t0)
        except BaseException:
            if not any(k == u[1] for u in self.uploads):
                self.reads.release(k)
            raise
        self.status(t, "Splitting complete.")

    def _to_device(self, t, k, st, dst):
        import torch
        from . import flacio
        cur = torch.cuda.current_stream()

        def fits(info, frames):
            # the slice was cut from the header: the file must be what the header said
            return (dst is not None and frames == dst.shape[0] and info.sample_rate == t.header.sample_rate
                    and info.channels == t.header.channels)
        if st.device:
            # the device decoder stages the bytes itself and synchronises
            x, finfo, blocks = flacio.decode_flac_device(st.raw)
            self.reads.release(k)
            info = WavInfo(finfo.sample_rate, finfo.channels, 1, 32)
            info.packet_starts = np.concatenate([[0], np.cumsum(blocks.astype(np.int64))[:-1]])
            code, frames, d_raw = "s32", int(x.shape[0]), x
            self._check_header(t, info.sample_rate, info.channels)
            direct = False
        else:
            info, code, frames = st.info, st.code, st.frames
            if t.header.kind == "flac":
                self._check_header(t, info.sample_rate, info.channels)
            direct = wavio.chain_kind(info.channels, code)[2]
            if direct and fits(info, frames):
                d_raw = dst.view(torch.uint8).reshape(-1)          # the file's bytes are the chain input
            else:
                d_raw = torch.empty(st.raw.size, dtype=torch.uint8, device="cuda")
            h = torch.from_numpy(st.raw)
            pinned = h.is_pinned()
            self.copy_in.wait_stream(cur)          # (the destination's earlier use has been enqueued)
            with torch.cuda.stream(self.copy_in):
                d_raw.copy_(h, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.copy_in)
            cur.wait_event(ev)
            if pinned:
                self.uploads.append((ev, k))
            else:
                self.reads.release(k)              # (a pageable copy has returned from the host side)
        in_place = fits(info, frames)
        d_in, ch_in, s16 = self._ame._chain_input(d_raw, info.channels, code, frames,
                                                  out=dst if in_place and not direct else None)
        if d_in.dim() == 1:
            d_in = d_in.reshape(-1, ch_in)
        t.d_in, t.frames, t.fs, t.ch_in, t.s16 = d_in, frames, info.sample_rate, ch_in, s16
        t.in_place = in_place
        t.bounds = bounds_for(frames, info.sample_rate, info)
        t.target = output_rate(t.settings, info.sample_rate)
        self._flush_handover(block=False)

    def _run_group(self, members):
        import torch
        if len(members) == 1:
            t = members[0]
            try:
                self._upload(t)
            except Exception as e:   # noqa: BLE001
                t.fail(e)
                return
            self._run_single(t)
            return
        t0 = members[0]
        kind, ch_in = t0.header.chain_input
        total = sum(t.header.frames for t in members)
        d_all = torch.empty((total, ch_in), dtype=torch.int16 if kind == "s16" else torch.float32, device="cuda")
        off = 0
        for t in members:
            try:
                self._upload(t, d_all[off:off + t.header.frames])
            except Exception as e:   # noqa: BLE001
                t.fail(e)
            off += t.header.frames
        ok = [t for t in members if not t.done]
        same = [t for t in ok if (t.fs, t.ch_in, t.s16) == (t0.header.sample_rate, ch_in, kind == "s16")
                and t.frames > 0]
        stray = [t for t in ok if t not in same]
        if len(same) >= 2:
            if len(same) == len(members) and all(t.in_place for t in same):
                d_in = d_all
            else:
                # a member failed or is not what its header said: the others, back to back
                d_in = torch.cat([t.d_in for t in same])
            self._flush_handover()
            try:
                outs = self._device_stage(same, d_in)
            except Exception:   # noqa: BLE001
                # one at a time through master_audio's own sequence: each file then gets its
                # own :243-246 fallback, or its own error
                logging.exception("master_files: a group of %d files failed on the device; "
                                  "running them one at a time", len(same))
                outs = None
            del d_in
            if outs is None:
                stray = ok
            else:
                for t, (y, fs_out) in zip(same, outs):
                    self._emit_device_stage(t, len(t.bounds))
                    try:
                        rate = {"sample_rate": fs_out}
                        y = self._deliver_rate(y, rate, t.target)
                        t.result["sample_rate"] = int(rate["sample_rate"])
                        self._deliver(t, y, rate["sample_rate"])
                    except Exception as e:   # noqa: BLE001
                        t.fail(e)
                    t.d_in = None
        else:
            stray = ok
        del d_all
        for t in stray:
            self._run_single(t)

    def _deliver_rate(self, y, rate, target):
        from .engine import deliver
        return deliver(y, rate, target)

    def _device_stage(self, tracks, d_in):
        """One MasteringJob for the group, each file with its own chunk bounds, through
        master_audio's call sequence; returns [(y, rate)] per track and fills mode / stats"""
        import torch
        from .engine import MasteringJob
        t0 = tracks[0]
        settings = t0.settings
        frames = [t.frames for t in tracks]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        job = MasteringJob(t0.fs, t0.ch_in, settings, frames, input_s16=t0.s16,
                           chunks=plan_tracks(frames, t0.fs, explicit=[t.bounds for t in tracks]))
        try:
            job.run_chunks(d_in)
            torch.cuda.current_stream().synchronize()
            job.loudness_pass1()
            lufs = settings.get("lufs") is not None
            if lufs:
                job.loudness_pass2(carry=False)
                job.histograms()
            job.decide()
            rep = job.fetch_report(raise_dynamic=False)
            dyn_out = {}
            if lufs:
                # (one dynamic track: dynamic_track, master_audio's own call; several: side by
                # side on streams of their own)
                job.finish_dynamic(rep)
                dyn_out = {i: (y, info["sample_rate"]) for i, (y, info) in job.dyn_out.items()}
            job.finalize(None)
            outs = [dyn_out[i] if i in dyn_out else (job.track_output(i), t.fs) for i, t in enumerate(tracks)]
            b.record()
            self.device_events.append((a, b))
        finally:
            job.close()
        for i, t in enumerate(tracks):
            mode = rep["modes"][i] if lufs else "off"
            if mode == "skip":
                logging.warning("Measured loudness is -inf (silent audio). Skipping normalization.")
            t.result["mode"] = mode
            t.result["stats"] = rep["stats"][i] if lufs else None
        return outs

    def _run_single(self, t):
        """master_audio's own sequence from "Splitting complete." on, for a file that is
        alone in its group or whose group failed; the write goes behind like every other"""
        import torch
        self._flush_handover()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()

        def progress(cur, total):
            if cur == total:
                t.held.append((cur, total))      # :224 fires once the file is written
            else:
                self.progress(t, cur, total)

        def write(path, y, fs, settings):
            b.record()
            self.device_events.append((a, b))
            self._deliver(t, y, fs)
        res = {}
        try:
            self._ame._master_device(t.settings, lambda m: self.status(t, m), progress, t.d_in, t.fs, t.frames,
                                     t.ch_in, t.s16, t.bounds, t.settings["output_file"], t.target,
                                     write=write, result=res)
            t.result.update(res)
        except Exception as e:   # noqa: BLE001
            t.held = []
            t.fail(e)
        t.d_in = None

    # ---------------------------------------------------------------- stage 2 -> 3
    def _deliver(self, t, y, fs):
        """The finished master y (a device int16 tensor [frames, channels]) on its way to
        its file: for a *.flac name the device encode, then D2H into pinned staging on the
        copy stream; the writers take it once the copy's event has passed."""
        import time
        import torch
        from . import flacio
        t0 = time.perf_counter()
        path = t.settings["output_file"]
        if y.dim() == 1:
            y = y[:, None]
        y = y.contiguous()
        frames, channels = int(y.shape[0]), int(y.shape[1])
        parts = [y.view(torch.uint8).reshape(-1) if frames else y.new_empty(0, dtype=torch.uint8)]
        flac = None
        if os.path.splitext(str(path))[1].lower() == ".flac":
            lpc = flacio._lpc_order((t.settings or {}).get("flac_lpc_order", 0))
            if frames:
                payload, fbytes = flacio.encode_flac_device(y, fs, 4096, lpc_order=lpc)
                parts += [payload, fbytes.view(torch.uint8).reshape(-1)]
            flac = True
        offs, need = [], 0
        for p in parts:
            offs.append(need)
            need += (p.numel() + 15) & ~15
        lease = self._acquire_out(need)
        cur = torch.cuda.current_stream()
        self.copy_out.wait_stream(cur)
        host = lease.buf
        with torch.cuda.stream(self.copy_out):
            for p, o in zip(parts, offs):
                if p.numel():
                    host[o:o + p.numel()].copy_(p, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_out)
        h = host.numpy()
        views = [h[o:o + p.numel()] for p, o in zip(parts, offs)]
        if flac:
            if frames:
                flac = (views[1], views[2].view(np.int32), frames, 4096)
            else:
                flac = (np.empty(0, np.uint8), np.empty(0, np.int32), 0, 4096)
        args = (path, views[0], channels, int(fs), flac if flac else None)
        # (parts: the device tensors stay referenced until the copy's event has passed)
        self.handover.append((ev, t, lease, args, parts))
        self.times["d2h_enqueue"] = self.times.get("d2h_enqueue", 0.0) + (time.perf_counter() - t0)
        self._flush_handover(block=False)

    def _flush_handover(self, block=True):
        """hand every finished D2H (block: every enqueued one) to the writers"""
        import time
        keep = []
        for ev, t, lease, args, refs in self.handover:
            if not block and not ev.query():
                keep.append((ev, t, lease, args, refs))
                continue
            t0 = time.perf_counter()
            ev.synchronize()
            self.times["d2h"] = self.times.get("d2h", 0.0) + (time.perf_counter() - t0)
            fut = self.executor.submit(write_master, *args)
            self.writes.append((fut, t, lease))
        self.handover = keep

    def _acquire_out(self, nbytes):
        while True:
            lease = self.pool_out.try_acquire(nbytes)
            if lease is not None:
                return lease
            if self.handover:
                self._flush_handover()
            elif self.writes:
                wait([w[0] for w in self.writes], return_when=FIRST_COMPLETED)
            else:
                raise RuntimeError("amx.files: the output staging pool holds %d bytes nobody owns"
                                   % self.pool_out.used)
            self._reap_writes()

    def _reap_writes(self, block=False):
        keep = []
        for fut, t, lease in self.writes:
            if not block and not fut.done():
                keep.append((fut, t, lease))
                continue
            try:
                md5_s, write_s = fut.result()
                self._add("md5", md5_s)
                self._add("write", write_s)
            except Exception as e:   # noqa: BLE001
                t.held = []
                t.fail(e)
            self.pool_out.release(lease)
            if t.result["error"] is None:
                n = len(t.bounds)
                for cur, total in (t.held or [(n + 4, n + 4)]):
                    self.progress(t, cur, total)
                t.held = []
                logging.info("Finished GPU pipeline, exported to %s", t.settings["output_file"])
            t.done = True
        self.writes = keep

    def _drain(self):
        """everything in flight to its end (also on the way out of an error)"""
        self._flush_handover()
        self._reap_writes(block=True)
        reads = getattr(self, "reads", None)
        if reads is not None:
            for ev, k in self.uploads:
                ev.synchronize()
            self.uploads = []
            for k, f in enumerate(reads.futures):
                if f is not None:
                    f.cancel()
                    try:
                        f.exception()
                    except BaseException:   # noqa: BLE001 -- a cancelled read
                        pass
                    reads.release(k)


def master_files(engine, jobs, status_callback=None, progress_callback=None, *, workers=None, staging_bytes=None,
                 max_group_frames=None, _times=None):
    """audio_mastering_engine.master_files (its docstring is the contract).  engine: that
    module, whose _check_settings, _chain_input and _master_device are master_audio's own
    pieces (handed in, so this package does not import the module above it)."""
    if not isinstance(jobs, list) or not all(isinstance(j, dict) for j in jobs):
        raise TypeError("master_files takes a list of settings dicts")
    seen = {}
    for i, job in enumerate(jobs):
        out = job.get("output_file")
        if not out:
            continue
        key = os.path.normcase(os.path.abspath(os.fspath(out))) if isinstance(out, (str, bytes, os.PathLike)) else out
        try:
            first = seen.setdefault(key, i)
        except TypeError:
            continue
        if first != i:
            raise ValueError("jobs %d and %d name the same output_file %r" % (first, i, out))
    n_workers = worker_count(workers, len(jobs))      # a bad `workers`: before any file is read
    if not jobs:
        return []
    batch = FileBatch(engine, jobs, status_callback, progress_callback, n_workers, staging_bytes, max_group_frames)
    results = batch.run()
    if _times is not None:
        _times.update(batch.times)
        ms = 0.0
        for a, b in batch.device_events:
            ms += a.elapsed_time(b)
        _times["device_events_ms"] = ms
        _times["staging_peak"] = (batch.pool_in.peak, batch.pool_out.peak) if hasattr(batch, "pool_in") else (0, 0)
    return results
