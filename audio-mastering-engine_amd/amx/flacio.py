"""FLAC input (the GUI's *.flac, mastering_gui.py:170; ffmpeg decodes it at :178) and FLAC
output (an output_file named *.flac, which ffmpeg's last command writes as FLAC, :223).

The bitstream is decoded by libamx's host decoder (amx_flac_decode, csrc/amx_flac.cpp:
frames decoded on a thread pool) into int32 samples left-justified to 32 bits -- the
value ffmpeg's FLAC decoder hands on -- so the file reaches the device decode as s32
PCM (amx_pcm_to_s16: >> 16, what the segment muxer's s16 WAV chunks hold).
decode_flac_device fills the same array on the device instead (amx_flac_decode_device,
csrc/amx_flacdec.hip): the host only lists the frame starts (amx_flac_scan) and uploads
the file's bytes.

The write side encodes on the device (amx_flac_encode, csrc/amx_flacenc.hip): the int16
master stays where the limiter left it, only the encoded frames cross the bus, and the
host adds the 42 bytes in front of them (flac_container).
"""
import ctypes

import numpy as np

from . import capi
from .wavio import WavInfo


def _skip_id3(data):
    """offset past a leading ID3v2 tag (taggers prepend one; ffmpeg skips it)"""
    if len(data) >= 10 and data[:3] == b"ID3":
        size = ((data[6] & 0x7F) << 21) | ((data[7] & 0x7F) << 14) | ((data[8] & 0x7F) << 7) | (data[9] & 0x7F)
        off = 10 + size + (10 if data[5] & 0x10 else 0)
        return off
    return 0


def is_flac(path):
    with open(path, "rb") as f:
        head = f.read(4096)
    o = _skip_id3(head)
    if o + 4 > len(head):
        with open(path, "rb") as f:
            f.seek(o)
            return f.read(4) == b"fLaC"
    return head[o:o + 4] == b"fLaC"


# samples per byte a FLAC stream can reach at most: a frame of the largest block
# (65535 samples) is at least ~11 bytes (a 6-byte header + the 16-bit block size, one
# constant subframe of 2 bytes, the CRC-16), i.e. <= ~5958 samples per byte; a
# STREAMINFO length beyond 6144 per byte is not trusted for the allocation (a size
# query decides it first), so valid streams -- long silence included -- decode once
_MAX_SAMPLES_PER_BYTE = 6144


def decode_flac(data, threads=0, with_blocks=False, alloc=None):
    """(int32 array [frames, channels] left-justified to 32 bits, FlacInfo) of FLAC bytes;
    with_blocks: also the FLAC frames' block sizes in stream order (the demuxer's packets);
    alloc(frames, channels): the int32 array to decode into (amx.files: a view of pinned
    staging memory), None: a new one"""
    # the decoder reads the caller's bytes in place (no copy): a numpy view of them
    raw = np.frombuffer(data, np.uint8)
    o = _skip_id3(raw[:10].tobytes())
    size = raw.size - o
    if size <= 0:
        raise capi.AmxError("not a FLAC stream (empty)")
    buf = ctypes.c_void_p(raw.ctypes.data + o)
    L = capi.load()
    info = capi.FlacInfo()
    rc = L.amx_flac_info(buf, size, ctypes.byref(info))
    if rc != capi.AMX_OK:
        raise capi.AmxError("not a FLAC stream (amx_flac_info %d)" % rc)
    n = ctypes.c_int64(info.total_frames)
    if n.value <= 0 or n.value > size * _MAX_SAMPLES_PER_BYTE:
        # STREAMINFO without the length, or one the file cannot hold: a size query first
        rc = L.amx_flac_decode(buf, size, None, 0, ctypes.byref(n), int(threads), None, 0, None)
        if rc != capi.AMX_OK:
            raise capi.AmxError("corrupt FLAC stream (amx_flac_decode %d)" % rc)
    out = np.empty((n.value, info.channels), np.int32) if alloc is None else alloc(n.value, info.channels)
    got = ctypes.c_int64(0)
    # frames of at least 16 samples (the format's minimum block size but the last)
    max_blocks = n.value // 16 + 2
    blocks = np.zeros(max_blocks, np.int32)
    nb = ctypes.c_int64(0)
    rc = L.amx_flac_decode(buf, size, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(got),
                           int(threads), blocks.ctypes.data_as(ctypes.c_void_p), max_blocks, ctypes.byref(nb))
    if rc != capi.AMX_OK or got.value != n.value:
        raise capi.AmxError("corrupt FLAC stream (amx_flac_decode %d)" % rc)
    if with_blocks:
        return out, info, blocks[:nb.value].copy()
    return out, info


def flac_scan(data, room=None):
    """amx_flac_scan of FLAC bytes (no ID3 tag in front): (rc, FlacScan, candidate table as a
    uint8 array of FlacCand records, or None unless rc is AMX_OK).  Host only.  `room`: a
    uint8 array to build the table in (the caller's pinned staging buffer), else a fresh one."""
    raw = np.frombuffer(data, np.uint8)
    L = capi.load()
    sc = capi.FlacScan()
    rec = ctypes.sizeof(capi.FlacCand)
    buf = ctypes.c_void_p(raw.ctypes.data)
    # most streams hold a frame per few kilobytes: room for one per 256 bytes, else ask again
    cap = raw.size // 256 + 1024 if room is None else room.size // rec
    tab = np.empty(cap * rec, np.uint8) if room is None else room
    rc = L.amx_flac_scan(buf, raw.size, tab.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(sc))
    if rc == capi.AMX_ERANGE:
        cap = sc.n_cand
        tab = np.empty(cap * rec, np.uint8)
        rc = L.amx_flac_scan(buf, raw.size, tab.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(sc))
    if rc != capi.AMX_OK:
        return rc, sc, None
    return rc, sc, tab[:sc.n_cand * rec]


def _flac_host_to_device(data):
    """decode_flac_device's result by the host decoder and an upload: what a stream outside
    the device path's range gets (amx.h, AMX_EUNSUPPORTED)"""
    import torch
    x, info, blocks = decode_flac(data, with_blocks=True)
    return torch.from_numpy(x).to("cuda"), info, blocks


def decode_flac_device(data):
    """decode_flac(data, with_blocks=True) on the device: (int32 device tensor [frames,
    channels] left-justified to 32 bits, FlacInfo, block sizes).  The file's bytes and the
    host scan's candidate table go up from one pinned buffer; three kernels decode, chain
    and place the frames (amx_flac_decode_device).  Raises AmxError with
    decode_flac's messages; a stream the device path does not cover (more than 24 bits, no
    length in STREAMINFO) goes through decode_flac and an upload."""
    import torch
    raw = np.frombuffer(data, np.uint8)
    o = _skip_id3(raw[:10].tobytes())
    size = raw.size - o
    if size <= 0:
        raise capi.AmxError("not a FLAC stream (empty)")
    raw = raw[o:]
    L = capi.load()
    info = capi.FlacInfo()
    rc = L.amx_flac_info(ctypes.c_void_p(raw.ctypes.data), size, ctypes.byref(info))
    if rc != capi.AMX_OK:
        raise capi.AmxError("not a FLAC stream (amx_flac_info %d)" % rc)
    # one pinned staging buffer: the stream, then (16-byte aligned) the candidate table
    rec = ctypes.sizeof(capi.FlacCand)
    t_off = (size + 15) & ~15
    stage = torch.empty(t_off + (size // 256 + 1024) * rec, dtype=torch.uint8, pin_memory=True)
    h = stage.numpy()
    h[:size] = raw
    rc, sc, tab = flac_scan(h[:size], room=h[t_off:])
    if rc == capi.AMX_EUNSUPPORTED:
        return _flac_host_to_device(data)
    if rc != capi.AMX_OK:
        raise capi.AmxError("corrupt FLAC stream (amx_flac_decode %d)" % rc)
    if tab.ctypes.data != h.ctypes.data + t_off:
        # more candidates than the staging buffer had room for: a second one for the table
        stage2 = torch.empty(tab.size, dtype=torch.uint8, pin_memory=True)
        stage2.numpy()[:] = tab
        d_data = stage[:size].to("cuda", non_blocking=True)
        d_cand = stage2.to("cuda", non_blocking=True)
    else:
        d_all = stage[:t_off + tab.size].to("cuda", non_blocking=True)
        d_data, d_cand = d_all[:size], d_all[t_off:]
    out = torch.empty((sc.total_frames, sc.channels), dtype=torch.int32, device="cuda")
    d_blocks = torch.empty(sc.n_cand, dtype=torch.int32, device="cuda")
    d_res = torch.empty(4, dtype=torch.int64, device="cuda")
    ws = torch.empty((sc.workspace_bytes + 15) // 16 * 2, dtype=torch.int64, device="cuda")
    capi.check(L.amx_flac_decode_device(capi.ptr(d_data), size, capi.ptr(d_cand), ctypes.byref(sc), capi.ptr(out),
                                        sc.total_frames, capi.ptr(d_blocks), sc.n_cand, capi.ptr(d_res),
                                        capi.ptr(ws), ws.numel() * 8, capi.ptr_stream()),
               "amx_flac_decode_device")
    res = d_res.cpu().numpy()          # (synchronises: the staging buffers are free again)
    if res[0] == capi.AMX_EUNSUPPORTED:
        return _flac_host_to_device(data)
    if res[0] != capi.AMX_OK or res[1] != sc.total_frames:
        raise capi.AmxError("corrupt FLAC stream (amx_flac_decode %d)" % res[0])
    return out, info, d_blocks[:int(res[2])].cpu().numpy()


def read_flac_native(path):
    """(int32 [frames, channels] left-justified samples, WavInfo of s32 PCM).  The WavInfo
    also carries packet_starts: the first sample of every FLAC frame, the packets the
    segment split cuts at (chunking.chunk_bounds_packets)"""
    with open(path, "rb") as f:
        x, info, blocks = decode_flac(f.read(), with_blocks=True)
    w = WavInfo(info.sample_rate, info.channels, 1, 32)
    w.packet_starts = np.concatenate([[0], np.cumsum(blocks.astype(np.int64))[:-1]])
    return x, w


def read_flac_raw(path):
    """read_wav_raw's triple for a FLAC file: the decoded samples as s32 PCM bytes (the
    WavInfo with packet_starts)"""
    x, fmt = read_flac_native(path)
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1), fmt, "s32"


def flac_container(payload, frame_bytes, fs, channels, total_frames, block, md5=None):
    """FLAC file bytes: 'fLaC', one STREAMINFO block marked last, then the frame stream
    `payload` (bytes-like).  frame_bytes: every frame's length (STREAMINFO's min / max frame
    size); block: the fixed block size (the minimum too, unless the stream is one shorter
    frame: then both fields hold its length, but no less than 16); md5: the 16-byte MD5 of the little-endian interleaved samples, or None for
    zeros ("unknown", RFC 9639 8.2).  Pure host code."""
    fb = np.asarray(frame_bytes, np.int64).reshape(-1)
    total_frames, block = int(total_frames), int(block)
    if not 1 <= channels <= 8 or not 1 <= fs <= 1048575 or not 16 <= block <= 65535:
        raise ValueError("flac_container: channels 1..8, rate 1..1048575, block 16..65535")
    if md5 is None:
        md5 = bytes(16)
    if len(md5) != 16:
        raise ValueError("flac_container: md5 must be 16 bytes")
    if fb.size != (total_frames + block - 1) // block:
        raise ValueError("flac_container: %d frame lengths for %d samples in blocks of %d"
                         % (fb.size, total_frames, block))
    # (RFC 9639 8.2: both block sizes lie in 16..65535, also for one frame of 1..15 samples)
    max_block = block if fb.size != 1 else max(16, total_frames)
    min_block = max_block if fb.size <= 1 else block
    min_frame = int(fb.min()) if fb.size else 0
    max_frame = int(fb.max()) if fb.size else 0
    if max_frame >= 1 << 24:
        min_frame = max_frame = 0                      # "unknown": the field holds 24 bits
    v = min_block
    for value, bits in ((max_block, 16), (min_frame, 24), (max_frame, 24), (int(fs), 20),
                        (channels - 1, 3), (16 - 1, 5), (total_frames, 36)):
        v = (v << bits) | (int(value) & ((1 << bits) - 1))
    head = b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + v.to_bytes(18, "big") + bytes(md5)
    return head + bytes(payload)


def _lpc_order(lpc_order):
    """lpc_order as an int in 0..8 (ValueError otherwise, before any device call)"""
    if isinstance(lpc_order, bool) or not isinstance(lpc_order, (int, np.integer)) or not 0 <= lpc_order <= 8:
        raise ValueError("lpc_order must be an int in 0..8, not %r" % (lpc_order,))
    return int(lpc_order)


def encode_flac_device(d_pcm16, fs, block=4096, sub_bits=False, lpc_order=0):
    """The FLAC frame stream of a device int16 tensor [frames, channels] (or [frames]),
    encoded on the device: (payload uint8 device tensor, frame lengths int32 device tensor);
    with sub_bits also the chosen subframes' sizes in bits, int32 [n_frames, channels].
    lpc_order 1..8 adds LPC subframes up to that order to the search (0: FIXED only)."""
    import torch
    lpc_order = _lpc_order(lpc_order)
    x = d_pcm16
    if x.dtype != torch.int16 or not x.is_cuda:
        raise ValueError("encode_flac_device takes an int16 tensor on the device")
    if x.dim() == 1:
        x = x[:, None]
    x = x.contiguous()
    frames, channels = int(x.shape[0]), int(x.shape[1])
    L = capi.load()
    nf, cap, wsb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    capi.check(L.amx_flac_encode_size_ex(frames, channels, int(block), lpc_order, ctypes.byref(nf),
                                         ctypes.byref(cap), ctypes.byref(wsb)), "amx_flac_encode_size_ex")
    dev = x.device
    out = torch.empty(cap.value, dtype=torch.uint8, device=dev)
    fbytes = torch.empty(nf.value, dtype=torch.int32, device=dev)
    sb = torch.empty((nf.value, channels), dtype=torch.int32, device=dev) if sub_bits else None
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty((wsb.value + 7) // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        capi.check(L.amx_flac_encode_ex(capi.ptr(x), frames, channels, int(fs), int(block), lpc_order,
                                        capi.ptr(out), cap.value, capi.ptr(fbytes), capi.ptr(sb), capi.ptr(total),
                                        capi.ptr(ws), ws.numel() * 8, capi.ptr_stream()), "amx_flac_encode_ex")
        n = int(total.item())
    if sub_bits:
        return out[:n], fbytes, sb
    return out[:n], fbytes


def flac_bytes(x16, fs, block=4096, md5=True, lpc_order=0):
    """The FLAC file of int16 samples [frames, channels] (a device tensor or a numpy array);
    lpc_order as in encode_flac_device."""
    import hashlib
    import torch
    lpc_order = _lpc_order(lpc_order)
    if isinstance(x16, np.ndarray):
        x16 = torch.from_numpy(np.ascontiguousarray(x16, np.int16))
    if x16.dim() == 1:
        x16 = x16[:, None]
    frames, channels = int(x16.shape[0]), int(x16.shape[1])
    if frames == 0:
        # nothing to encode: STREAMINFO alone (the MD5 of no samples)
        return flac_container(b"", [], fs, channels, 0, block, hashlib.md5(b"").digest() if md5 else None)
    digest = None
    if md5:
        # the host hashes the raw PCM: the D2H of the samples the encoder otherwise saves
        digest = hashlib.md5(x16.cpu().contiguous().numpy().astype("<i2", copy=False).tobytes()).digest()
    payload, fbytes = encode_flac_device(x16.to("cuda"), fs, block, lpc_order=lpc_order)
    return flac_container(payload.cpu().numpy().tobytes(), fbytes.cpu().numpy(), fs, channels, frames, block, digest)


def write_flac(path, x16, fs, block=4096, md5=True, lpc_order=0):
    """x16 int16 [frames, channels] (device tensor or numpy array) as a 16-bit FLAC file.
    md5=False leaves STREAMINFO's MD5 zero and moves only the encoded bytes off the device.
    lpc_order 1..8: LPC subframes up to that order (a smaller file, one more kernel); an
    order outside 0..8 raises ValueError and leaves no file."""
    data = flac_bytes(x16, fs, block, md5, lpc_order)
    with open(path, "wb") as f:
        f.write(data)
