"""A strict FLAC reader for the tests (test infrastructure, never imported by amx/).

Written from RFC 9639 alone: it shares no code with csrc/amx_flac.cpp or tests/flac_enc.py
(its own bit reading, table-driven CRC-8 / CRC-16 and coded-number decoding), so that an
encoder's stream has a judge other than the in-tree decoder.  It reads the subset the
device encoder emits (fixed block size, CONSTANT / VERBATIM / FIXED subframes, Rice coding
method 0 without escapes) plus wasted bits, and checks every field on the way; anything
outside the subset raises a rule of its own and is never skipped.

    samples, report = verify(data, profile=False, frames=None, frame_bytes=None)

samples: int64 [n, C].  Raises FlacFormatError(rule, frame, detail) on the first violation;
`rule` is a short stable name (RULES).  profile=True adds the device encoder's own promises
(include/amx.h).  frames: an iterable of frame indices to decode fully; every
other frame gets the header checks and the CRC-8 only and is stepped over by its length,
which the caller then has to pass as frame_bytes (the samples of such frames stay 0 and the
MD5 is not compared).  frame_bytes alone: every frame's length is compared as well.

report: the STREAMINFO fields, "md5_checked", "metadata_blocks" and "frames", one dict per
frame: offset, length, number, number_bytes, header_bytes, block, block_code, rate_code,
size_code, assignment, decoded, and for decoded frames pad_bits and subframes (type, order,
wasted, bits, start_bit, partition_order, po_bit, parameters) with bit positions counted
from the frame's first bit.
"""
import hashlib

import numpy as np

RULES = (
    "stream_marker", "streaminfo_first", "metadata_truncated", "streaminfo_block_range",
    "streaminfo_block_order", "streaminfo_max_block", "streaminfo_min_block",
    "streaminfo_min_frame_size", "streaminfo_max_frame_size", "streaminfo_rate", "streaminfo_bits",
    "streaminfo_total_samples", "streaminfo_md5",
    "frame_truncated", "frame_sync", "frame_reserved", "blocking_strategy_changed", "variable_blocksize",
    "frame_number_coding", "frame_number_overlong", "frame_number_behind", "frame_number_ahead",
    "block_size_reserved", "block_size_extra", "block_size_changed", "block_size_short",
    "rate_code_invalid", "rate_code_mismatch", "rate_extra_mismatch",
    "sample_size_reserved", "sample_size_mismatch",
    "channel_assignment_reserved", "channel_assignment", "header_crc8",
    "subframe_padding", "subframe_type_reserved", "subframe_lpc", "wasted_bits",
    "rice_method_1", "rice_method_reserved", "rice_escape", "partition_order", "sample_range",
    "frame_padding", "frame_crc16", "frame_length", "frame_count", "trailing_bytes",
    "profile_sample_size_code", "profile_wasted_bits", "profile_partition_order", "profile_metadata",
    "profile_rate_code", "profile_block_code",
)


class FlacFormatError(Exception):
    def __init__(self, rule, frame, detail=""):
        assert rule in RULES, rule
        self.rule, self.frame, self.detail = rule, frame, detail
        super().__init__("%s (frame %s): %s" % (rule, frame, detail))


# ------------------------------------------------------------------ CRCs (RFC 9639 9.1.8, 9.3)
def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_T8 = _crc_table(0x07, 8)            # x^8 + x^2 + x + 1
_T16 = _crc_table(0x8005, 16)        # x^16 + x^15 + x^2 + 1


def crc8(b):
    c = 0
    for x in b:
        c = _T8[c ^ x]
    return c


def crc16(b):
    c = 0
    for x in b:
        c = ((c << 8) & 0xFF00) ^ _T16[(c >> 8) ^ x]
    return c


# ------------------------------------------------------------------ header tables (9.1)
_BLOCK_TABLE = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096,
                13: 8192, 14: 16384, 15: 32768}
_RATE_TABLE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100,
               10: 48000, 11: 96000}
_SIZE_TABLE = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
# bytes a coded number takes at the least: below 2^7 one, then 2^11, 2^16, 2^21, 2^26, 2^31
_NUMBER_LIMITS = (1 << 7, 1 << 11, 1 << 16, 1 << 21, 1 << 26, 1 << 31, 1 << 36)


def coded_number(data, pos):
    """(value, bytes) of the coded number at data[pos:] (9.1.5), or None if it is malformed"""
    if pos >= len(data):
        return None
    b0 = data[pos]
    if b0 < 0x80:
        return b0, 1
    nb = 0
    while nb < 8 and b0 & (0x80 >> nb):
        nb += 1
    if nb < 2 or nb > 7 or pos + nb > len(data):
        return None                                   # 10xxxxxx leads nothing, 11111111 is no lead byte
    v = b0 & (0x7F >> nb)
    for i in range(1, nb):
        c = data[pos + i]
        if c & 0xC0 != 0x80:
            return None
        v = (v << 6) | (c & 0x3F)
    return v, nb


def shortest_number_bytes(v):
    for i, lim in enumerate(_NUMBER_LIMITS):
        if v < lim:
            return i + 1
    raise ValueError(v)


def profile_rate_code(fs):
    """the sample-rate code the device encoder's header table implies"""
    for code, rate in _RATE_TABLE.items():
        if rate == fs:
            return code
    if fs < 65536:
        return 13
    if fs % 10 == 0 and fs < 655350:
        return 14
    return 0


def profile_block_code(n):
    for code, size in _BLOCK_TABLE.items():
        if size == n:
            return code
    return 6 if n <= 256 else 7


# ------------------------------------------------------------------ bits of one frame
class _Bits:
    """the bits of data[start:start + limit] as a '0'/'1' string (unary runs are a find)
    and as a numpy array (VERBATIM samples are a reshape)"""

    def __init__(self, data, start, limit):
        raw = np.frombuffer(data, np.uint8, count=min(limit, len(data) - start), offset=start)
        self.arr = np.unpackbits(raw)
        self.s = (self.arr + 48).tobytes().decode("ascii")
        self.n = len(self.s)
        self.pos = 0

    def need(self, k, frame):
        if self.pos + k > self.n:
            raise FlacFormatError("frame_truncated", frame, "the frame runs past the bytes there are")

    def u(self, k, frame):
        if k == 0:
            return 0
        self.need(k, frame)
        v = int(self.s[self.pos:self.pos + k], 2)
        self.pos += k
        return v

    def i(self, k, frame):
        v = self.u(k, frame)
        return v - (1 << k) if k and v >> (k - 1) else v

    def unary(self, frame):
        e = self.s.find("1", self.pos)
        if e < 0:
            raise FlacFormatError("frame_truncated", frame, "a unary run without its stop bit")
        q = e - self.pos
        self.pos = e + 1
        return q

    def signed_block(self, n, w, frame):
        self.need(n * w, frame)
        b = self.arr[self.pos:self.pos + n * w].reshape(n, w).astype(np.int64)
        self.pos += n * w
        v = b @ (np.int64(1) << np.arange(w - 1, -1, -1, dtype=np.int64))
        return v - (b[:, 0] << w)


# ------------------------------------------------------------------ metadata (8)
def _metadata(data, profile):
    if len(data) < 4 or bytes(data[:4]) != b"fLaC":
        raise FlacFormatError("stream_marker", None, "the stream does not start with fLaC")
    pos, blocks, info = 4, 0, None
    while True:
        if pos + 4 > len(data):
            raise FlacFormatError("metadata_truncated", None, "no metadata block header at %d" % pos)
        last, kind = data[pos] >> 7, data[pos] & 0x7F
        length = int.from_bytes(data[pos + 1:pos + 4], "big")
        if blocks == 0 and (kind != 0 or length != 34):
            raise FlacFormatError("streaminfo_first", None, "first block has type %d, length %d" % (kind, length))
        if pos + 4 + length > len(data):
            raise FlacFormatError("metadata_truncated", None, "block %d runs past the stream" % blocks)
        if blocks == 0:
            v = int.from_bytes(data[pos + 4:pos + 22], "big")
            info = dict(min_block=v >> 128, max_block=(v >> 112) & 0xFFFF, min_frame=(v >> 88) & 0xFFFFFF,
                        max_frame=(v >> 64) & 0xFFFFFF, sample_rate=(v >> 44) & 0xFFFFF,
                        channels=((v >> 41) & 7) + 1, bits=((v >> 36) & 31) + 1,
                        total_samples=v & ((1 << 36) - 1), md5=bytes(data[pos + 22:pos + 38]))
        blocks += 1
        pos += 4 + length
        if last:
            break
    info["metadata_blocks"] = blocks
    lo, hi = info["min_block"], info["max_block"]
    if not (16 <= lo <= 65535 and 16 <= hi <= 65535):
        raise FlacFormatError("streaminfo_block_range", None, "block sizes %d, %d outside 16..65535" % (lo, hi))
    if lo > hi:
        raise FlacFormatError("streaminfo_block_order", None, "minimum block %d above the maximum %d" % (lo, hi))
    if info["sample_rate"] == 0:
        raise FlacFormatError("streaminfo_rate", None, "sample rate 0")
    if info["bits"] < 4:
        raise FlacFormatError("streaminfo_bits", None, "%d bits per sample" % info["bits"])
    if profile and blocks != 1:
        raise FlacFormatError("profile_metadata", None, "%d metadata blocks" % blocks)
    return info, pos


# ------------------------------------------------------------------ frame header (9.1)
def _header(data, off, k, info, state, profile):
    """the checked header of frame k at byte off: a dict with header_bytes (CRC-8 included)"""
    if off + 6 > len(data):
        raise FlacFormatError("frame_truncated", k, "%d bytes left at %d" % (len(data) - off, off))
    b1, b2, b3 = data[off + 1], data[off + 2], data[off + 3]
    if data[off] != 0xFF or b1 & 0xFC != 0xF8:
        raise FlacFormatError("frame_sync", k, "no sync code at byte %d" % off)
    bcode, rcode = b2 >> 4, b2 & 15
    if bcode == 0:
        raise FlacFormatError("block_size_reserved", k, "block-size code 0")
    if rcode == 15:
        raise FlacFormatError("rate_code_invalid", k, "sample-rate code 15")
    num = coded_number(data, off + 4)
    if num is None:
        raise FlacFormatError("frame_number_coding", k, "malformed coded number")
    number, nbytes = num
    p = off + 4 + nbytes
    bx = 1 if bcode == 6 else 2 if bcode == 7 else 0
    rx = 1 if rcode == 12 else 2 if rcode in (13, 14) else 0
    if p + bx + rx + 1 > len(data):
        raise FlacFormatError("frame_truncated", k, "the header runs past the stream")
    bextra = int.from_bytes(data[p:p + bx], "big")
    rextra = int.from_bytes(data[p + bx:p + bx + rx], "big")
    p += bx + rx
    if crc8(data[off:p]) != data[p]:
        raise FlacFormatError("header_crc8", k, "CRC-8 %02x, the header gives %02x" % (data[p], crc8(data[off:p])))
    # ---- the fields' meaning
    if b1 & 2 or b3 & 1:
        raise FlacFormatError("frame_reserved", k, "a reserved header bit is set")
    strategy = b1 & 1
    if state.setdefault("strategy", strategy) != strategy:
        raise FlacFormatError("blocking_strategy_changed", k, "blocking strategy %d after %d"
                              % (strategy, state["strategy"]))
    if strategy:
        raise FlacFormatError("variable_blocksize", k, "variable-blocksize streams are outside the subset")
    if number != k:
        raise FlacFormatError("frame_number_behind" if number < k else "frame_number_ahead", k,
                              "coded frame number %d" % number)
    if nbytes != shortest_number_bytes(number):
        raise FlacFormatError("frame_number_overlong", k, "%d coded in %d bytes" % (number, nbytes))
    block = _BLOCK_TABLE[bcode] if bcode in _BLOCK_TABLE else bextra + 1
    if block > 65535:
        raise FlacFormatError("block_size_extra", k, "block size %d" % block)
    if rcode in (12, 13, 14):
        rate = rextra * (1000 if rcode == 12 else 1 if rcode == 13 else 10)
        if rate != info["sample_rate"]:
            raise FlacFormatError("rate_extra_mismatch", k, "code %d says %d Hz, STREAMINFO %d"
                                  % (rcode, rate, info["sample_rate"]))
    elif rcode and _RATE_TABLE[rcode] != info["sample_rate"]:
        raise FlacFormatError("rate_code_mismatch", k, "code %d says %d Hz, STREAMINFO %d"
                              % (rcode, _RATE_TABLE[rcode], info["sample_rate"]))
    scode = (b3 >> 1) & 7
    if scode == 3:
        raise FlacFormatError("sample_size_reserved", k, "sample-size code 3")
    if scode and _SIZE_TABLE[scode] != info["bits"]:
        raise FlacFormatError("sample_size_mismatch", k, "code %d says %d bits, STREAMINFO %d"
                              % (scode, _SIZE_TABLE[scode], info["bits"]))
    assign = b3 >> 4
    if assign > 10:
        raise FlacFormatError("channel_assignment_reserved", k, "channel assignment %d" % assign)
    if (2 if assign >= 8 else assign + 1) != info["channels"]:
        raise FlacFormatError("channel_assignment", k, "assignment %d in a %d-channel stream"
                              % (assign, info["channels"]))
    if block > info["max_block"]:
        raise FlacFormatError("streaminfo_max_block", k, "block %d above STREAMINFO's %d" % (block, info["max_block"]))
    if profile:
        if scode != 4:
            raise FlacFormatError("profile_sample_size_code", k, "sample-size code %d" % scode)
        if rcode != profile_rate_code(info["sample_rate"]):
            raise FlacFormatError("profile_rate_code", k, "rate code %d for %d Hz, the table implies %d"
                                  % (rcode, info["sample_rate"], profile_rate_code(info["sample_rate"])))
        if bcode != profile_block_code(block):
            raise FlacFormatError("profile_block_code", k, "block code %d for %d samples" % (bcode, block))
    return dict(offset=off, number=number, number_bytes=nbytes, header_bytes=p + 1 - off, block=block,
                block_code=bcode, rate_code=rcode, size_code=scode, assignment=assign, decoded=False)


def _not_last(fr, k, info, state):
    """what holds for every frame but the last, checked once a next frame is known to follow"""
    if fr["block"] < 16:
        raise FlacFormatError("block_size_short", k, "%d samples in a frame that is not the last" % fr["block"])
    if fr["block"] != state["block"]:
        raise FlacFormatError("block_size_changed", k, "%d samples after frames of %d" % (fr["block"], state["block"]))
    if fr["block"] < info["min_block"]:
        raise FlacFormatError("streaminfo_min_block", k, "block %d below STREAMINFO's %d"
                              % (fr["block"], info["min_block"]))


# ------------------------------------------------------------------ subframes (9.2)
def _residual(br, k, block, order, profile, sub):
    method = br.u(2, k)
    if method == 1:
        raise FlacFormatError("rice_method_1", k, "5-bit Rice parameters are outside the subset")
    if method > 1:
        raise FlacFormatError("rice_method_reserved", k, "residual coding method %d" % method)
    sub["po_bit"] = br.pos
    po = br.u(4, k)
    sub["partition_order"] = po
    if block % (1 << po) or (block >> po) < order:
        raise FlacFormatError("partition_order", k, "partition order %d, block %d, predictor order %d"
                              % (po, block, order))
    if profile and po > 6:
        raise FlacFormatError("profile_partition_order", k, "partition order %d" % po)
    res, params = [], []
    s, find = br.s, br.s.find
    for part in range(1 << po):
        par = br.u(4, k)
        if par == 15:
            raise FlacFormatError("rice_escape", k, "an escaped partition is outside the subset")
        params.append(par)
        pos = br.pos
        for _ in range((block >> po) - (order if part == 0 else 0)):
            e = find("1", pos)
            if e < 0 or e + 1 + par > br.n:
                raise FlacFormatError("frame_truncated", k, "a residual runs past the bytes there are")
            u = e - pos
            pos = e + 1
            if par:
                u = (u << par) | int(s[pos:pos + par], 2)
                pos += par
            res.append(-((u + 1) >> 1) if u & 1 else u >> 1)
        br.pos = pos
    sub["parameters"] = params
    return res


def _subframe(br, k, block, w, profile):
    sub = dict(start_bit=br.pos)
    if br.u(1, k):
        raise FlacFormatError("subframe_padding", k, "the subframe's first bit is set")
    t = br.u(6, k)
    wasted = 0
    if br.u(1, k):
        wasted = br.unary(k) + 1
        if profile:
            raise FlacFormatError("profile_wasted_bits", k, "%d wasted bits" % wasted)
        if wasted >= w:
            raise FlacFormatError("wasted_bits", k, "%d wasted bits of %d" % (wasted, w))
    ew = w - wasted
    sub.update(type=t, wasted=wasted, order=0)
    if t == 0:
        x = np.full(block, br.i(ew, k), np.int64)
    elif t == 1:
        x = br.signed_block(block, ew, k)
    elif 8 <= t <= 12:
        order = t - 8
        sub["order"] = order
        if order > block:
            raise FlacFormatError("partition_order", k, "predictor order %d in a block of %d" % (order, block))
        v = [br.i(ew, k) for _ in range(order)]
        res = _residual(br, k, block, order, profile, sub)
        # 9.2.5: the predictions 0, a, 2a - b, 3a - 3b + c, 4a - 6b + 4c - d
        if order == 0:
            v = res
        elif order == 1:
            for r in res:
                v.append(r + v[-1])
        elif order == 2:
            for r in res:
                v.append(r + 2 * v[-1] - v[-2])
        elif order == 3:
            for r in res:
                v.append(r + 3 * v[-1] - 3 * v[-2] + v[-3])
        else:
            for r in res:
                v.append(r + 4 * v[-1] - 6 * v[-2] + 4 * v[-3] - v[-4])
        lim = 1 << 62
        if any(not -lim <= s < lim for s in v):
            raise FlacFormatError("sample_range", k, "a decoded sample does not fit %d bits" % ew)
        x = np.asarray(v, np.int64)
    elif t >= 32:
        raise FlacFormatError("subframe_lpc", k, "an LPC subframe (order %d) is outside the subset" % (t - 31))
    else:
        raise FlacFormatError("subframe_type_reserved", k, "subframe type %d" % t)
    if len(x) and (x.min() < -(1 << (ew - 1)) or x.max() >= 1 << (ew - 1)):
        raise FlacFormatError("sample_range", k, "a decoded sample does not fit %d bits" % ew)
    sub["bits"] = br.pos - sub["start_bit"]
    return x << wasted, sub


def _frame_body(data, fr, k, info, limit, profile):
    """decode frame k's subframes, padding and CRC-16: (samples [block, C], length in bytes)"""
    C, bits, block, assign = info["channels"], info["bits"], fr["block"], fr["assignment"]
    br = _Bits(data, fr["offset"], limit)
    br.pos = 8 * fr["header_bytes"]
    chans, subs = [], []
    for c in range(C):
        side = assign == 8 and c == 1 or assign == 9 and c == 0 or assign == 10 and c == 1
        x, sub = _subframe(br, k, block, bits + 1 if side else bits, profile)
        chans.append(x)
        subs.append(sub)
    if assign == 8:
        chans[1] = chans[0] - chans[1]
    elif assign == 9:
        chans[0] = chans[0] + chans[1]
    elif assign == 10:
        mid = (chans[0] << 1) | (chans[1] & 1)
        chans = [(mid + chans[1]) >> 1, (mid - chans[1]) >> 1]
    out = np.stack(chans, axis=1)
    if assign >= 8 and (out.min() < -(1 << (bits - 1)) or out.max() >= 1 << (bits - 1)):
        raise FlacFormatError("sample_range", k, "a stereo sample does not fit %d bits" % bits)
    pad = -br.pos % 8
    if br.u(pad, k):
        raise FlacFormatError("frame_padding", k, "non-zero bits before the CRC-16")
    nbody = br.pos // 8
    br.need(16, k)
    off = fr["offset"]
    want, got = crc16(data[off:off + nbody]), int.from_bytes(data[off + nbody:off + nbody + 2], "big")
    if want != got:
        raise FlacFormatError("frame_crc16", k, "CRC-16 %04x, the frame gives %04x" % (got, want))
    fr.update(decoded=True, pad_bits=pad, subframes=subs)
    return out, nbody + 2


# ------------------------------------------------------------------ the stream
def verify(data, *, profile=False, frames=None, frame_bytes=None):
    data = bytes(data)
    info, off = _metadata(data, profile)
    C = info["channels"]
    full = None if frames is None else set(int(f) for f in frames)
    lengths = None if frame_bytes is None else [int(v) for v in np.asarray(frame_bytes).reshape(-1)]
    if full is not None and lengths is None:
        raise ValueError("verify(frames=...) needs frame_bytes to step over the other frames")
    state, recs, blocks, prev, k, held = {}, [], [], None, 0, 0
    while off < len(data):
        if k and held == info["total_samples"]:
            raise FlacFormatError("trailing_bytes", k, "%d bytes after the frame that completes STREAMINFO's %d "
                                  "samples" % (len(data) - off, held))
        if lengths is not None and k >= len(lengths):
            raise FlacFormatError("frame_count", k, "bytes left after the %d frames given" % len(lengths))
        fr = _header(data, off, k, info, state, profile)
        state.setdefault("block", fr["block"])
        if prev is not None:
            _not_last(prev, k - 1, info, state)
        if fr["block"] > state["block"]:
            raise FlacFormatError("block_size_changed", k, "%d samples after frames of %d"
                                  % (fr["block"], state["block"]))
        if full is None or k in full:
            # the bits to unpack: the length given, else STREAMINFO's largest frame as a first
            # guess (a frame that outgrows the guess is read again from all that is left)
            limit = lengths[k] if lengths is not None else info["max_frame"] or len(data) - off
            try:
                x, n = _frame_body(data, fr, k, info, max(limit, fr["header_bytes"]), profile)
            except FlacFormatError as e:
                if e.rule != "frame_truncated" or lengths is not None or limit >= len(data) - off:
                    raise
                x, n = _frame_body(data, fr, k, info, len(data) - off, profile)
            if lengths is not None and n != lengths[k]:
                raise FlacFormatError("frame_length", k, "%d bytes, %d given" % (n, lengths[k]))
            blocks.append(x)
        else:
            n = lengths[k]
            if n < fr["header_bytes"] + 2 or off + n > len(data):
                raise FlacFormatError("frame_length", k, "%d bytes given at %d of %d" % (n, off, len(data)))
            blocks.append(fr["block"])
        fr["length"] = n
        held += fr["block"]
        recs.append(fr)
        prev = fr
        off += n
        k += 1
    if lengths is not None and k != len(lengths):
        raise FlacFormatError("frame_count", k, "%d frames, %d lengths given" % (k, len(lengths)))
    # ---- STREAMINFO against what the frames held
    sizes = [fr["length"] for fr in recs]
    total = sum(fr["block"] for fr in recs)
    if info["total_samples"] != total:
        raise FlacFormatError("streaminfo_total_samples", None, "STREAMINFO says %d samples, the frames hold %d"
                              % (info["total_samples"], total))
    if info["min_frame"] and sizes and info["min_frame"] != min(sizes):
        raise FlacFormatError("streaminfo_min_frame_size", None, "STREAMINFO says %d, the smallest frame is %d"
                              % (info["min_frame"], min(sizes)))
    if info["max_frame"] and sizes and info["max_frame"] != max(sizes):
        raise FlacFormatError("streaminfo_max_frame_size", None, "STREAMINFO says %d, the largest frame is %d"
                              % (info["max_frame"], max(sizes)))
    out = np.zeros((total, C), np.int64)
    at = 0
    for x in blocks:
        if isinstance(x, int):
            at += x
        else:
            out[at:at + len(x)] = x
            at += len(x)
    md5_checked = False
    if full is None and info["md5"] != bytes(16):
        nb = (info["bits"] + 7) // 8
        raw = out.astype("<i8").view(np.uint8).reshape(-1, 8)[:, :nb].tobytes()   # little-endian, nb bytes each
        if hashlib.md5(raw).digest() != info["md5"]:
            raise FlacFormatError("streaminfo_md5", None, "the MD5 of the decoded samples differs from STREAMINFO's")
        md5_checked = True
    report = dict(info, md5_checked=md5_checked, n_frames=len(recs), frames=recs)
    return out, report
