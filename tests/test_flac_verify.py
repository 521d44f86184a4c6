"""CPU: tests/flac_verify.py, the strict RFC 9639 reader the device encoder's streams are
held to (tests/test_gpu_flac_encode.py), checked without a GPU.

Agreement: streams of the test-side encoder (tests/flac_enc.py, restricted to CONSTANT,
VERBATIM and FIXED subframes) must read back exactly, and amx.flacio.decode_flac must agree
where the library loads.  flac_enc picks Rice coding method 1 (30 % of the residuals), an
escaped partition (8 % of the partitions) and, for a "constant" draw on samples that are not
constant, an LPC subframe at random; the reader refuses all three by name.  So every case
walks the seeds from 0: a stream the reader refuses must be refused with one of those three
rules (anything else fails the test), and the first stream it accepts must equal the input
and show the features the case is about.  Cases are kept to a few subframes so that a seed
is found soon.

It must notice: one valid stream, one mutation at a time, the CRC-8 and CRC-16 recomputed
(with flac_enc's bitwise CRCs, not the reader's tables) wherever the mutation sits under
them, and every mutation must raise its own rule.

Container: amx.flacio.flac_container's 42 bytes in front of one short frame.
"""
import hashlib

import numpy as np
import pytest

import flac_enc
import flac_verify as fv

OUTSIDE = {"subframe_lpc", "rice_method_1", "rice_escape"}
FIXED = ["fixed0", "fixed1", "fixed2", "fixed3", "fixed4"]
SEEDS = 3000


def _accepted(x, fs, block, kinds, assigns=None, want=None, metadata=True):
    """(stream, report) of the first seed whose flac_enc stream the reader accepts (and for
    which want(report) holds); the refused ones must carry a rule of OUTSIDE"""
    for seed in range(SEEDS):
        data = flac_enc.encode(x, fs, 16, seed=seed, block=block, kinds=kinds, assigns=assigns, metadata=metadata)
        try:
            got, rep = fv.verify(data)
        except fv.FlacFormatError as e:
            assert e.rule in OUTSIDE, (seed, str(e))
            continue
        np.testing.assert_array_equal(got, x)
        if want is None or want(rep):
            return data, rep
    raise AssertionError("no seed below %d gives a stream inside the subset" % SEEDS)


def _signal(n, C, seed, full_scale=False):
    """random walks of small steps: every FIXED order's residual stays below 2^13, where
    flac_enc would turn to coding method 1 for good; full_scale: the 16-bit extremes in the
    last samples (for VERBATIM-only streams)"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(-20, 21, (n, C)), axis=0).astype(np.int64) + rng.integers(-500, 500, C)
    if full_scale:
        x[-2], x[-1] = 32767, -32768
        x[-2:, -1] = -32768, 32767
    return x


def _types(rep):
    return [s["type"] for f in rep["frames"] for s in f["subframes"]]


def _agrees_with_the_library(data, x):
    try:
        from amx import capi, flacio
        capi.load()
    except Exception:   # noqa: BLE001 -- no library here: the reader alone is judged
        return
    got, _ = flacio.decode_flac(data)
    np.testing.assert_array_equal(got, (x << 16).astype(np.int32))


# ------------------------------------------------------------------ agreement
# (channels, assignment, block, samples, rate, kinds): every stereo assignment, mono, 3 and
# 8 channels; blocks 16, 192, 1000, 1152, 4096 with a short last frame (and 16 with a last
# frame below 16); the six rates (a table rate, Hz, tens of Hz, and one only STREAMINFO holds)
AGREE = [
    (2, 0, 192, 192 + 50, 8000, ["verbatim", "fixed1", "fixed2"]),
    (2, 8, 192, 192 + 50, 11025, ["verbatim", "fixed2", "fixed3"]),
    (2, 9, 1000, 1000 + 17, 44100, ["verbatim", "fixed0", "fixed4"]),
    (2, 10, 16, 3 * 16 + 5, 96000, ["verbatim", "fixed1", "fixed4"]),
    (1, None, 4096, 4096 + 700, 352800, FIXED),
    (1, None, 1152, 2 * 1152 + 16, 768000, FIXED),
    (1, None, 1000, 2 * 1000 + 1, 11025, ["verbatim", "fixed3"]),
    (1, None, 16, 6 * 16 + 3, 8000, FIXED),
    (3, None, 192, 192 + 16, 44100, ["verbatim", "fixed2"]),
    (8, None, 16, 16 + 7, 96000, ["verbatim", "fixed1"]),
]


@pytest.mark.parametrize("C,assign,block,n,fs,kinds", AGREE)
def test_reads_flac_enc_streams(C, assign, block, n, fs, kinds):
    x = _signal(n, C, seed=C * 7 + block)
    # at least one FIXED subframe, so the residual reading is part of every case
    data, rep = _accepted(x, fs, block, kinds, None if assign is None else [assign],
                          want=lambda r: any(t >= 8 for t in _types(r)))
    assert (rep["sample_rate"], rep["channels"], rep["bits"], rep["total_samples"]) == (fs, C, 16, n)
    assert [f["block"] for f in rep["frames"]] == [min(block, n - s) for s in range(0, n, block)]
    assert [f["number"] for f in rep["frames"]] == list(range(len(rep["frames"])))
    if assign is not None:
        assert all(f["assignment"] == (1 if assign == 0 else assign) for f in rep["frames"])
    assert rep["metadata_blocks"] == 3 and not rep["md5_checked"]
    _agrees_with_the_library(data, x)


@pytest.mark.parametrize("assign", [0, 8, 9, 10])
def test_reads_full_scale_verbatim(assign):
    """the 16-bit extremes, opposite in the two channels: the side channel's 17 bits"""
    x = _signal(192 + 30, 2, seed=assign, full_scale=True)
    data, rep = _accepted(x, 48000, 192, ["verbatim"], [assign])
    assert set(_types(rep)) == {1} and x.max() == 32767 and x.min() == -32768
    _agrees_with_the_library(data, x)


@pytest.mark.parametrize("order", range(5))
def test_reads_every_fixed_order(order):
    """only FIXED(order) subframes"""
    x = _signal(2 * 192 + 40, 1, seed=order)
    data, rep = _accepted(x, 48000, 192, ["fixed%d" % order])
    assert set(_types(rep)) == {8 + order}
    _agrees_with_the_library(data, x)


def test_reads_constant_and_wasted_bits():
    """constant channels (CONSTANT subframes) and samples with trailing zero bits (flac_enc
    turns them into wasted bits for 30 % of the subframes)"""
    n = 2 * 192 + 20
    x = _signal(n, 2, seed=3) * 8
    x[:, 1] = -1234
    data, rep = _accepted(x, 44100, 192, ["constant", "verbatim", "fixed2"], [0],
                          want=lambda r: 0 in _types(r) and any(s["wasted"] for f in r["frames"]
                                                                for s in f["subframes"]))
    _agrees_with_the_library(data, x)
    with pytest.raises(fv.FlacFormatError) as e:
        fv.verify(data, profile=True)            # three metadata blocks, wasted bits, free header codes
    assert e.value.rule.startswith("profile_")


@pytest.mark.parametrize("kinds,rule", [(["lpc"], "subframe_lpc"), (["constant"], "subframe_lpc")])
def test_names_what_is_outside_the_subset(kinds, rule):
    x = _signal(192, 1, seed=1)
    with pytest.raises(fv.FlacFormatError) as e:
        fv.verify(flac_enc.encode(x, 48000, 16, seed=0, block=192, kinds=kinds))
    assert e.value.rule == rule


def test_names_method_1_escapes_and_variable_blocksize():
    x = _signal(4 * 192, 1, seed=2)
    seen = set()
    for seed in range(200):
        try:
            fv.verify(flac_enc.encode(x, 48000, 16, seed=seed, block=192, kinds=["fixed2"]))
        except fv.FlacFormatError as e:
            seen.add(e.rule)
    assert seen == {"rice_method_1", "rice_escape"}
    with pytest.raises(fv.FlacFormatError) as e:
        fv.verify(flac_enc.encode(x, 48000, 16, seed=0, block=192, kinds=["verbatim"], variable=True))
    assert e.value.rule == "variable_blocksize"


def test_partial_mode_steps_by_the_given_lengths():
    x = _signal(5 * 192 + 40, 2, seed=4)
    data, rep = _accepted(x, 44100, 192, ["verbatim", "fixed2"])
    fb = [f["length"] for f in rep["frames"]]
    got, part = fv.verify(data, frames=[1, 5], frame_bytes=fb)
    assert [f["decoded"] for f in part["frames"]] == [False, True, False, False, False, True]
    np.testing.assert_array_equal(got[192:384], x[192:384])
    np.testing.assert_array_equal(got[960:], x[960:])
    assert not got[:192].any() and not got[384:960].any()
    assert [f["number"] for f in part["frames"]] == list(range(6))
    np.testing.assert_array_equal(fv.verify(data, frame_bytes=fb)[0], x)
    for bad, rule in ((fb[:-1], "frame_count"), (fb + [12], "frame_count"),
                      ([fb[0] + 1] + fb[1:], "frame_length")):
        with pytest.raises(fv.FlacFormatError) as e:
            fv.verify(data, frame_bytes=bad)
        assert e.value.rule == rule
    with pytest.raises(fv.FlacFormatError) as e:
        fv.verify(data, frames=[5], frame_bytes=[fb[0] + 1] + fb[1:])
    assert e.value.rule == "frame_sync"           # the hop lands beside the next frame


def test_crcs_and_coded_numbers_against_flac_enc():
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 300):
        b = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        assert fv.crc8(b) == flac_enc.crc8(b) and fv.crc16(b) == flac_enc.crc16(b)
    for v in (0, 127, 128, 2047, 2048, 65535, 65536, (1 << 21) - 1, 1 << 21, (1 << 26) - 1, 1 << 26,
              (1 << 31) - 1, 1 << 31, (1 << 36) - 1):
        b = flac_enc._utf8(v)
        assert fv.coded_number(b, 0) == (v, len(b)) and fv.shortest_number_bytes(v) == len(b)
    for bad in (b"\x80", b"\xff", b"\xc2", b"\xc2\x00", b"\xe0\x80\xc0"):
        assert fv.coded_number(bad, 0) is None


# ------------------------------------------------------------------ it must notice
FS, BLOCK = 44100, 192


@pytest.fixture(scope="module")
def base():
    """(stream, report, samples): stereo, five frames of 192 and one of 40, STREAMINFO alone
    in front and a true MD5; some frame ends off a byte boundary, some subframe is FIXED(4)
    and some is VERBATIM -- the places the mutations below need"""
    x = _signal(5 * BLOCK + 40, 2, seed=11)

    def fit(rep):
        subs = [s for f in rep["frames"][1:-1] for s in f["subframes"]]
        return (any(f["pad_bits"] for f in rep["frames"]) and any(s["type"] == 12 for s in subs)
                and any(s["type"] == 1 for s in subs))

    data, rep = _accepted(x, FS, BLOCK, ["verbatim", "fixed4"], want=fit, metadata=False)
    data = data[:26] + hashlib.md5(x.astype("<i2").tobytes()).digest() + data[42:]
    got, rep = fv.verify(data)
    np.testing.assert_array_equal(got, x)
    assert rep["md5_checked"] and rep["metadata_blocks"] == 1 and rep["frames"][0]["offset"] == 42
    return data, rep, x


def _header_fields(frame, fr):
    nb, hb = fr["number_bytes"], fr["header_bytes"]
    bx = {6: 1, 7: 2}.get(fr["block_code"], 0)
    return dict(strategy=frame[1] & 1, reserved1=(frame[1] >> 1) & 1, bcode=frame[2] >> 4, rcode=frame[2] & 15,
                assign=frame[3] >> 4, scode=(frame[3] >> 1) & 7, reserved2=frame[3] & 1,
                number=bytes(frame[4:4 + nb]), bextra=bytes(frame[4 + nb:4 + nb + bx]),
                rextra=bytes(frame[4 + nb + bx:hb - 1]))


def _reheaded(data, rep, k, **changes):
    """the stream with frame k's header rebuilt from its fields and `changes`, CRC-8 and
    CRC-16 recomputed"""
    fr = rep["frames"][k]
    frame = data[fr["offset"]:fr["offset"] + fr["length"]]
    h = dict(_header_fields(frame, fr), **changes)
    head = bytes([0xFF, 0xF8 | h["reserved1"] << 1 | h["strategy"], h["bcode"] << 4 | h["rcode"],
                  h["assign"] << 4 | h["scode"] << 1 | h["reserved2"]]) + h["number"] + h["bextra"] + h["rextra"]
    body = head + bytes([flac_enc.crc8(head)]) + frame[fr["header_bytes"]:-2]
    return data[:fr["offset"]] + body + flac_enc.crc16(body).to_bytes(2, "big") + data[fr["offset"] + fr["length"]:]


def _bit_changed(data, rep, k, bit, value=None, width=1, recrc=True):
    """the stream with `width` bits at bit `bit` of frame k set to `value` (None: flipped);
    recrc: the frame's CRC-16 recomputed"""
    fr = rep["frames"][k]
    frame = data[fr["offset"]:fr["offset"] + fr["length"]]
    v = int.from_bytes(frame, "big")
    sh = 8 * len(frame) - bit - width
    mask = ((1 << width) - 1) << sh
    v = v ^ mask if value is None else (v & ~mask) | (value << sh)
    frame = v.to_bytes(len(frame), "big")
    if recrc:
        frame = frame[:-2] + flac_enc.crc16(frame[:-2]).to_bytes(2, "big")
    return data[:fr["offset"]] + frame + data[fr["offset"] + fr["length"]:]


def _streaminfo_changed(data, shift, bits, value):
    """the stream with the `bits`-bit STREAMINFO field `shift` bits above the MD5 set to value"""
    v = int.from_bytes(data[8:26], "big")
    v = (v & ~(((1 << bits) - 1) << shift)) | (value << shift)
    return data[:8] + v.to_bytes(18, "big") + data[26:]


def _find(rep, pred):
    """(frame index, subframe) of the first subframe of frames 1..4 (192 samples each) for
    which pred holds"""
    return next((k, s) for k, f in enumerate(rep["frames"][:-1]) if k for s in f["subframes"] if pred(s))


def _mutations(data, rep):
    rate_hz = dict(rcode=13, rextra=(FS + 1).to_bytes(2, "big"))
    m = {}
    m["frame number repeated"] = (_reheaded(data, rep, 2, number=b"\x01"), "frame_number_behind", 2)
    m["frame number skipped"] = (_reheaded(data, rep, 2, number=b"\x03"), "frame_number_ahead", 2)
    m["two-byte coding of 2"] = (_reheaded(data, rep, 2, number=b"\xc0\x82"), "frame_number_overlong", 2)
    m["rate extra bytes off by one"] = (_reheaded(data, rep, 1, **rate_hz), "rate_extra_mismatch", 1)
    m["rate code of 48 kHz"] = (_reheaded(data, rep, 1, rcode=10, rextra=b""), "rate_code_mismatch", 1)
    m["sample-size code 1"] = (_reheaded(data, rep, 3, scode=1), "sample_size_mismatch", 3)
    m["blocking strategy set in one frame"] = (_reheaded(data, rep, 1, strategy=1), "blocking_strategy_changed", 1)
    m["reserved bit after the sync code"] = (_reheaded(data, rep, 2, reserved1=1), "frame_reserved", 2)
    m["reserved bit after the sample size"] = (_reheaded(data, rep, 2, reserved2=1), "frame_reserved", 2)
    k = 1
    m["subframe padding bit"] = (_bit_changed(data, rep, k, rep["frames"][k]["subframes"][1]["start_bit"], 1),
                                 "subframe_padding", k)
    k = next(i for i, f in enumerate(rep["frames"]) if f["pad_bits"])
    m["alignment padding"] = (_bit_changed(data, rep, k, 8 * (rep["frames"][k]["length"] - 2) - 1, 1),
                              "frame_padding", k)
    m["STREAMINFO max block 15"] = (_streaminfo_changed(data, 112, 16, 15), "streaminfo_block_range", None)
    m["STREAMINFO min above max"] = (_streaminfo_changed(data, 128, 16, BLOCK + 1), "streaminfo_block_order", None)
    m["STREAMINFO min above the frames"] = (_streaminfo_changed(_streaminfo_changed(data, 128, 16, BLOCK + 1),
                                                                 112, 16, BLOCK + 1), "streaminfo_min_block", 0)
    m["STREAMINFO max below the frames"] = (_streaminfo_changed(_streaminfo_changed(data, 128, 16, BLOCK - 1),
                                                                 112, 16, BLOCK - 1), "streaminfo_max_block", 0)
    m["total samples + 1"] = (_streaminfo_changed(data, 0, 36, rep["total_samples"] + 1),
                              "streaminfo_total_samples", None)
    m["one MD5 byte flipped"] = (data[:30] + bytes([data[30] ^ 0x10]) + data[31:], "streaminfo_md5", None)
    m["max frame size - 1"] = (_streaminfo_changed(data, 64, 24, rep["max_frame"] - 1),
                               "streaminfo_max_frame_size", None)
    m["min frame size + 1"] = (_streaminfo_changed(data, 88, 24, rep["min_frame"] + 1),
                               "streaminfo_min_frame_size", None)
    # 192 >> 6 = 3 samples in the first partition, below the four warm-up samples of FIXED(4)
    k, s = _find(rep, lambda s: s["type"] == 12)
    m["partition order 6 under FIXED(4)"] = (_bit_changed(data, rep, k, s["po_bit"], 6, 4), "partition_order", k)
    # 192 is no multiple of 128
    m["partition order 7"] = (_bit_changed(data, rep, k, s["po_bit"], 7, 4), "partition_order", k)
    m["coding method 1"] = (_bit_changed(data, rep, k, s["po_bit"] - 2, 1, 2), "rice_method_1", k)
    m["one trailing byte"] = (data + b"\x00", "trailing_bytes", len(rep["frames"]))
    m["a frame missing"] = (data[:rep["frames"][-1]["offset"]], "streaminfo_total_samples", None)
    m["a short frame in the middle"] = (data[:rep["frames"][1]["offset"]] + _renumbered_tail(data, rep),
                                        "block_size_changed", 1)
    m["stereo assignment in a mono stream"] = (_streaminfo_changed(data, 41, 3, 0), "channel_assignment", 0)
    m["sample-size code 3"] = (_reheaded(data, rep, 1, scode=3), "sample_size_reserved", 1)
    m["channel assignment 11"] = (_reheaded(data, rep, 1, assign=11), "channel_assignment_reserved", 1)
    # no CRC recomputed: the CRCs are what notices
    assert rep["frames"][1]["number_bytes"] == 1            # byte 4 of frame 1 is its number
    m["a frame-number bit, CRC-8 as it was"] = (_bit_changed(data, rep, 1, 8 * 4 + 7, recrc=False), "header_crc8", 1)
    k, s = _find(rep, lambda s: s["type"] == 1)
    m["a VERBATIM sample's low bit, CRC-16 as it was"] = (
        _bit_changed(data, rep, k, s["start_bit"] + s["bits"] - 1, recrc=False), "frame_crc16", k)
    m["a CRC-16 bit"] = (_bit_changed(data, rep, 4, 8 * rep["frames"][4]["length"] - 3, recrc=False),
                         "frame_crc16", 4)
    return m


def _renumbered_tail(data, rep):
    """the last (short) frame as frame 1, followed by frame 2 on: a 40-sample frame that is
    not the last"""
    last = rep["frames"][-1]
    moved = _reheaded(data, rep, len(rep["frames"]) - 1, number=b"\x01")[last["offset"]:]
    out = moved
    for k in range(1, len(rep["frames"]) - 1):
        fr = rep["frames"][k]
        out += _reheaded(data, rep, k, number=bytes([k + 1]))[fr["offset"]:fr["offset"] + fr["length"]]
    return out


MUTATIONS = [
    "frame number repeated", "frame number skipped", "two-byte coding of 2", "rate extra bytes off by one",
    "rate code of 48 kHz", "sample-size code 1", "blocking strategy set in one frame",
    "reserved bit after the sync code", "reserved bit after the sample size", "subframe padding bit",
    "alignment padding", "STREAMINFO max block 15", "STREAMINFO min above max", "STREAMINFO min above the frames",
    "STREAMINFO max below the frames", "total samples + 1", "one MD5 byte flipped", "max frame size - 1",
    "min frame size + 1", "partition order 6 under FIXED(4)", "partition order 7", "coding method 1",
    "one trailing byte", "a frame missing", "a short frame in the middle", "stereo assignment in a mono stream",
    "sample-size code 3", "channel assignment 11", "a frame-number bit, CRC-8 as it was",
    "a VERBATIM sample's low bit, CRC-16 as it was", "a CRC-16 bit",
]


@pytest.mark.parametrize("name", MUTATIONS)
def test_notices(base, name):
    data, rep, x = base
    table = _mutations(data, rep)
    assert sorted(table) == sorted(MUTATIONS)
    mutated, rule, frame = table[name]
    assert mutated != data
    with pytest.raises(fv.FlacFormatError) as e:
        fv.verify(mutated)
    assert (e.value.rule, e.value.frame) == (rule, frame), str(e.value)


def test_rebuilding_a_header_unchanged_changes_nothing(base):
    """the mutation helpers themselves: no change, no difference"""
    data, rep, x = base
    for k in range(len(rep["frames"])):
        assert _reheaded(data, rep, k) == data
        assert _bit_changed(data, rep, k, 0, 1) == data


def test_profile_rules(base):
    data, rep, x = base
    assert fv.profile_rate_code(65535) == 13 and fv.profile_rate_code(65536) == 0
    assert fv.profile_rate_code(655350) == 0 and fv.profile_rate_code(655340) == 14
    assert fv.profile_rate_code(384000) == 14 and fv.profile_rate_code(352800) == 14
    assert fv.profile_rate_code(1048575) == 0 and fv.profile_rate_code(96000) == 11
    assert [fv.profile_block_code(n) for n in (192, 576, 4608, 256, 4096, 16, 255, 257, 4607)] == \
        [1, 2, 5, 8, 12, 6, 6, 7, 7]
    # the base stream with the encoder's header codes in every frame passes the profile ...
    prof = _streaminfo_changed(_streaminfo_changed(data, 88, 24, 0), 64, 24, 0)    # frame sizes: unknown
    for k, fr in enumerate(rep["frames"]):
        n = fr["block"]
        code = fv.profile_block_code(n)
        prof = _reheaded(prof, fv.verify(prof)[1], k, scode=4, rcode=9, rextra=b"", bcode=code,
                         bextra=(n - 1).to_bytes(1, "big") if code == 6 else b"")
    got, prep = fv.verify(prof, profile=True)
    np.testing.assert_array_equal(got, x)
    # ... and one header code off the table does not
    for changes, rule in ((dict(scode=0), "profile_sample_size_code"), (dict(rcode=0), "profile_rate_code"),
                          (dict(rcode=13, rextra=FS.to_bytes(2, "big")), "profile_rate_code"),
                          (dict(bcode=7, bextra=(BLOCK - 1).to_bytes(2, "big")), "profile_block_code")):
        with pytest.raises(fv.FlacFormatError) as e:
            fv.verify(_reheaded(prof, prep, 2, **changes), profile=True)
        assert (e.value.rule, e.value.frame) == (rule, 2)
        fv.verify(_reheaded(prof, prep, 2, **changes))
    with pytest.raises(fv.FlacFormatError) as e:
        fv.verify(prof[:4] + b"\x00" + prof[5:42] + b"\x81\x00\x00\x02ab" + prof[42:], profile=True)
    assert e.value.rule == "profile_metadata"


# ------------------------------------------------------------------ the container on small inputs
@pytest.mark.parametrize("n", [1, 3, 15, 16, 700])
def test_container_of_one_short_frame(n):
    """flac_container in front of one frame of n samples in a block of 4096: both of
    STREAMINFO's block sizes must lie in 16..65535 (RFC 9639 8.2)"""
    from amx import flacio
    x = _signal(n, 2, seed=n)
    src, rep = _accepted(x, 48000, 4096, ["verbatim", "fixed1"], metadata=False)
    payload = src[42:]
    md5 = hashlib.md5(x.astype("<i2").tobytes()).digest()
    out = flacio.flac_container(payload, [len(payload)], 48000, 2, n, 4096, md5)
    got, rep = fv.verify(out, frame_bytes=[len(payload)])
    np.testing.assert_array_equal(got, x)
    assert rep["md5_checked"] and rep["min_block"] == rep["max_block"] == max(16, n)
    _agrees_with_the_library(out, x)
