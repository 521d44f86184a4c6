"""FLAC input decoded on the device (amx_flac_decode_device, csrc/amx_flacdec.hip) against
the host decoder (amx_flac_decode, csrc/amx_flac.cpp: no decoding code in common): the same
int32 array, bit for bit, and the same block list.  Every case first decodes on the host,
so none is vacuous, and checks that the scan accepts the stream, so none is the fallback.
The streams are flac_fixtures.matrix() (the matrix test_flac_decode_core.py runs on the CPU
through the same core); then the device encoder's streams (partition order 6, 12-bit LPC
coefficients), corrupt input, the streams left to the host path, and buffer reuse."""
import ctypes

import numpy as np
import pytest

import flac_enc
import flac_fixtures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def streams():
    """[(name, bytes, host samples, host blocks)], the host decode done once"""
    from amx import flacio
    out = []
    for name, data in flac_fixtures.matrix():
        x, _, blocks = flacio.decode_flac(data, with_blocks=True)
        out.append((name, data, x, blocks))
    return out


def _check(data, want, blocks):
    """the device path on `data` (it must take it: no fallback) equals the host's result"""
    import torch
    from amx import capi, flacio
    rc, sc, _ = flacio.flac_scan(data[flacio._skip_id3(data[:10]):])
    assert rc == capi.AMX_OK
    got, info, gblocks = flacio.decode_flac_device(data)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert gblocks.tolist() == blocks.tolist()
    assert (info.channels, info.total_frames) == (want.shape[1], want.shape[0])
    return sc


GROUPS = {
    "depths": lambda n: n.startswith("depth"),
    "kinds_a0_a8": lambda n: "_a0_" in n or "_a8_" in n,
    "kinds_a9_a10": lambda n: "_a9_" in n or "_a10_" in n,
    "blocking": lambda n: n.startswith(("block", "tail", "variable")),
    "channels": lambda n: n.startswith("ch"),
    "one_long_frame": lambda n: n == "mono65535",
    "id3": lambda n: n == "id3",
}


def test_groups_cover_the_matrix(streams):
    names = [s[0] for s in streams if s[0] != "false_syncs"]
    assert all(sum(bool(g(n)) for g in GROUPS.values()) == 1 for n in names)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_matrix(gpu, streams, group):
    sel = [s for s in streams if GROUPS[group](s[0])]
    assert sel
    for name, data, want, blocks in sel:
        sc = _check(data, want, blocks)
        if name == "block16x200":
            assert sc.n_cand >= 200 and len(blocks) == 200          # several waves, two-byte frame numbers
        if name == "mono65535":
            assert blocks.tolist() == [65535]


def test_false_syncs(gpu, streams):
    name, data, want, blocks = [s for s in streams if s[0] == "false_syncs"][0]
    sc = _check(data, want, blocks)
    assert sc.n_cand > len(blocks) == flac_fixtures.false_sync_stream()[1]


@pytest.mark.parametrize("lpc_order,block", [(0, 4096), (8, 4096), (0, 256), (8, 256)])
def test_device_encoder_round_trip(gpu, lpc_order, block):
    """the device encoder's streams (partition orders up to 6, LPC with 12-bit coefficients)
    decode back to the samples, and as the host decodes them"""
    import torch
    from amx import flacio, synth
    fs, n = 48000, 20000
    x = np.clip(np.round(synth.mix_like(n, fs, 2, seed=11) * 32767.0), -32768, 32767).astype(np.int16)
    data = flacio.flac_bytes(x, fs, block=block, md5=False, lpc_order=lpc_order)
    want, _, blocks = flacio.decode_flac(data, with_blocks=True)
    got, _, gblocks = flacio.decode_flac_device(data)
    assert torch.equal(got.cpu(), torch.from_numpy(x.astype(np.int32) << 16))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert gblocks.tolist() == blocks.tolist()


def _message(fn, data):
    from amx import capi
    with pytest.raises(capi.AmxError) as e:
        fn(data)
    return str(e.value)


def test_corrupt_input_raises_like_the_host(gpu, streams):
    """(run on the GPU only because test_flac_decode_core.py's fuzz of the same code passes)"""
    from amx import flacio
    name, data, want, blocks = [s for s in streams if s[0] == "depth16_ch2"][0]
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10                       # a middle frame's CRC-16 fails
    for bad in (bytes(flipped), data[:len(data) * 2 // 3], b"RIFF" + bytes(100)):
        assert _message(flacio.decode_flac_device, bad) == _message(flacio.decode_flac, bad)
        _check(data, want, blocks)                        # and the next valid decode is exact


def test_streams_left_to_the_host(gpu):
    """32 bits per sample and a STREAMINFO without the length: the scan says so before any
    launch, and decode_flac_device hands on the host decoder's samples"""
    import torch
    from amx import capi, flacio
    x32 = flac_fixtures.signal(3000, 2, 32, seed=8)
    d32 = flac_enc.encode(x32, 48000, 32, seed=8, kinds=["verbatim", "fixed1"], assigns=[0], block=576)
    d0 = bytearray(flac_enc.encode(flac_fixtures.signal(3000, 2, 16, seed=9), 48000, 16, seed=9, block=576))
    d0[21] &= 0xF0                                        # STREAMINFO's 36-bit length: 0 = unknown
    d0[22:26] = bytes(4)
    for data in (d32, bytes(d0)):
        want, _, blocks = flacio.decode_flac(data, with_blocks=True)
        assert len(want) == 3000
        assert flacio.flac_scan(data)[0] == capi.AMX_EUNSUPPORTED
        got, _, gblocks = flacio.decode_flac_device(data)
        assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(want))
        assert gblocks.tolist() == blocks.tolist()


class _Raw:
    """amx_flac_decode_device on caller-held buffers"""

    def __init__(self, out_elems, ws_bytes, max_blocks):
        import torch
        self.out = torch.full((out_elems,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.ws = torch.zeros(ws_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        self.blocks = torch.full((max_blocks,), -7, dtype=torch.int32, device="cuda")
        self.res = torch.zeros(4, dtype=torch.int64, device="cuda")

    def run(self, data):
        import torch
        from amx import capi, flacio
        rc, sc, tab = flacio.flac_scan(data)
        assert rc == capi.AMX_OK and sc.workspace_bytes <= self.ws.numel() * 8
        d_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        d_cand = torch.from_numpy(tab.copy()).cuda()
        L = capi.load()
        capi.check(L.amx_flac_decode_device(capi.ptr(d_data), len(data), capi.ptr(d_cand), ctypes.byref(sc),
                                            capi.ptr(self.out), self.out.numel() // sc.channels,
                                            capi.ptr(self.blocks), self.blocks.numel(), capi.ptr(self.res),
                                            capi.ptr(self.ws), self.ws.numel() * 8, capi.ptr_stream()),
                   "amx_flac_decode_device")
        res = self.res.cpu().numpy()
        assert res[0] == capi.AMX_OK and res[1] == sc.total_frames
        return sc, self.out.cpu().numpy(), self.blocks.cpu().numpy()[:res[2]]


def test_buffers_reused_and_not_overrun(gpu, streams):
    """two different streams through the same workspace, output and block buffers; the output
    buffer holds spare elements behind the larger stream, which stay untouched, and nothing
    is written past frames x channels of the smaller one"""
    from amx import flacio
    pick = [s for s in streams if s[0] in ("variable", "lpc_a10_b576", "depth24_ch2", "variable")]
    assert len(pick) == 3
    ws = max(flacio.flac_scan(s[1])[1].workspace_bytes for s in pick)
    largest = max(s[2].size for s in pick)
    raw = _Raw(largest + 1, ws, max(flacio.flac_scan(s[1])[1].n_cand for s in pick))
    for name, data, want, blocks in pick + pick[:1]:
        raw.out.fill_(0x5A5A5A5A)
        sc, out, gblocks = raw.run(data)
        assert np.array_equal(out[:want.size], want.reshape(-1)), name
        assert np.all(out[want.size:] == 0x5A5A5A5A), name
        assert gblocks.tolist() == blocks.tolist(), name


def test_arguments_are_checked_before_any_launch(gpu, streams):
    import torch
    from amx import capi, flacio
    name, data, want, blocks = streams[0]
    rc, sc, tab = flacio.flac_scan(data)
    L = capi.load()
    d = torch.zeros(max(want.size, sc.workspace_bytes // 4 + 8), dtype=torch.int32, device="cuda")
    d_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_cand = torch.from_numpy(tab.copy()).cuda()

    def call(out_frames=sc.total_frames, max_blocks=sc.n_cand, ws_bytes=sc.workspace_bytes, ws_shift=0, scan=sc):
        return L.amx_flac_decode_device(capi.ptr(d_data), len(data), capi.ptr(d_cand), ctypes.byref(scan),
                                        capi.ptr(d), out_frames, capi.ptr(d), max_blocks, capi.ptr(d),
                                        ctypes.c_void_p(d.data_ptr() + ws_shift), ws_bytes, capi.ptr_stream())
    assert call(out_frames=sc.total_frames - 1) == capi.AMX_ERANGE
    assert call(max_blocks=0) == capi.AMX_ERANGE
    assert call(ws_bytes=sc.workspace_bytes - 1) == capi.AMX_ERANGE
    assert call(ws_shift=4) == capi.AMX_EINVAL
    empty = capi.FlacScan()
    assert call(scan=empty) == capi.AMX_EINVAL
    torch.cuda.synchronize()
    assert int(d.abs().max()) == 0                        # nothing ran
