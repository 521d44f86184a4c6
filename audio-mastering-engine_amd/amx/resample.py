"""The finished master at another sample rate: amx_resampler_* of
include/amx.h, libswresample's float resampler on the int16 master and its f32 -> s16
conversion, one HIP kernel (csrc/amx_resample.hip).

resample_s16 is what master_audio / master_array run after the alimiter when the
settings key output_rate asks for a rate the master is not at."""
import ctypes

from . import capi

TILE = 256        # output frames per workgroup of k_resample (AMX_RS_TILE, amx_tables.hpp)

_cache = {}


def size(in_rate, out_rate, frames=0):
    """amx_resample_size: (out_frames, filter_length, filter_alloc, phases) of the pair;
    capi.AmxError for a pair the resampler does not take (host only, no GPU needed)"""
    n, t, al, ph = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    capi.check(capi.load().amx_resample_size(int(in_rate), int(out_rate), int(frames), ctypes.byref(n),
                                             ctypes.byref(t), ctypes.byref(al), ctypes.byref(ph)),
               "amx_resample_size")
    return n.value, t.value, al.value, ph.value


def check_pair(in_rate, out_rate):
    """ValueError naming both rates unless the resampler takes in_rate -> out_rate (equal
    rates need none and pass)"""
    if int(in_rate) == int(out_rate):
        return
    rc = capi.load().amx_resample_size(int(in_rate), int(out_rate), 0, None, None, None, None)
    if rc != capi.AMX_OK:
        raise ValueError("output_rate: a master at %d Hz cannot be resampled to %d Hz (supported: rate pairs "
                         "out / in = L / M reduced with L <= 1024 and out >= in / 7.76)"
                         % (int(in_rate), int(out_rate)))


class Resampler:
    """Owns an amx_resampler* for one (in_rate, out_rate, channels)."""

    def __init__(self, in_rate, out_rate, channels):
        h = ctypes.c_void_p()
        capi.check(capi.load().amx_resampler_create(int(in_rate), int(out_rate), int(channels), ctypes.byref(h)),
                   "amx_resampler_create")
        self.h = h
        self.in_rate, self.out_rate, self.channels = int(in_rate), int(out_rate), int(channels)

    def out_frames(self, frames):
        return size(self.in_rate, self.out_rate, frames)[0]

    def run(self, y, out, capacity_frames=None, stream=None):
        """y int16 [frames, C] -> out (int16, room for capacity_frames frames; default: what
        the tensor holds); returns amx_resampler_run's code"""
        import torch
        if y.dtype != torch.int16 or out.dtype != torch.int16 or not y.is_contiguous() or not out.is_contiguous():
            raise ValueError("contiguous int16 tensors")
        if y.dim() != 2 or y.shape[1] != self.channels:
            raise ValueError("input must be [frames, %d]" % self.channels)
        cap = out.numel() // self.channels if capacity_frames is None else int(capacity_frames)
        if cap * self.channels > out.numel():
            raise ValueError("capacity_frames past the output tensor")
        return capi.load().amx_resampler_run(self.h, capi.ptr(y), int(y.shape[0]), capi.ptr(out), cap,
                                             capi.ptr_stream(stream))

    def close(self):
        if getattr(self, "h", None):
            capi.load().amx_resampler_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resample_s16(y_device, in_rate, out_rate, stream=None):
    """int16 CUDA tensor [frames, C] (C 1..8) at in_rate -> int16 CUDA tensor [out_frames, C]
    at out_rate, asynchronous on the stream (default: the current one).  The filter bank of
    a (rates, channels, device) triple is built once and kept."""
    import torch
    y = y_device
    if y.dim() == 1:
        y = y.reshape(-1, 1)
    if not y.is_cuda or y.dtype != torch.int16 or y.dim() != 2:
        raise ValueError("resample_s16 takes an int16 CUDA tensor [frames, C]")
    y = y.contiguous()
    key = (y.device.index, int(in_rate), int(out_rate), int(y.shape[1]))
    rs = _cache.get(key)
    if rs is None:
        with torch.cuda.device(y.device):
            rs = _cache[key] = Resampler(in_rate, out_rate, y.shape[1])
    n_out = rs.out_frames(y.shape[0])
    out = torch.empty((n_out, y.shape[1]), dtype=torch.int16, device=y.device)
    if n_out:
        with torch.cuda.device(y.device):
            capi.check(rs.run(y, out, n_out, stream), "amx_resampler_run")
    return out
