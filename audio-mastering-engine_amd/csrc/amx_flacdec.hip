// amx_flacdec.hip -- FLAC input decoded on the device: the file's bytes go
// up as they are, the host scan (amx_flac_scan) lists every sync candidate with its parsed
// header, and three kernels turn them into the int32 [frames][C] array amx_flac_decode
// fills.
//
//   k_flacd_frames  one wave per candidate, one lane of it decoding: the frame's subframes
//                   (amx_flacdec_core.hpp, the text the CPU test runs) into the candidate's
//                   scratch slot, the frame's end, its CRC-16, and the candidate that starts
//                   at that end
//   k_flacd_chain   one workgroup: the chain of frames that tiles the stream from the
//                   first one, each frame's first sample, the block list, the status
//   k_flacd_emit    one workgroup per chained frame: stereo decorrelation, left
//                   justification, interleaved stores at the frame's first sample
//
// The decoded samples pass through a 32-sample ring in LDS: it is the LPC history, and it
// leaves for the scratch slot in runs of 16 samples as 16-byte stores.  LPC coefficients
// live in LDS too; nothing is indexed dynamically in registers.
#include "../../include/amx.h"
#include "amx_internal.hpp"
#include "amx_flacdec_core.hpp"

namespace amx {
namespace {

#define FLACD_LANES 64
#define FLACD_CHAIN_LDS 8192   // candidates k_flacd_chain stages in LDS (more: it walks global memory)

struct LaneStore {
    int32_t *ring;   // LDS [32]: the last 32 samples, unshifted
    int32_t *cf;     // LDS [32]
    int32_t *slot;   // the candidate's scratch slot: C planes of `stride` samples
    int64_t stride;
    int32_t *dst;
    int wasted;
    __device__ void begin(int channel, int w) {
        dst = slot + channel * stride;
        wasted = w;
    }
    __device__ void flush(int i0) {   // samples i0 .. i0 + 15 (i0 a multiple of 16, inside the plane)
        for (int j = 0; j < 16; j += 4) {
            int4 v;
            v.x = (int32_t)((uint32_t)ring[((i0 + j) & 31)] << wasted);
            v.y = (int32_t)((uint32_t)ring[((i0 + j + 1) & 31)] << wasted);
            v.z = (int32_t)((uint32_t)ring[((i0 + j + 2) & 31)] << wasted);
            v.w = (int32_t)((uint32_t)ring[((i0 + j + 3) & 31)] << wasted);
            *reinterpret_cast<int4 *>(dst + i0 + j) = v;
        }
    }
    __device__ void put(int i, int32_t v) {
        ring[(i & 31)] = v;
        if ((i & 15) == 15) flush(i - 15);
    }
    __device__ int32_t get(int i) const { return ring[(i & 31)]; }
    __device__ void finish(int n) {
        if (n & 15) flush(n & ~15);   // the plane is padded to whole runs (plane_stride)
    }
    __device__ void coef_set(int k, int32_t c) { cf[k] = c; }
    __device__ int32_t coef(int k) const { return cf[k]; }
    __device__ void out_of_width() {}
};

// flag: 0 not a frame (syntax, width, bound or CRC-16), 1 ok, 2 a frame header of more than
// 24 bits (the host path's)
__global__ __launch_bounds__(FLACD_LANES) void k_flacd_frames(const uint8_t *data, int64_t size,
                                                              const amx_flac_cand_t *cand, int64_t nc, int C,
                                                              int32_t *scratch, int64_t scratch_samples,
                                                              int64_t *endb, int32_t *nxt, int32_t *flag) {
    __shared__ int32_t ring[32];
    __shared__ int32_t coef[32];
    __shared__ uint16_t tab[256];
    for (int i = threadIdx.x; i < 256; i += FLACD_LANES) tab[i] = flacd::crc16_entry(i);
    __syncthreads();
    // one candidate per wave: the wave's other lanes only helped with the table (3.11: packing
    // candidates into a wave's lanes makes every lane wait for every other lane's loads)
    const int64_t k = blockIdx.x;
    if (threadIdx.x != 0 || k >= nc) return;
    const amx_flac_cand_t c = cand[k];
    int f = 0;
    int64_t e = 0;
    if (c.block >= 1 && c.block <= 65535) {
        const int64_t stride = flacd::plane_stride(c.block);
        // the slot the scan assigned must lie inside the scratch array, on a 16-byte boundary
        if (c.slot >= 0 && (c.slot & 3) == 0 && c.slot <= scratch_samples - C * stride) {
            if (c.bps > 24) {
                f = 2;
            } else {
                LaneStore st{ring, coef, scratch + c.slot, stride, nullptr, 0};
                if (flacd::decode_frame(data, size, c.offset, c.data_byte, c.limit, c.block, c.bps, c.assign, C, st,
                                        tab, &e))
                    f = 1;
            }
        }
    }
    // the candidate that starts exactly where this frame ends (offsets ascend)
    int32_t j = -1;
    if (f == 1 && e < size) {
        int64_t lo = k + 1, hi = nc;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (cand[mid].offset < e) lo = mid + 1;
            else hi = mid;
        }
        if (lo < nc && cand[lo].offset == e) j = (int32_t)lo;
    }
    flag[k] = f;
    endb[k] = e;
    nxt[k] = j;
}

// result: [0] status (AMX_OK, AMX_EINVAL, AMX_ERANGE, or AMX_EUNSUPPORTED: the chain met a
// frame the device path leaves to the host), [1] frames, [2] chained FLAC frames, [3] the
// candidate the walk stopped at (-1: a clean end)
__global__ __launch_bounds__(256) void k_flacd_chain(const amx_flac_cand_t *cand, int64_t nc, int64_t first_frame,
                                                     int64_t total, int64_t max_blocks, const int32_t *nxt,
                                                     const int32_t *flag, int32_t *chain, int64_t *first,
                                                     int32_t *blocks, int64_t *result) {
    __shared__ int32_t s_nxt[FLACD_CHAIN_LDS];   // the next candidate, -1 none, -2 this one is not ok
    __shared__ uint16_t s_blk[FLACD_CHAIN_LDS];  // block - 1
    const bool lds = nc <= FLACD_CHAIN_LDS;
    if (lds) {
        for (int64_t i = threadIdx.x; i < nc; i += blockDim.x) {
            s_nxt[i] = flag[i] == 1 ? nxt[i] : -2;
            s_blk[i] = (uint16_t)(cand[i].block - 1);
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int64_t samples = 0, stop = -1, n;
    if (lds)
        n = flacd::walk_chain(
            nc, [&](int64_t k) { return s_nxt[k] == -2 ? 0 : 1; }, [&](int64_t k) { return (int64_t)s_nxt[k]; },
            [&](int64_t k) { return (int)s_blk[k] + 1; }, max_blocks, chain, first, blocks, &samples, &stop);
    else
        n = flacd::walk_chain(
            nc, [&](int64_t k) { return flag[k]; }, [&](int64_t k) { return (int64_t)nxt[k]; },
            [&](int64_t k) { return cand[k].block; }, max_blocks, chain, first, blocks, &samples, &stop);
    int64_t status = AMX_OK;
    if (cand[0].offset != first_frame) {
        status = AMX_EINVAL;
    } else if (stop >= 0 && flag[stop] == 2) {
        status = AMX_EUNSUPPORTED;
    } else if (stop >= 0 && flag[stop] == 1) {
        status = AMX_ERANGE;                       // max_blocks reached
    } else {
        if (samples > total) samples = total;      // (a padded last frame)
        if (samples < total) status = AMX_EINVAL;  // a corrupt or missing frame ended the chain early
    }
    result[0] = status;
    result[1] = status == AMX_OK ? samples : 0;
    result[2] = n;
    result[3] = stop;
}

__global__ __launch_bounds__(256) void k_flacd_emit(const amx_flac_cand_t *cand, int C, const int32_t *scratch,
                                                    const int32_t *chain, const int64_t *first,
                                                    const int64_t *result, int32_t *out) {
    const int64_t q = blockIdx.x;
    if (result[0] != AMX_OK || q >= result[2]) return;
    const amx_flac_cand_t c = cand[chain[q]];
    const int64_t f0 = first[q];
    const int64_t left = result[1] - f0;
    const int take = (int)(left < c.block ? (left > 0 ? left : 0) : c.block);
    const int64_t stride = flacd::plane_stride(c.block);
    const int32_t *p0 = scratch + c.slot;
    const int sh = 32 - c.bps;
    int32_t *o = out + f0 * C;
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int t = threadIdx.x, nt = blockDim.x;
    if (C == 2) {
        const int32_t *p1 = p0 + stride;
        auto one = [&](int i, int32_t &l, int32_t &r) {
            flacd::undo_stereo(c.assign, p0[i], p1[i], l, r);
            l = (int32_t)((uint32_t)l << sh);
            r = (int32_t)((uint32_t)r << sh);
        };
        // pairs of frames from the first frame that sits on a 16-byte boundary
        const int head = aligned ? (int)(f0 & 1) : take;
        for (int i = t; i < (head < take ? head : take); i += nt) {
            int32_t l, r;
            one(i, l, r);
            o[2 * i] = l;
            o[2 * i + 1] = r;
        }
        const int pairs = take > head ? (take - head) >> 1 : 0;
        for (int pi = t; pi < pairs; pi += nt) {
            const int i = head + 2 * pi;
            int4 v;
            one(i, v.x, v.y);
            one(i + 1, v.z, v.w);
            *reinterpret_cast<int4 *>(o + 2 * i) = v;
        }
        for (int i = head + 2 * pairs + t; i < take; i += nt) {
            int32_t l, r;
            one(i, l, r);
            o[2 * i] = l;
            o[2 * i + 1] = r;
        }
    } else if (C == 1) {
        const int head0 = (int)((4 - (f0 & 3)) & 3);
        const int head = aligned ? (head0 < take ? head0 : take) : take;
        for (int i = t; i < head; i += nt) o[i] = (int32_t)((uint32_t)p0[i] << sh);
        const int quads = (take - head) >> 2;
        for (int qi = t; qi < quads; qi += nt) {
            const int i = head + 4 * qi;
            int4 v;
            v.x = (int32_t)((uint32_t)p0[i] << sh);
            v.y = (int32_t)((uint32_t)p0[i + 1] << sh);
            v.z = (int32_t)((uint32_t)p0[i + 2] << sh);
            v.w = (int32_t)((uint32_t)p0[i + 3] << sh);
            *reinterpret_cast<int4 *>(o + i) = v;
        }
        for (int i = head + 4 * quads + t; i < take; i += nt) o[i] = (int32_t)((uint32_t)p0[i] << sh);
    } else {
        const int64_t n = (int64_t)take * C;
        for (int64_t idx = t; idx < n; idx += nt) {
            const int i = (int)(idx / C), ch = (int)(idx - (int64_t)i * C);
            o[idx] = (int32_t)((uint32_t)p0[ch * stride + i] << sh);
        }
    }
}

}  // namespace

int64_t flac_decode_ws_bytes(int64_t n_cand, int64_t scratch_samples) {
    return 32 * n_cand + 64 + 4 * scratch_samples;
}

hipError_t launch_flac_decode(const uint8_t *data, int64_t size, const amx_flac_cand_t *cand, int64_t nc, int C,
                              int64_t total, int64_t first_frame, int64_t scratch_samples, int32_t *out,
                              int32_t *blocks, int64_t max_blocks, int64_t *result, void *ws, hipStream_t st) {
    if (nc < 1 || nc > INT32_MAX || C < 1 || C > 8) return hipErrorInvalidValue;
    char *w = static_cast<char *>(ws);
    int64_t *endb = reinterpret_cast<int64_t *>(w);
    int64_t *first = reinterpret_cast<int64_t *>(w + 8 * nc);
    int32_t *nxt = reinterpret_cast<int32_t *>(w + 16 * nc);
    int32_t *flag = reinterpret_cast<int32_t *>(w + 20 * nc);
    int32_t *chain = reinterpret_cast<int32_t *>(w + 24 * nc);
    int32_t *scratch = reinterpret_cast<int32_t *>(w + ((32 * nc + 63) & ~(int64_t)63));
    hipLaunchKernelGGL(k_flacd_frames, dim3((unsigned)nc), dim3(FLACD_LANES), 0, st, data, size, cand, nc, C, scratch,
                       scratch_samples, endb, nxt, flag);
    hipLaunchKernelGGL(k_flacd_chain, dim3(1), dim3(256), 0, st, cand, nc, first_frame, total, max_blocks, nxt, flag,
                       chain, first, blocks, result);
    const int64_t ge = nc < max_blocks ? nc : max_blocks;
    if (ge > 0)
        hipLaunchKernelGGL(k_flacd_emit, dim3((unsigned)ge), dim3(256), 0, st, cand, C, scratch, chain, first, result,
                           out);
    return hipGetLastError();
}

}  // namespace amx
