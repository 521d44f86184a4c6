// amx_resample.hip -- the finished master at another sample rate.
//
// libswresample's float (FLTP) resampler applied to the 16-bit master, as
// `ffmpeg -i master.wav -af aresample=R:internal_sample_fmt=fltp` runs it, then the
// f32 -> s16 conversion: restated in oracle/amx_oracle.c (swr_block, swr_dot) and pinned
// to that restatement.  With exact_rational the phase step is an integer for every pair
// with L <= 1024 phases (out / in = L / M reduced), so no output interpolates:
//   output j   reads input frames base - center + i, i < filter_alloc,
//              base = (j M) div L, row (j M) mod L of the bank (amx::swr_bank);
//   the input  is mirrored at both ends (x[-k] = x[k], x[n + k] = x[n - 1 - k]), as often
//              as it takes: an input may be shorter than the filter;
//   a tap      is (float)x * (1.0f / 32768.0f);
//   the dot    is 8 fused chains over taps k, k + 8, k + 16, ... of the whole row, then
//              (a0 + a4 + a2 + a6) + (a1 + a5 + a3 + a7)  (resample.asm, FMA3);
//   the sample is av_clip_int16(lrintf(v * 32768)).
//
// One workgroup makes AMX_RS_TILE output frames of all C channels.  The tile's input
// window is staged once in LDS as floats, one plane per channel, already mirrored; lane s
// of the tile makes output sample s (frame s / C, channel s % C), so a wave's int16 stores
// are one contiguous run.  The plane pitch is 2 mod 32 dwords: the two channels of a stereo
// half-wave then read disjoint banks.  With one phase (an integer ratio such as 192 -> 48
// kHz) the row is the same for every lane and its taps are scalar operands (k_resample<true>).
// With more the bank is stored tap-major ([tap][phase]), so the lanes of a wave read one tap
// of their rows from a span of L floats: from LDS, staged once per persistent workgroup
// (k_resample_lb), when it fits beside the windows (147 x 144 floats = 85 KB for 192 -> 44.1
// kHz, which needs the dynamic-LDS attribute), else from global memory (k_resample<false>:
// 2.3 to 2.7 times slower where both run).  Every output sample is written
// by exactly one store and nothing else is written.
#include "amx_swr_dev.hpp"

namespace amx {

struct RsGeom {
    int32_t L, M;          // out / in reduced: output j sits at input position j M / L
    int32_t alloc, center; // filter_alloc, (filter_length - 1) / 2
    int32_t C;             // channels, 1..8
    int32_t pitch;         // dwords per channel plane of the window
};

// frames per window plane a tile can need, and the plane pitch (2 mod 32 dwords)
static int rs_window(int L, int M, int alloc) {
    return (int)(((int64_t)(AMX_RS_TILE - 1) * M) / L) + 1 + alloc;
}
static int rs_pitch(int window) { return ((window - 2 + 31) / 32) * 32 + 2; }

// One tile: `tile` output frames from j0, by the 256 threads `tid` of one tile group.
// win: the group's window planes; bank: ONE: the row; else tap-major [alloc][L], in global
// memory or (k_resample_lb) in LDS.  The caller puts a barrier between the two halves.
__device__ __forceinline__ void rs_stage(float *win, const int16_t *__restrict__ in, int64_t n, const RsGeom &g,
                                         int64_t j0, int tile, int tid, int &r0) {
    const int64_t p0 = j0 * g.M;
    const int64_t b0 = p0 / g.L;
    r0 = (int)(p0 - b0 * g.L);
    const int64_t w0 = b0 - g.center;                  // input frame of window position 0
    // the tile's last output starts at window position (r0 + (tile - 1) M) div L
    const int wn = (r0 + (tile - 1) * g.M) / g.L + g.alloc;
    for (int e = tid; e < wn * g.C; e += AMX_BLOCK) {
        const int x = e / g.C, c = e - x * g.C;
        win[c * g.pitch + x] = swr_s16(in[swr_reflect(w0 + x, n) * g.C + c]);
    }
}

template <bool ONE>
__device__ __forceinline__ void rs_dots(const float *win, const float *__restrict__ bank, int16_t *__restrict__ out,
                                        const RsGeom &g, int64_t j0, int tile, int tid, int r0) {
    for (int s = tid; s < tile * g.C; s += AMX_BLOCK) {
        const int f = s / g.C, c = s - f * g.C;
        const int t = r0 + f * g.M;
        const int xb = t / g.L, ph = t - xb * g.L;
        const float *w = win + c * g.pitch + xb;
        // the bank's tap stride: ONE: the row; else tap-major, row ph
        const float v = swr_dot_rows<float>([&](int k) { return w[k]; }, ONE ? bank : bank + ph, ONE ? 1 : g.L, g.alloc);
        out[j0 * g.C + s] = q_f32_to_s16_ffmpeg(v);
    }
}

template <bool ONE>
__global__ void __launch_bounds__(AMX_BLOCK) k_resample(const int16_t *__restrict__ in, int64_t n,
                                                         int16_t *__restrict__ out, int64_t out_frames,
                                                         const float *__restrict__ bank, RsGeom g) {
    extern __shared__ float rs_win[];
    const int64_t j0 = (int64_t)blockIdx.x * AMX_RS_TILE;
    const int64_t left = out_frames - j0;
    const int tile = left < AMX_RS_TILE ? (int)left : AMX_RS_TILE;
    int r0;
    rs_stage(rs_win, in, n, g, j0, tile, threadIdx.x, r0);
    __syncthreads();
    rs_dots<ONE>(rs_win, bank, out, g, j0, tile, threadIdx.x, r0);
}

// The many-phase form with the bank in LDS: persistent workgroups of AMX_RS_LB_GROUPS tile
// groups (256 threads and a window each) stage the tap-major bank once and then take tiles
// gridDim.x * AMX_RS_LB_GROUPS apart.
#define AMX_RS_LB_GROUPS 4
__global__ void __launch_bounds__(AMX_BLOCK *AMX_RS_LB_GROUPS)
    k_resample_lb(const int16_t *__restrict__ in, int64_t n, int16_t *__restrict__ out, int64_t out_frames,
                  const float *__restrict__ bank, RsGeom g, int64_t tiles) {
    extern __shared__ float rs_win[];
    float *lbank = rs_win + AMX_RS_LB_GROUPS * g.C * g.pitch;
    for (int i = threadIdx.x; i < g.alloc * g.L; i += AMX_BLOCK * AMX_RS_LB_GROUPS) lbank[i] = bank[i];
    const int grp = threadIdx.x / AMX_BLOCK, tid = threadIdx.x - grp * AMX_BLOCK;
    float *win = rs_win + grp * g.C * g.pitch;
    for (int64_t t0 = (int64_t)blockIdx.x * AMX_RS_LB_GROUPS; t0 < tiles;
         t0 += (int64_t)gridDim.x * AMX_RS_LB_GROUPS) {
        const int64_t j0 = (t0 + grp) * AMX_RS_TILE;
        const int64_t left = out_frames - j0;
        const int tile = left < AMX_RS_TILE ? (left > 0 ? (int)left : 0) : AMX_RS_TILE;
        int r0 = 0;
        __syncthreads();                               // the bank; the previous turn's window reads
        if (tile > 0) rs_stage(win, in, n, g, j0, tile, tid, r0);
        __syncthreads();
        if (tile > 0) rs_dots<false>(win, lbank, out, g, j0, tile, tid, r0);
    }
}

// LDS bytes: k_resample's window, and k_resample_lb's windows + bank.  Above 64 KiB a kernel
// needs the dynamic-LDS attribute (resample_prepare, from amx_resampler_create).
#define AMX_RS_LDS_MAX (80 * 1024)
#define AMX_RS_LB_LDS_MAX (160 * 1024)
static int64_t rs_lds(int L, int M, int alloc, int C) {
    return (int64_t)rs_pitch(rs_window(L, M, alloc)) * C * (int64_t)sizeof(float);
}
static int64_t rs_lb_lds(int L, int M, int alloc, int C) {
    return AMX_RS_LB_GROUPS * rs_lds(L, M, alloc, C) + (int64_t)L * alloc * (int64_t)sizeof(float);
}
// the bank goes to LDS when there are several phases and it fits beside the windows
static bool rs_use_lb(int L, int M, int alloc, int C) {
    return L > 1 && rs_lb_lds(L, M, alloc, C) <= AMX_RS_LB_LDS_MAX;
}
hipError_t resample_prepare(int L, int M, int alloc, int C) {
    if (rs_lds(L, M, alloc, C) > AMX_RS_LDS_MAX) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (rs_lds(L, M, alloc, C) > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resample<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, AMX_RS_LDS_MAX);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resample<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, AMX_RS_LDS_MAX);
    }
    if (e == hipSuccess && rs_use_lb(L, M, alloc, C) && rs_lb_lds(L, M, alloc, C) > 64 * 1024)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resample_lb),
                                hipFuncAttributeMaxDynamicSharedMemorySize, AMX_RS_LB_LDS_MAX);
    return e;
}

// bank: L == 1: the row (alloc floats); else tap-major [alloc][L].  ncu: the device's CUs
// (k_resample_lb's persistent grid)
hipError_t launch_resample(int L, int M, int alloc, int center, int C, const float *bank, int ncu,
                           const int16_t *in, int64_t frames, int16_t *out, int64_t out_frames, hipStream_t st) {
    if (frames <= 0 || out_frames <= 0) return hipSuccess;
    const int64_t tiles = (out_frames + AMX_RS_TILE - 1) / AMX_RS_TILE;
    if (tiles > INT32_MAX || C < 1 || C > 8 || alloc < 8 || (alloc & 7) || ncu < 1) return hipErrorInvalidValue;
    RsGeom g;
    g.L = L;
    g.M = M;
    g.alloc = alloc;
    g.center = center;
    g.C = C;
    g.pitch = rs_pitch(rs_window(L, M, alloc));
    const size_t lds = (size_t)rs_lds(L, M, alloc, C);
    if (L == 1) {
        hipLaunchKernelGGL(k_resample<true>, dim3((unsigned)tiles), dim3(AMX_BLOCK), lds, st, in, frames, out,
                           out_frames, bank, g);
    } else if (rs_use_lb(L, M, alloc, C)) {
        const int64_t groups = (tiles + AMX_RS_LB_GROUPS - 1) / AMX_RS_LB_GROUPS;
        hipLaunchKernelGGL(k_resample_lb, dim3((unsigned)(groups < ncu ? groups : ncu)),
                           dim3(AMX_BLOCK * AMX_RS_LB_GROUPS), (size_t)rs_lb_lds(L, M, alloc, C), st, in, frames,
                           out, out_frames, bank, g, tiles);
    } else {
        hipLaunchKernelGGL(k_resample<false>, dim3((unsigned)tiles), dim3(AMX_BLOCK), lds, st, in, frames, out,
                           out_frames, bank, g);
    }
    return hipGetLastError();
}

}  // namespace amx
