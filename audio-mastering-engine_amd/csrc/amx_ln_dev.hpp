// amx_ln_dev.hpp -- what af_loudnorm's frame-by-frame kernel k_ln_dyn<C> (amx_ln_dyn.hip,
// 2..8 channels) shares with the parallel form's k_lp_* (amx_loudnorm.hip, stereo).
// The frame geometry at 192 kHz, the workgroup reductions, the s16 conversion and
// r128_in's statistics from pass 1's hop energies (gating-block histogram, gated
// integrated loudness, relative gate, 3 s short-term).  The statistics read one track's
// hop rows [hops][2] and know nothing of the channel count: a C-channel track passes the
// rows amx_mc_loudness_combine wrote (the weighted sum in lane 0, 0 in lane 1).
#pragma once
#include "amx_dev.hpp"

#pragma clang fp contract(off)

namespace amx {

#define LN_FR 19200          // frame_size(192000, 100)
#define LN_FIRST 576000      // frame_size(192000, 3000)
#define LN_LIMF 40320        // frame_size(192000, 210): limiter ring frames
#define LN_ATT 1920          // frame_size(192000, 10)

// libebur128's default channel map (ebur128_init_channel_map): 4 channels L R Ls Rs, 5
// L R C Ls Rs, otherwise L R C unused Ls Rs, later channels unused; the surrounds
// (Mp110 / Mm110) weigh 1.41 (ebur128_calc_gating_block)
__device__ __forceinline__ double ebur_weight(int C, int c) {
    if (C == 4) return c < 2 ? 1.0 : 1.41;
    if (C == 5) return c < 3 ? 1.0 : 1.41;
    return c < 3 ? 1.0 : (c == 3 ? 0.0 : (c < 6 ? 1.41 : 0.0));
}

// ------------------------------------------------------------ block helpers
// The filter runs on one workgroup of LN_NT threads per track: every thread carries the
// (block-uniform) scalar state, the per-sample loops are shared out over the block.  One
// wave alone left every loop waiting on its own loads (HBM / L2 latency per 64 samples).
#define LN_NT 512
#define LN_NW (LN_NT / 64)

__device__ __forceinline__ double ln_wsum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// block sum / max of one value per thread (s_red: LN_NW doubles); every thread gets it
__device__ __forceinline__ double ln_bsum(double v, double *s_red) {
    v = ln_wsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int w = 0; w < LN_NW; w++) r += s_red[w];
    return r;
}
__device__ __forceinline__ double ln_bmax(double v, double *s_red) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s_red[0];
#pragma unroll
    for (int w = 1; w < LN_NW; w++) r = fmax(r, s_red[w]);
    return r;
}

__device__ __forceinline__ int16_t ln_s16(double v) {            // av_clip_int16(llrint(v * 32768))
    const double r = rint(v * 32768.0);
    return (int16_t)(r > 32767.0 ? 32767 : (r < -32768.0 ? -32768 : (int)r));
}

// ln_s16 with the clamp as fmax / fmin (two fp64 operations instead of two compares and
// four selects; the same value for every non-NaN v)
__device__ __forceinline__ int16_t ln_s16_lim(double v) {
    return (int16_t)(int)fmin(fmax(rint(v * 32768.0), -32768.0), 32767.0);
}

// k_ln_dyn's LDS, CH the channel count of the scan rows
template <int CH>
struct LnSharedT {
    unsigned hist[1000];               // r128_in's gating-block histogram, rebuilt here
    double E[1000], B[1001];
    double th[CH][LN_NT + 12];         // |x| of a scan group and the 12 positions after it
    double red[LN_NW];
    double oe[30];                     // r128_out: the last 30 frames' energies
    int first[LN_NW];
    double sbuf[1001];                 // ln_seq_sum
    int scan[LN_NW + 1];
};

__device__ __forceinline__ int ln_find_bin(const double *B, double e) {
    int lo = 0, hi = 1000;
    do {
        const int mid = (lo + hi) / 2;
        if (e >= B[mid]) lo = mid; else hi = mid;
    } while (hi - lo != 1);
    return lo;
}

// libebur128's sum over the bins j >= lo of hist[j] * E[j], in its sequential order
// (ebur128_gated_loudness's loop; k_decide's wave_seq_sum does the same): thread t owns
// bins [PER t, PER t + PER), the non-empty ones are compacted in bin order into sbuf
// (an empty bin adds 0.0, exactly) and thread 0 adds them one by one.  Every thread
// gets the sum.  sbuf: 1000 doubles; scan: NT / 64 + 1 ints.
template <int NT>
__device__ double ln_seq_sum(const unsigned *hist, const double *E, int lo, double *sbuf, int *scan) {
    constexpr int PER = (1000 + NT - 1) / NT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int mine = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int j = tid * PER + q;
        mine += (j < 1000 && j >= lo && hist[j] != 0u) ? 1 : 0;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) scan[w] = incl;
    __syncthreads();
    int off = incl - mine, tot = 0;
    for (int v = 0; v < NT / 64; v++) {
        off += v < w ? scan[v] : 0;
        tot += scan[v];
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int j = tid * PER + q;
        if (j < 1000 && j >= lo && hist[j] != 0u) sbuf[off++] = (double)hist[j] * E[j];
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int k = 0; k < tot; k++) acc += sbuf[k];
        sbuf[1000] = acc;
    }
    __syncthreads();
    const double r = sbuf[1000];
    __syncthreads();
    return r;
}

// ebur128 gated loudness + relative threshold of the histogram (every thread)
template <class SH>
__device__ void ln_global(SH &L, double &global, double &rel_thr) {
    const int tid = threadIdx.x;
    double c = 0.0;
    for (int j = tid; j < 1000; j += LN_NT) c += (double)L.hist[j];
    const double s = ln_seq_sum<LN_NT>(L.hist, L.E, 0, L.sbuf, L.scan);
    c = ln_bsum(c, L.red);
    if (c == 0.0) {
        global = -HUGE_VAL;
        rel_thr = -70.0;
        return;
    }
    double rel = s / c;
    rel *= 0.1;                                       // RELATIVE_GATE_FACTOR
    rel_thr = 10 * log10(rel) - 0.691;
    int start;
    if (rel < L.B[0]) start = 0;
    else {
        start = ln_find_bin(L.B, rel);
        if (rel > L.E[start]) ++start;
    }
    double a = 0.0;
    for (int j = start + tid; j < 1000; j += LN_NT) a += (double)L.hist[j];
    const double g = ln_seq_sum<LN_NT>(L.hist, L.E, start, L.sbuf, L.scan);
    a = ln_bsum(a, L.red);
    global = a == 0.0 ? -HUGE_VAL : 10 * log10(g / a) - 0.691;
}

// gating block ending at hop k (k >= 4): the mean square of hops k-4 .. k-1
__device__ __forceinline__ double ln_block_energy(const double *hops, int64_t k) {
    const double c0 = ((hops[2 * (k - 4)] + hops[2 * (k - 3)]) + hops[2 * (k - 2)]) + hops[2 * (k - 1)];
    const double c1 = ((hops[2 * (k - 4) + 1] + hops[2 * (k - 3) + 1]) + hops[2 * (k - 2) + 1]) + hops[2 * (k - 1) + 1];
    return (c0 + c1) / (double)(4 * LN_FR);
}
template <class SH>
__device__ __forceinline__ void ln_add_block(SH &L, const double *hops, int64_t k) {
    const double en = ln_block_energy(hops, k);
    __syncthreads();
    if (threadIdx.x == 0 && en >= L.B[0]) L.hist[ln_find_bin(L.B, en)] += 1u;
    __syncthreads();
}

// 3 s short-term loudness ending at hop k (hops k-30 .. k-1)
__device__ __forceinline__ double ln_shortterm(const double *hops, int64_t k, double *s_red) {
    const int tid = threadIdx.x;
    double c0 = 0.0, c1 = 0.0;
    if (tid < 30 && k - 30 + tid >= 0) {
        c0 = hops[2 * (k - 30 + tid)];
        c1 = hops[2 * (k - 30 + tid) + 1];
    }
    const double e = (ln_bsum(c0, s_red) + ln_bsum(c1, s_red)) / (double)LN_FIRST;
    return 10 * log10(e) - 0.691;
}

enum { LIM_OUT_, LIM_ATTACK_, LIM_SUSTAIN_, LIM_RELEASE_ };

// cycle counts of the kernel's parts (d_summary[2..]): where a track's time goes
struct LnProf {
    uint64_t fill = 0, detect = 0, env = 0, out = 0, stats = 0, feed = 0;
    uint64_t n_detect = 0, n_serial = 0;
};

}  // namespace amx
