// amx_swr_dev.hpp -- libswresample's float (FLTP) resampler arithmetic on the device, once,
// for the 192 kHz measurement (amx_loud192.hip), loudnorm's upsamplers (amx_loudnorm.hip) and
// the output resampler (amx_resample.hip).  Restated in oracle/amx_oracle.c ("libswresample").
//
//   a tap      is (float)s16 * (1.0f / 32768.0f);
//   the input  is mirrored at both ends, x[-k] = x[k], x[n + k] = x[n - 1 - k];
//   the dot    of a window with a bank row is the x86 FMA3 kernel's (resample.asm): 8 fused
//              chains over taps k, k + 8, k + 16, ... of the whole row, then
//              ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7)).
//
// The first term of a chain is the product w h, the later ones explicit fused multiply-adds;
// resample.asm starts from a zeroed register, fma(w, h, +0).  The two give the same bits here:
// a chain differs only when every product in it is a zero, +0 + -0 being +0 where -0 alone
// stays -0, and the dot differs only if all 8 chains are -0 under the multiply-first form
// (any +0 or non-zero chain makes the sum the same).  That needs the product at the row's
// positive main-lobe tap to be -0, so a -0.0f input, which (float)int16 * 2^-15 never is (every
// row swr_bank builds has a tap > 0: tests/test_plan_build.py).  The helpers use explicit
// fmaf / __builtin_elementwise_fma and plain adds, so they mean the same with FMA contraction
// on or off.
#pragma once
#include "amx_dev.hpp"

namespace amx {

#define SWR_TAPS 32        // filter_length = filter_alloc of every rate up to 192 kHz / 0.97
#define SWR_C 15           // its center tap, (SWR_TAPS - 1) / 2

typedef float swr_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float swr_s16(int16_t x) { return (float)x * (1.0f / 32768.0f); }
// channel ch of a stereo s16 frame
__device__ __forceinline__ float swr_tap(uint32_t w, int ch) { return swr_s16(ch ? hi16(w) : lo16(w)); }

// The mirror, applied as often as it takes (an input may be shorter than the filter): a
// compare and a subtraction per turn, where a closed form would be a 64-bit modulo per tap.
// A window starts less than one row outside [0, n) (-k or k - n + 1 <= AMX_RS_MAX_ALLOC, the
// widest row the resampler allows) and two turns move an index 2 n - 1 >= 3 towards the
// range when n >= 2, so 2 AMX_RS_MAX_ALLOC / 3 + 2 turns would do there; at n == 1 every
// index maps to 0, which is what running out of turns returns (n <= 0 cannot hang either).
__device__ __forceinline__ int64_t swr_reflect(int64_t k, int64_t n) {
    for (int it = 0; it < 2 * AMX_RS_MAX_ALLOC + 2; it++) {
        if (k < 0) k = -k;
        else if (k >= n) k = 2 * n - 1 - k;
        else return k;
    }
    return 0;
}

// the FMA3 kernel's horizontal sum of the 8 chains (V: float, or one lane per channel)
template <class V>
__device__ __forceinline__ V swr_hsum8(const V *a) {
    return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
}

// a window of SWR_TAPS taps in registers with a row of the bank
__device__ __forceinline__ float swr_dot32(const float *w, const float *__restrict__ h) {
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float acc = w[k] * h[k];
        acc = fmaf(w[k + 8], h[k + 8], acc);
        acc = fmaf(w[k + 16], h[k + 16], acc);
        acc = fmaf(w[k + 24], h[k + 24], acc);
        a[k] = acc;
    }
    return swr_hsum8(a);
}

// swr_dot32 with the 8 chains as 4 packed pairs (v_pk_fma_f32 / v_pk_add_f32): the same
// operations lane by lane.  P: the row's pointer type (k_ln_up_static's is address_space(4))
template <class P>
__device__ __forceinline__ float swr_dot32_pk(const float *w, P h) {
    swr_f2 a[4];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        swr_f2 acc = swr_f2{w[k], w[k + 1]} * swr_f2{h[k], h[k + 1]};
        acc = __builtin_elementwise_fma(swr_f2{w[k + 8], w[k + 9]}, swr_f2{h[k + 8], h[k + 9]}, acc);
        acc = __builtin_elementwise_fma(swr_f2{w[k + 16], w[k + 17]}, swr_f2{h[k + 16], h[k + 17]}, acc);
        acc = __builtin_elementwise_fma(swr_f2{w[k + 24], w[k + 25]}, swr_f2{h[k + 24], h[k + 25]}, acc);
        a[k >> 1] = acc;
    }
    const swr_f2 b01 = a[0] + a[2], b23 = a[1] + a[3];      // (a0+a4, a1+a5), (a2+a6, a3+a7)
    const swr_f2 c = b01 + b23;                             // (b0+b2, b1+b3)
    return c.x + c.y;
}

// a row of `alloc` taps (a multiple of 8; the zero padding after filter_length multiplies
// the frames there, as the x86 kernel does): tap(i) is the window's i-th tap -- a float, or
// a vector V with one lane per channel -- and the row's i-th tap is h[i * stride]
template <class V, class Tap>
__device__ __forceinline__ V swr_dot_rows(Tap tap, const float *__restrict__ h, int stride, int alloc) {
    V a[8];
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = tap(k) * h[k * stride];
    for (int q = 8; q < alloc; q += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) a[k] = __builtin_elementwise_fma(tap(q + k), (V)h[(q + k) * stride], a[k]);
    }
    return swr_hsum8(a);
}

// libswresample's linear float kernel (resample.asm, FMA3) for the rates whose 192 kHz
// phase step is not an integer (22.05 / 11.025 kHz: 1024 phases): the dots with rows h
// (phase ph) and h2 (ph + 1) as two sets of 8 fused chains over taps k, k+8, k+16, k+24;
// each set folded to 4 lanes (a[k] + a[k+4]); per lane val + (v2 - val) wf as one FMA
// (wf = (float)frac * (1.0f / src_incr), the plan's table); then the common kernel's
// horizontal sum.  oracle/amx_oracle.c swr_dot_lin is the same sequence.
__device__ __forceinline__ float swr_dot_lin(const float *w, const float *__restrict__ h,
                                             const float *__restrict__ h2, float wf) {
    float a[8], c[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float acc = __builtin_fmaf(w[k], h[k], 0.0f), acc2 = __builtin_fmaf(w[k], h2[k], 0.0f);
#pragma unroll
        for (int q = 8; q < 32; q += 8) {
            acc = __builtin_fmaf(w[k + q], h[k + q], acc);
            acc2 = __builtin_fmaf(w[k + q], h2[k + q], acc2);
        }
        a[k] = acc;
        c[k] = acc2;
    }
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float b = a[k] + a[k + 4], d = (c[k] + c[k + 4]) - b;
        e[k] = __builtin_fmaf(d, wf, b);
    }
    return (e[0] + e[2]) + (e[1] + e[3]);
}

}  // namespace amx
