// amx_ln_dyn.hip -- af_loudnorm's filter frame by frame on one track of C = 2..8 interleaved
// channels: k_ln_dyn<C>, restated from FFmpeg af_loudnorm.c as the oracle does
// (oracle/amx_oracle.c ln_detect_peak, ln_true_peak_limiter, ln_filter_frame, ln_flush; this
// file follows the oracle's structure, not the reverse).  af_loudnorm is a state machine over
// 100 ms frames (the AGC gain of a frame depends on the previous frames' decisions) whose
// true-peak limiter is a state machine over samples, so it runs in order: one workgroup of
// LN_NT threads per track, every thread carrying the scalar state (Gaussian smoothing,
// statistics, limiter state), the per-sample loops shared out over the workgroup:
//   - the ring is [LN_LIMF][C] doubles and every sample index moves in steps of C; the
//     fills, the envelope loops and the output are shared out by SAMPLE (thread t takes
//     ring sample s = i C + c), so their loads and stores stay contiguous for every C;
//   - detect_peak keeps prev_smp, the local-maximum test and the 10-sample look-ahead per
//     channel; the peak value is the largest |sample| of the C channels at the position;
//   - one envelope gain per frame multiplies its C samples; clamp and s16 per sample;
//   - r128_out (read only while above_threshold is 0): libebur128's K filter on one thread
//     per channel, the frame's energy summed in channel order with libebur128's channel
//     weights, unused channels (an LFE) skipped -- the limiter still sees them;
//   - r128_in's statistics (3 s short-term, gated integrated, relative gate) need no C: they
//     read one track's hop energies of this same 192 kHz stream (amx_ln_dev.hpp; a C >= 3
//     track passes the combined ones), the histogram rebuilt in LDS block by block;
//   - af_loudnorm's delta[30] is indexed at run time: it lives in LDS.
// The 192 kHz stream is P = (C + 1) / 2 stereo float planes, one per channel pair, made by
// the stereo upsampler (launch_ln_upsample): channel c is lane c & 1 of plane c >> 1; an
// odd C's last right lane is never read.  A stereo track is its one plane.
// Stereo only (C == 2): the kernel is one step of launch_loudnorm's sequence around the
// parallel form k_lp_* (amx_loudnorm.hip), which says through lp_ctl
// whether it runs at all, resolves the options (lp_dctl) and takes a quiet start back at
// a segment start (lp_recG, lp_D, lp_tstop).  C >= 3 tracks run here from end to end.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md §3.9.
// Floating point: no FMA contraction (the reference's C is compiled that way too,
// -ffp-contract=off in the oracle), so every expression keeps the reference's order.
#include "amx_dev.hpp"
#include "amx_ln_dev.hpp"

#pragma clang fp contract(off)

namespace amx {

template <int C>
struct LnLim {                   // true_peak_limiter state (block-uniform)
    int state, env_cnt, env_index, peak_index, attack_length;
    double gr0, gr1, prev[C];
};

template <int C>
__device__ __forceinline__ int ln_wrap(int i) {
    constexpr int RSZ = C * LN_LIMF;
    while (i >= RSZ) i -= RSZ;
    return i;
}

// channel c of 192 kHz frame j
__device__ __forceinline__ float ln_u(const LnArgs &a, int64_t j, int c) {
    return a.u[(int64_t)(c >> 1) * a.plane + 2 * j + (c & 1)];
}

// detect_peak from output offset `offset` over `count` positions: returns peak_delta
// (-1: none) and sets peak_value, peak_index, prev[].  Groups of LN_NT positions: each
// thread stages one position's C |x| (and threads < 12 the positions after the group: the
// next sample and the 10-sample look-ahead read past a position; the ring always holds
// real samples there); a ballot finds the first position where some channel is a
// candidate with the normal predecessor (the previous sample), and only from there on is
// the scan serial (a candidate that fails the look-ahead keeps the older predecessor, so
// later positions depend on it), every thread stepping it alike.
template <int C>
__device__ __forceinline__ int ln_detect(const double *ring, LnLim<C> &S, int lbi, int offset, int count, bool first,
                         double ceiling, double &peak_value, LnSharedT<C> &L, LnProf &P) {
    constexpr int RSZ = C * LN_LIMF;
    P.n_detect++;
    const int tid = threadIdx.x;
    int index = lbi + (offset * C) + (LN_ATT * C);
    if (index >= RSZ) index -= RSZ;
    if (index < 0) index += RSZ;                      // (never in af_loudnorm's own sequences: a guard)
    if (first) {
#pragma unroll
        for (int c = 0; c < C; c++) S.prev[c] = fabs(ring[index + c - C]);
    }
    for (int base = 0; base < count; base += LN_NT) {
        {
            const int idx = ln_wrap<C>(index + C * (base + tid));
            double av[C], bv[C];
#pragma unroll
            for (int c = 0; c < C; c++) av[c] = fabs(ring[idx + c]);
            if (tid < 12) {
                const int jx = ln_wrap<C>(index + C * (base + LN_NT + tid));
#pragma unroll
                for (int c = 0; c < C; c++) bv[c] = fabs(ring[jx + c]);
            }
            __syncthreads();                          // the previous group's reads are done
#pragma unroll
            for (int c = 0; c < C; c++) L.th[c][tid] = av[c];
            if (tid < 12) {
#pragma unroll
                for (int c = 0; c < C; c++) L.th[c][LN_NT + tid] = bv[c];
            }
            __syncthreads();
        }
        const int n = base + tid;
        const int last = (count - base < LN_NT ? count - base : LN_NT) - 1;
        bool cand = false;
        if (n < count) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double th = L.th[c][tid], nx = L.th[c][tid + 1];
                const double pv = tid == 0 ? S.prev[c] : L.th[c][tid - 1];
                cand |= pv <= th && nx <= th && th > ceiling && n > 0;
            }
        }
        const unsigned long long m = __ballot(cand);
        if ((tid & 63) == 0) L.first[tid >> 6] = m ? (tid + __ffsll((long long)m) - 1) : LN_NT;
        __syncthreads();
        int L0 = LN_NT;
#pragma unroll
        for (int w = 0; w < LN_NW; w++) L0 = L.first[w] < L0 ? L.first[w] : L0;
        if (L0 == LN_NT) {
#pragma unroll
            for (int c = 0; c < C; c++) S.prev[c] = L.th[c][last];
            continue;
        }
        P.n_serial++;
        if (L0 > 0) {
#pragma unroll
            for (int c = 0; c < C; c++) S.prev[c] = L.th[c][L0 - 1];
        }
        for (int k = L0; k <= last; k++) {
            const int nn = base + k;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double t = L.th[c][k], nxt = L.th[c][k + 1];
                if ((S.prev[c] <= t) && (nxt <= t) && (t > ceiling) && (nn > 0)) {
                    bool detected = true;
                    for (int i = 2; i < 12; i++)
                        if (L.th[c][k + i] > t) { detected = false; break; }
                    if (!detected) continue;
                    double mp = 0.0;
#pragma unroll
                    for (int d = 0; d < C; d++) {
                        const double p = L.th[d][k];
                        if (d == 0 || p > mp) mp = p;
                        S.prev[d] = p;
                    }
                    S.peak_index = ln_wrap<C>(index + C * nn);
                    peak_value = mp;
                    return nn;
                }
                S.prev[c] = t;
            }
        }
    }
    return -1;
}

// apply env(i) to the k ring frames from env_index on, one gain per frame over its C
// samples.  As in af_loudnorm, env_index may be the ring size itself (its wrap test is
// `>`, not `>=`): that first frame then lies just past the ring, in the C doubles of
// slack the ring is allocated with (AMX_LN_MC_RING).
template <int C, class F>
__device__ __forceinline__ void ln_env_apply(double *ring, int e0, int k, F env) {
    const int tid = threadIdx.x;
    constexpr int U = 4;
    const int ns = k * C;
    for (int s0 = 0; s0 < ns; s0 += LN_NT * U) {
        int sl[U];
        double r[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int s = s0 + LN_NT * q + tid;
            const int i = s / C, c = s - i * C;
            sl[q] = (i > 0 ? ln_wrap<C>(e0 + C * i) : e0) + c;
            r[q] = s < ns ? ring[sl[q]] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int s = s0 + LN_NT * q + tid;
            if (s < ns) ring[sl[q]] = r[q] * env(s / C);
        }
    }
    __syncthreads();
}

template <int C>
__device__ __forceinline__ int ln_env_end(int e0, int k) {
    constexpr int RSZ = C * LN_LIMF;
    if (k <= 0) return e0;
    int e = e0 + C * (k - 1);
    if (k > 1) e = ln_wrap<C>(e);
    e += C;
    if (e >= RSZ) e -= RSZ;
    return e;
}

// true_peak_limiter: nb output frames from ring position lbi into y (s16 [nb][C])
template <int C>
__device__ __forceinline__ void ln_limiter(double *ring, LnLim<C> &S, int lbi, int nb, bool first, double ceiling,
                           int16_t *y, LnSharedT<C> &L, LnProf &P) {
    constexpr int RSZ = C * LN_LIMF;
    const int tid = threadIdx.x;
    if (first) {
        double mx = 0.0;
        for (int s = tid; s < LN_ATT * C; s += LN_NT) mx = fmax(mx, fabs(ring[s]));
        mx = ln_bmax(mx, L.red);
        if (mx > ceiling) {
            S.gr1 = ceiling / mx;
            S.state = LIM_SUSTAIN_;
            for (int s = tid; s < LN_ATT * C; s += LN_NT) ring[s] *= S.gr1;
            __syncthreads();
        }
    }
    int smp = 0;
    double pv = 0.0;
    do {
        switch (S.state) {
        case LIM_OUT_: {
            const uint64_t t0 = clock64();
            const int pd = ln_detect<C>(ring, S, lbi, smp, nb - smp, first, ceiling, pv, L, P);
            P.detect += clock64() - t0;
            if (pd != -1) {
                S.env_cnt = 0;
                smp += (pd - S.attack_length);
                S.gr0 = 1.;
                S.gr1 = ceiling / pv;
                S.state = LIM_ATTACK_;
                S.env_index = S.peak_index - (S.attack_length * C);
                if (S.env_index < 0) S.env_index += RSZ;
                S.env_index += (S.env_cnt * C);
                if (S.env_index > RSZ) S.env_index -= RSZ;
            } else {
                smp = nb;
            }
            break;
        }
        case LIM_ATTACK_: {
            int k = S.attack_length - S.env_cnt;
            if (k > nb - smp) k = nb - smp;
            if (k < 0) k = 0;
            const int c0 = S.env_cnt, al = S.attack_length;
            const double g0 = S.gr0, g1 = S.gr1;
            const uint64_t t0 = clock64();
            ln_env_apply<C>(ring, S.env_index, k,
                            [&](int i) { return g0 - ((double)(c0 + i) / (al - 1) * (g0 - g1)); });
            P.env += clock64() - t0;
            S.env_index = ln_env_end<C>(S.env_index, k);
            S.env_cnt += k;
            smp += k;
            if (smp < nb) {
                S.env_cnt = 0;
                S.attack_length = LN_ATT;
                S.state = LIM_SUSTAIN_;
            }
            break;
        }
        case LIM_SUSTAIN_: {
            const uint64_t t0 = clock64();
            const int pd = ln_detect<C>(ring, S, lbi, smp, nb, first, ceiling, pv, L, P);
            P.detect += clock64() - t0;
            if (pd == -1) {
                S.state = LIM_RELEASE_;
                S.gr0 = S.gr1;
                S.gr1 = 1.;
                S.env_cnt = 0;
                break;
            }
            const double gain_reduction = ceiling / pv;
            if (gain_reduction < S.gr1) {
                S.state = LIM_ATTACK_;
                S.attack_length = pd;
                if (S.attack_length <= 1) S.attack_length = 2;
                S.gr0 = S.gr1;
                S.gr1 = gain_reduction;
                S.env_cnt = 0;
                break;
            }
            int k = pd;
            if (k > nb - smp) k = nb - smp;
            if (k < 0) k = 0;
            const double g1 = S.gr1;
            const uint64_t t1 = clock64();
            ln_env_apply<C>(ring, S.env_index, k, [&](int) { return g1; });
            P.env += clock64() - t1;
            S.env_index = ln_env_end<C>(S.env_index, k);
            S.env_cnt = k;
            smp += k;
            break;
        }
        default: {   // RELEASE
            const int rl = LN_FR;
            int k = rl - S.env_cnt;
            if (k > nb - smp) k = nb - smp;
            if (k < 0) k = 0;
            const int c0 = S.env_cnt;
            const double g0 = S.gr0, g1 = S.gr1;
            const uint64_t t0 = clock64();
            ln_env_apply<C>(ring, S.env_index, k,
                            [&](int i) { return g0 + (((double)(c0 + i) / (rl - 1)) * (g1 - g0)); });
            P.env += clock64() - t0;
            S.env_index = ln_env_end<C>(S.env_index, k);
            S.env_cnt += k;
            smp += k;
            if (smp < nb) {
                S.env_cnt = 0;
                S.state = LIM_OUT_;
            }
            break;
        }
        }
    } while (smp < nb);
    const uint64_t t_out = clock64();
    constexpr int U = 4;
    const int ns = nb * C;
    for (int s0 = 0; s0 < ns; s0 += LN_NT * U) {
        double r[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int s = s0 + LN_NT * q + tid;
            r[q] = s < ns ? ring[ln_wrap<C>(lbi + s)] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < U; q++) {
            const int s = s0 + LN_NT * q + tid;
            double o = r[q];
            if (fabs(o) > ceiling) o = ceiling * (o < 0 ? -1 : 1);
            if (s < ns) y[s] = ln_s16(o);
        }
    }
    P.out += clock64() - t_out;
}

// libebur128's K filter (direct form) over the frame's clamped output, thread c the
// channel c (r128_out, read only while above_threshold is 0): the frame's energy to every
// thread, the channels added in order with libebur128's weights and the unused ones
// skipped (ebur128_calc_gating_block); DBL_MIN flush at the end as ebur128_filter does
template <int C>
__device__ __forceinline__ double ln_out_energy(const double *ring, int lbi, int nb, double ceiling, const double *kb,
                                const double *ka, double (&kv)[5], double *s_red) {
    const int tid = threadIdx.x;
    double e = 0.0;
    if (tid < C && ebur_weight(C, tid) != 0.0) {
        double v0, v1 = kv[1], v2 = kv[2], v3 = kv[3], v4 = kv[4];     // (scalars: the state stays in registers)
        for (int i = 0; i < nb; i++) {
            const int slot = ln_wrap<C>(lbi + C * i);
            double o = ring[slot + tid];
            if (fabs(o) > ceiling) o = ceiling * (o < 0 ? -1 : 1);
            v0 = o - ka[1] * v1 - ka[2] * v2 - ka[3] * v3 - ka[4] * v4;
            const double yv = kb[0] * v0 + kb[1] * v1 + kb[2] * v2 + kb[3] * v3 + kb[4] * v4;
            e += yv * yv;
            v4 = v3; v3 = v2; v2 = v1; v1 = v0;
        }
        kv[1] = fabs(v1) < 2.2250738585072014e-308 ? 0.0 : v1;
        kv[2] = fabs(v2) < 2.2250738585072014e-308 ? 0.0 : v2;
        kv[3] = fabs(v3) < 2.2250738585072014e-308 ? 0.0 : v3;
        kv[4] = fabs(v4) < 2.2250738585072014e-308 ? 0.0 : v4;
    }
    __syncthreads();
    if (tid < C) s_red[tid] = e;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const double w = ebur_weight(C, c);
        if (w == 0.0) continue;                           // FF_EBUR128_UNUSED
        double cs = s_red[c];
        if (w != 1.0) cs *= w;
        r += cs;
    }
    __syncthreads();
    return r;
}

static_assert(LN_NW >= 8, "ln_out_energy: one s_red slot per channel");

// C == 2, phase 0 (after k_lp_stats): the tracks the parallel form does not start -- the
// < 3 s linear fallback, a quiet start (handed over at the first segment start after
// above_threshold turns 1, lp_ctl[0] = 4); phase 1 (after k_lp_walk): a whole track the
// walker handed back (lp_ctl[0] = 2), frame by frame to the end.  C >= 3: the whole track.
template <int C>
__global__ void __launch_bounds__(LN_NT) k_ln_dyn(LnArgs a0, int phase) {
    constexpr int RSZ = C * LN_LIMF;
    LnArgs a = a0;
    bool walked = false;                                 // handed over by k_lp_walk (summary[13])
    if constexpr (C == 2) {
        if (a0.lp_ctl && a0.lp_ctl[0] != (phase == 0 ? 1 : 2)) return;
        if (a0.lp_dctl) {
            a.offset = a0.lp_dctl[1];
            a.measured_i = a0.lp_dctl[2];
            a.measured_thresh = a0.lp_dctl[3];
        }
        walked = a0.lp_ctl && a0.lp_ctl[0] == 2;
    }
    // what follows summary[0..9]: stereo leaves 14..15 to k_lp_*
    auto summary_tail = [&]() {
        for (int q = 10; q < (C == 2 ? 13 : 16); q++) a.summary[q] = 0.0;
        if constexpr (C == 2) a.summary[13] = walked ? 1.0 : 0.0;
    };
    __shared__ LnSharedT<C> L;
    __shared__ double s_delta[30];                       // af_loudnorm's delta[] (indexed at run time)
    const int tid = threadIdx.x;
    for (int i = tid; i < 1000; i += LN_NT) { L.hist[i] = 0u; L.E[i] = a.energies[i]; }
    for (int i = tid; i < 1001; i += LN_NT) L.B[i] = a.bounds[i];
    if (tid < 30) L.oe[tid] = 0.0;
    __syncthreads();
    const int64_t n = a.n192;
    double *ring = a.ring;
    const double ceiling = a.target_tp;
    LnProf P;
    if (n < LN_FIRST) {
        // the first frame is the whole input: af_loudnorm falls back to LINEAR_MODE with an
        // offset from r128_in's integrated loudness and the largest channel's sample peak
        for (int64_t k = 4; k * LN_FR <= n; k++) ln_add_block(L, a.hops, k);
        double global, rel;
        [[clang::always_inline]] ln_global(L, global, rel);
        const double true_peak = a.peak[0] > a.peak[1] ? a.peak[0] : a.peak[1];
        const double offset = pow(10., (a.target_i - global) / 20.);
        const double offset_tp = true_peak * offset;
        const double off = offset_tp < a.target_tp ? offset : a.target_tp / true_peak;
        for (int64_t s = tid; s < n * C; s += LN_NT) {
            const int64_t j = s / C;
            a.y[s] = ln_s16((double)ln_u(a, j, (int)(s - j * C)) * off);
        }
        if (tid == 0) {
            a.summary[0] = 1.0;
            a.summary[1] = off;
            if constexpr (C != 2)
                for (int q = 2; q < 10; q++) a.summary[q] = 0.0;
            summary_tail();
        }
        return;
    }
    if (tid < C) ring[RSZ + tid] = 0.0;                  // the slack behind the ring (ln_env_apply)
    // ---- FIRST frame (3 s)
    for (int64_t k = 4; k <= LN_FIRST / LN_FR; k++) ln_add_block(L, a.hops, k);
    int index = 1, above;
    double prev_delta;
    {
        const double shortterm = ln_shortterm(a.hops, LN_FIRST / LN_FR, L.red);
        double env_shortterm;
        if (shortterm < a.measured_thresh) {
            above = 0;
            env_shortterm = shortterm <= -70. ? 0. : a.target_i - a.measured_i;
        } else {
            above = 1;
            env_shortterm = shortterm <= -70. ? 0. : a.target_i - shortterm;
        }
        const double d = pow(10., env_shortterm / 20.);
        if (tid < 30) s_delta[tid] = d;
        prev_delta = d;
        for (int s = tid; s < RSZ; s += LN_NT) {
            const int i = s / C;
            ring[s] = (double)ln_u(a, i, s - i * C) * d * a.offset;
        }
    }
    __syncthreads();
    LnLim<C> S;
    S.state = LIM_OUT_;
    S.env_cnt = S.env_index = S.peak_index = 0;
    S.attack_length = LN_ATT;
    S.gr0 = S.gr1 = 0.0;
#pragma unroll
    for (int c = 0; c < C; c++) S.prev[c] = 0.0;
    int lbi = 0;
    double kv[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int oe_i = 0;
    auto out_feed = [&](int nb) {                        // r128_out, only while needed
        const uint64_t t0 = clock64();
        const double e = ln_out_energy<C>(ring, lbi, nb, ceiling, a.kb, a.ka, kv, L.red);
        if (tid == 0) L.oe[oe_i] = e;
        oe_i = oe_i + 1 < 30 ? oe_i + 1 : 0;
        __syncthreads();
        P.feed += clock64() - t0;
    };
    int64_t out_pos = 0;
    ln_limiter<C>(ring, S, lbi, LN_FR, true, ceiling, a.y, L, P);
    if (above == 0) out_feed(LN_FR);
    out_pos = LN_FR;
    int64_t R = LN_LIMF, Pin = LN_FIRST;
    auto gauss = [&](int idx) {
        double r = 0.;
        idx = idx - 10 > 0 ? idx - 10 : idx + 20;
#pragma unroll
        for (int i = 0; i < 21; i++) r += s_delta[((idx + i) < 30) ? (idx + i) : (idx + i - 30)] * a.weights[i];
        return r;
    };
    [[maybe_unused]] int ho_f = -1, ho_k = -1;           // hand-over frame / segment (stereo quiet start)
    // ---- INNER frames (100 ms)
    while (Pin < n) {
        const int t_in = (int)((Pin - LN_FIRST) / LN_FR);     // this INNER frame
        if constexpr (C == 2) {
            if (phase == 0 && t_in >= a0.lp_tstop) return;    // (a shard: past rank 0's frames)
        }
        const int nb = (int)(n - Pin < LN_FR ? n - Pin : LN_FR);
        const uint64_t t_fill = clock64();
        const double gain = gauss(index + 10 < 30 ? index + 10 : index + 10 - 30);
        const double gain_next = gauss(index + 11 < 30 ? index + 11 : index + 11 - 30);
        {
            constexpr int U = 4;
            const int ns = nb * C;
            for (int s0 = 0; s0 < ns; s0 += LN_NT * U) {
                float v[U];
#pragma unroll
                for (int q = 0; q < U; q++) {
                    const int s = s0 + LN_NT * q + tid;
                    const int i = s / C;
                    v[q] = s < ns ? ln_u(a, R + i, s - i * C) : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < U; q++) {
                    const int s = s0 + LN_NT * q + tid;
                    if (s < ns) {
                        const int i = s / C;
                        const double g = gain + (((double)i / nb) * (gain_next - gain));
                        ring[ln_wrap<C>(lbi + s)] = (double)v[q] * g * a.offset;
                    }
                }
            }
        }
        __syncthreads();
        lbi = ln_wrap<C>(lbi + C * nb);
        {
            const int sub = (LN_FR - nb) * C;
            lbi = lbi + sub < RSZ ? lbi + sub : lbi + sub - RSZ;
        }
        R += nb;
        Pin += nb;
        P.fill += clock64() - t_fill;
        ln_limiter<C>(ring, S, lbi, nb, false, ceiling, a.y + C * out_pos, L, P);
        if (above == 0) out_feed(nb);
        const uint64_t t_stats = clock64();
        out_pos += nb;
        // r128_in after this frame: a full frame ends on hop Pin / 19200 (one new block)
        const int64_t hk = Pin / LN_FR;
        if (nb == LN_FR) ln_add_block(L, a.hops, hk);
        double global, relative_threshold;
        [[clang::always_inline]] ln_global(L, global, relative_threshold);   // (a call keeps both results in scratch)
        const double shortterm = ln_shortterm(a.hops, hk, L.red);
        if (above == 0) {
            if (shortterm > a.measured_thresh) prev_delta *= 1.0058;
            double so = 0.0;
            for (int q = 0; q < 30; q++) so += L.oe[q];
            const double shortterm_out = 10 * log10(so / (double)LN_FIRST) - 0.691;
            if (shortterm_out >= a.target_i) above = 1;
        }
        double dnew;
        if (shortterm < relative_threshold || shortterm <= -70. || above == 0) {
            dnew = prev_delta;
        } else {
            const double env_global = fabs(shortterm - global) < (a.target_lra / 2.)
                                          ? shortterm - global
                                          : (a.target_lra / 2.) * ((shortterm - global) < 0 ? -1 : 1);
            const double env_shortterm = a.target_i - shortterm;
            dnew = pow(10., (env_global + env_shortterm) / 20.);
        }
        __syncthreads();                                 // every thread has read this frame's gains
        if (tid == 0) s_delta[index] = dnew;
        __syncthreads();
        prev_delta = dnew;
        index = index + 1 < 30 ? index + 1 : 0;
        P.stats += clock64() - t_stats;
        if constexpr (C == 2) {
            if (a0.lp_D && tid == 0) a0.lp_D[t_in] = dnew;
            if (phase == 0 && a0.lp_recG && above && ho_f < 0) {
                // from here the deltas follow r128_in alone: hand over at the next segment
                // start (frame 1 + k Fs, k <= J) -- after frame ho_f - 1, before ho_f's fill
                const int phi = t_in + 1;
                int k = (phi + a0.lp_Fs - 1) / a0.lp_Fs;
                if (k < 1) k = 1;
                if (k <= a0.lp_J) {
                    ho_k = k;
                    ho_f = 1 + k * a0.lp_Fs;
                } else {
                    ho_f = 0;                                      // none left: run to the end
                }
            }
            if (ho_f > 0 && t_in + 1 == ho_f - 1) {
                // the state at frame ho_f's start, as k_lp_snapshot records it: the limiter
                // scalars (envelope slot in frames) and the 2048 ring slots from the frame's
                // first output position (19200 ho_f; INNER slot = position mod the ring)
                double *rec = a0.lp_recG + (int64_t)ho_k * AMX_LN_REC;
                if (tid == 0) {
                    rec[0] = S.state;
                    rec[1] = S.env_cnt;
                    rec[2] = S.env_index / 2;
                    rec[3] = S.attack_length;
                    rec[4] = S.gr0;
                    rec[5] = S.gr1;
                    rec[6] = ho_f;
                    rec[7] = 0.0;
                    a0.lp_ctl[0] = 4;
                    a0.lp_ctl[4] = ho_k;
                    a0.lp_ctl[5] = ho_f;
                }
                const int s0 = (int)(((int64_t)LN_FR * ho_f) % LN_LIMF);
                for (int j = tid; j < AMX_LN_WIN; j += LN_NT) {
                    const int sl = s0 + j < LN_LIMF ? s0 + j : s0 + j - LN_LIMF;
                    rec[16 + 2 * j] = ring[2 * sl];
                    rec[17 + 2 * j] = ring[2 * sl + 1];
                }
                return;
            }
        }
    }
    // ---- FINAL frame (flush_frame: the last 3 s less one frame, re-read)
    {
        const int nbf = LN_FIRST - LN_FR;                // (buf_size - prev_nb) - (100 ms - prev_nb)
        const int64_t S0 = n - nbf;                      // its first frame in the stream
        const double gain = gauss(index + 10 < 30 ? index + 10 : index + 10 - 30);
        for (int s = tid; s < RSZ; s += LN_NT) {
            const int i = s / C;
            ring[s] = (double)ln_u(a, S0 + i, s - i * C) * gain * a.offset;
        }
        __syncthreads();
        lbi = 0;
        int64_t src = LN_LIMF;
        for (int it = 0; it < nbf / LN_FR; it++) {
            ln_limiter<C>(ring, S, lbi, LN_FR, false, ceiling, a.y + C * out_pos, L, P);
            for (int s = tid; s < LN_FR * C; s += LN_NT) {
                const int i = s / C;
                const bool in = src + i < nbf;
                ring[ln_wrap<C>(lbi + s)] = in ? (double)ln_u(a, S0 + src + i, s - i * C) * gain * a.offset : 0.;
            }
            __syncthreads();
            src += LN_FR;
            lbi = ln_wrap<C>(lbi + C * LN_FR);
            out_pos += LN_FR;
        }
    }
    if (tid == 0) {
        a.summary[0] = 0.0;
        a.summary[1] = (double)above;
        a.summary[2] = (double)P.fill;
        a.summary[3] = (double)P.detect;
        a.summary[4] = (double)P.env;
        a.summary[5] = (double)P.out;
        a.summary[6] = (double)P.stats;
        a.summary[7] = (double)P.feed;
        a.summary[8] = (double)P.n_detect;
        a.summary[9] = (double)P.n_serial;
        summary_tail();
    }
}

hipError_t launch_ln_dyn(const LnArgs &a, int C, int phase, hipStream_t st) {
    switch (C) {
#define LN_DYN(CC) \
    case CC: hipLaunchKernelGGL(k_ln_dyn<CC>, dim3(1), dim3(LN_NT), 0, st, a, phase); break;
    LN_DYN(2) LN_DYN(3) LN_DYN(4) LN_DYN(5) LN_DYN(6) LN_DYN(7) LN_DYN(8)
#undef LN_DYN
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace amx
