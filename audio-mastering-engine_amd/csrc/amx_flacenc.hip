// amx_flacenc.hip -- the mastered int16 track -> a FLAC frame stream, on the device.
//
// The reference's last ffmpeg command writes output_file with the container its
// extension names (audio_mastering_engine.py:223): a .flac master.  FLAC is lossless, so
// any conforming stream that decodes to the mastered samples carries the same audio;
// this encoder fixes its search space so that every subframe's size
// has one right answer:
//   CONSTANT (all samples equal), VERBATIM, FIXED order 0..min(4, block);
//   residual coding method 0 (4-bit Rice parameters), k 0..14, no escapes, partition
//   order p 0..min(6, ctz(block)) with (block >> p) >= order;
//   stereo: the smallest of independent, left/side, side/right, mid/side;
//   with lpc_order M > 0 also LPC of order 1..min(M, block - 1): 12-bit coefficients from
//   an integer Welch window, an exact integer autocorrelation and Levinson in fp64 in a
//   fixed operation order (DESIGN.md §3.10 "LPC"), every folded residual below 2^22.
// The kernels (RFC 9639 for the bitstream):
//   k_flac_analyze  one workgroup per (frame, channel candidate): the exact minimum over
//                   the search space and the choice that reaches it (one pass over the
//                   samples, then one wave per predictor order)
//   k_flac_lpc      (lpc_order > 0 only) one workgroup per (frame, channel candidate): the
//                   LPC orders' exact sizes; the best replaces the analysis' choice when
//                   it is strictly smaller
//   k_flac_place    one workgroup: the channel assignment, each frame's byte length and
//                   the exclusive scan of the lengths (the frames' offsets)
//   k_flac_pack     one workgroup per frame: the frame staged in pre-zeroed LDS (codes
//                   ORed in at the bit offsets a prefix sum of the code lengths gives),
//                   CRC-8 / CRC-16, copied out with plain vector stores
// Every output word is written by exactly one kernel store: nothing is zeroed first and
// the bytes do not depend on the order the lanes run in.
#include "amx_internal.hpp"

namespace amx {

#define FE_NT 256            // lanes of an analysis / pack workgroup
#define FE_MAXP 64           // finest partitions (partition order 6)
#define FE_NK 15             // Rice parameters 0..14
#define FE_CAP 0x3fffffffu   // sums saturate here: far above any VERBATIM size, never the minimum
#define FE_MAXO 8            // LPC orders 1..8
#define FE_LPC0 32           // cinfo / subframe type of LPC order o: FE_LPC0 + o - 1

// workspace layout (amx_flac_encode_size): offsets i64 [nf], assign u32 [nf],
// cbits u32 [nf][ncand], cinfo u32 [nf][ncand], ck u8 [nf][ncand][64]
struct FeWs {
    int64_t *off;
    uint32_t *assign, *cbits, *cinfo;
    uint8_t *ck;
};
// appended with lpc_order > 0: lq i16 [nf][ncand][8] (the coefficients), lsh u32 [nf][ncand]
// (the shift), read only for the slots whose cinfo names an LPC subframe.  A structure of
// its own: the lpc_order == 0 kernels keep their arguments.
struct FeLpcWs {
    int16_t *lq;
    uint32_t *lsh;
};
__host__ __device__ static inline FeWs fe_ws(void *ws, int64_t nf, int ncand) {
    FeWs w;
    uint8_t *p = reinterpret_cast<uint8_t *>(ws);
    w.off = reinterpret_cast<int64_t *>(p);
    p += nf * 8;
    w.assign = reinterpret_cast<uint32_t *>(p);
    p += nf * 4;
    w.cbits = reinterpret_cast<uint32_t *>(p);
    p += nf * ncand * 4;
    w.cinfo = reinterpret_cast<uint32_t *>(p);
    p += nf * ncand * 4;
    w.ck = p;
    return w;
}
__host__ __device__ static inline FeLpcWs fe_lpc_ws(const FeWs &ws, int64_t nf, int ncand) {
    FeLpcWs w;
    uint8_t *p = ws.ck + nf * ncand * FE_MAXP;
    w.lq = reinterpret_cast<int16_t *>(p);
    p += nf * ncand * FE_MAXO * 2;
    w.lsh = reinterpret_cast<uint32_t *>(p);
    return w;
}

// the sample of channel candidate `cand` at frame i: the file's channel, or for stereo
// 0 L, 1 R, 2 mid = (L + R) >> 1, 3 side = L - R (17 bits)
__device__ __forceinline__ int fe_sample(const int16_t *__restrict__ pcm, int64_t i, int C, int cand) {
    if (C != 2) return pcm[i * C + cand];
    const int l = pcm[2 * i], r = pcm[2 * i + 1];
    return cand == 0 ? l : cand == 1 ? r : cand == 2 ? ((l + r) >> 1) : (l - r);
}

// LPC residual of order o at i >= o: coefficients q[0 .. 8) (q[0] multiplies the sample just
// before), shift sh.  Coefficients (12 bits) and samples (17) fit the 24-bit multiply.
__device__ __forceinline__ int fe_lpc_residual(const int *s, int i, int o, const int *q, int sh) {
    int acc = 0;
#pragma unroll
    for (int j = 0; j < FE_MAXO; j++)
        if (j < o) acc += __mul24(q[j], s[i - 1 - j]);
    return s[i] - (acc >> sh);
}
// FIXED predictor residual of order o at i >= o
__device__ __forceinline__ int fe_residual(const int *s, int i, int o) {
    switch (o) {
    case 0: return s[i];
    case 1: return s[i] - s[i - 1];
    case 2: return s[i] - 2 * s[i - 1] + s[i - 2];
    case 3: return s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
    default: return s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    }
}
__device__ __forceinline__ uint32_t fe_fold(int r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// ------------------------------------------------------------------ analysis
// cinfo: type (0 CONSTANT, 1 VERBATIM, 8 + o FIXED) | partition order << 8
//
// Phase 1, all lanes: tpp = 256 / P lanes share a finest partition (P = 2^pmax of them);
// one pass over the samples forms sum(u >> k) for the five orders and fifteen k in
// registers, the lanes of a partition add up by shuffles and the sums land in LDS.
// Phase 2, one wave per order: lane j holds partition j's fifteen sums; each partition
// order's cost is a min over k and a wave sum, the next coarser one's sums are pairwise
// adds by shuffle -- no LDS, no barrier.  Phase 3: the smallest candidate.
// Sums saturate (FE_TCAP per lane, FE_CAP per partition): a saturated sum is above
// 2^22 bits, more than any VERBATIM subframe, so it is never part of the minimum and every
// sum that can be is exact.
#define FE_TCAP (1u << 22)

// Phase 2 for one predictor order o, run by one whole wave: Srow holds the 2^pmax finest
// partitions' fifteen sums, head the subframe's bits before the partitions' codes.  The
// smallest size over the partition orders goes to best[0], its partition order to best[1]
// and its Rice parameters to kout.
__device__ __forceinline__ void fe_partition_search(const uint32_t *Srow, int lane, int n, int pmax, int o,
                                                    uint32_t head, uint8_t *kout, uint32_t *best) {
    const int P = 1 << pmax;
    uint32_t S[FE_NK];
#pragma unroll
    for (int k = 0; k < FE_NK; k++) S[k] = lane < P ? Srow[lane * FE_NK + k] : 0u;
    uint32_t btot = 0xffffffffu, bk = 0;
    int bp = 0;
    for (int p = pmax; p >= 0; p--) {
        const int stride = 1 << (pmax - p), np = n >> p;
        const bool active = lane < P && (lane & (stride - 1)) == 0;
        const uint32_t nj = (uint32_t)(np - (lane == 0 ? o : 0));   // (np < o: the order is skipped)
        uint32_t m = 0xffffffffu, mk = 0;
#pragma unroll
        for (int k = 0; k < FE_NK; k++) {
            const uint32_t c = nj * (uint32_t)(k + 1) + S[k];
            if (c < m) { m = c; mk = k; }
        }
        uint32_t c = active && np >= o ? 4u + m : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t x = c + __shfl_xor(c, d);
            c = x < 0x7fffffffu ? x : 0x7fffffffu;
        }
        const uint32_t tot = head + c;
        if (np >= o && tot < btot) { btot = tot; bp = p; bk = mk; }
        if (p > 0) {
#pragma unroll
            for (int k = 0; k < FE_NK; k++) {
                const uint32_t x = S[k] + __shfl_down(S[k], (unsigned)stride);
                S[k] = x < FE_CAP ? x : FE_CAP;
            }
        }
    }
    const int sb = 1 << (pmax - bp);
    if (lane < P && (lane & (sb - 1)) == 0) kout[lane >> (pmax - bp)] = (uint8_t)bk;
    if (lane == 0) { best[0] = btot; best[1] = (uint32_t)bp; }
}

__global__ void __launch_bounds__(FE_NT) k_flac_analyze(const int16_t *__restrict__ pcm, int64_t frames, int C,
                                                        int B, int ncand, FeWs ws) {
    __shared__ int s[4608];
    __shared__ uint32_t Sall[5][FE_MAXP * FE_NK];
    __shared__ uint32_t obest[5][2];
    __shared__ uint8_t ordk[5][FE_MAXP];
    __shared__ int differ;

    const int t = threadIdx.x;
    const int64_t f = blockIdx.x / ncand;
    const int cand = (int)(blockIdx.x - f * ncand);
    const int64_t i0 = f * B;
    const int n = (int)(frames - i0 < B ? frames - i0 : B);
    const int w = (C == 2 && cand == 3) ? 17 : 16;
    if (t == 0) differ = 0;
    for (int i = t; i < 5 * FE_MAXP * FE_NK; i += FE_NT) (&Sall[0][0])[i] = 0;
    for (int i = t; i < n; i += FE_NT) s[i] = fe_sample(pcm, i0 + i, C, cand);
    __syncthreads();
    for (int i = t; i < n; i += FE_NT)
        if (s[i] != s[0]) differ = 1;

    const int pmax = min(6, __ffs(n) - 1);
    const int P = 1 << pmax, plen = n >> pmax, tpp = FE_NT / P;
    const int omax = n < 4 ? n : 4;
    {
        uint32_t acc[5][FE_NK];
#pragma unroll
        for (int o = 0; o < 5; o++)
#pragma unroll
            for (int k = 0; k < FE_NK; k++) acc[o][k] = 0;
        const int j = t / tpp, q = t - j * tpp;
        for (int i = j * plen + q; i < (j + 1) * plen; i += tpp) {
            // the five residuals at i as successive differences (those with i < o: no code)
            const int x0 = s[i], x1 = s[max(i - 1, 0)], x2 = s[max(i - 2, 0)], x3 = s[max(i - 3, 0)],
                      x4 = s[max(i - 4, 0)];
            const int a1 = x0 - x1, b1 = x1 - x2, c1 = x2 - x3, d1 = x3 - x4;
            const int a2 = a1 - b1, b2 = b1 - c1, c2 = c1 - d1;
            const int a3 = a2 - b2, b3 = b2 - c2;
            const int r[5] = {x0, a1, a2, a3, a3 - b3};
#pragma unroll
            for (int o = 0; o < 5; o++) {
                const uint32_t u = i >= o ? fe_fold(r[o]) : 0u;
#pragma unroll
                for (int k = 0; k < FE_NK; k++) acc[o][k] += u >> k;
            }
        }
        const int width = tpp < 64 ? tpp : 64;
#pragma unroll
        for (int o = 0; o < 5; o++)
#pragma unroll
            for (int k = 0; k < FE_NK; k++) {
                uint32_t v = acc[o][k] < FE_TCAP ? acc[o][k] : FE_TCAP;
                for (int d = 1; d < width; d <<= 1) v += __shfl_xor(v, d);
                if ((t & (width - 1)) == 0) atomicAdd(&Sall[o][j * FE_NK + k], v);
            }
    }
    __syncthreads();

    const int lane = t & 63;
    for (int o = t >> 6; o <= omax; o += FE_NT / 64) {
        fe_partition_search(Sall[o], lane, n, pmax, o, 8u + (uint32_t)(o * w) + 6u, ordk[o], obest[o]);
    }
    __syncthreads();

    uint32_t best = 8u + (uint32_t)n * w, info = 1;                 // VERBATIM
    if (!differ && 8u + w < best) { best = 8u + w; info = 0; }      // CONSTANT
    int bo = -1, bp = 0;
    for (int o = 0; o <= omax; o++)
        if (obest[o][0] < best) { best = obest[o][0]; bo = o; bp = (int)obest[o][1]; }
    if (bo >= 0) info = (uint32_t)(8 + bo) | ((uint32_t)bp << 8);
    const int64_t slot = (int64_t)blockIdx.x;
    if (t == 0) {
        ws.cbits[slot] = best;
        ws.cinfo[slot] = info;
    }
    if (t < FE_MAXP) ws.ck[slot * FE_MAXP + t] = bo >= 0 && t < (1 << bp) ? ordk[bo][t] : (uint8_t)0;
}

// ------------------------------------------------------------------ LPC
// One workgroup per (frame, candidate), after k_flac_analyze.  The predictor of every order
// is derived exactly as DESIGN.md §3.10 "LPC" fixes it, so that a host model recomputes the
// same integers: an integer Welch window, the autocorrelation in exact int64 sums (any
// order of adding gives the same R), Levinson and the quantisation in fp64 with every
// operation a correctly rounded +, -, *, / (the build has -ffp-contract=off), run by wave 0,
// every lane alike.  Then k_flac_analyze's phases 1 and 2, four orders at a time: the residuals'
// sum(u >> k) per finest partition, one wave per order for the partition search.  An order
// with a folded residual of FE_TCAP or more is no candidate.  The smallest candidate
// replaces the slot's choice only when it is strictly below it; nothing is written
// otherwise, and every word k_flac_pack reads of lq / lsh was written here.
#define FE_LB 4              // orders per batch: 4 x 15 accumulators in registers
// Phase 1 of k_flac_lpc for the orders ob + 1 .. ob + FE_LB: this lane's
// samples of its finest partition, the orders' residuals, sum(u >> k) in registers, added
// up over the partition's lanes into Sall.  An order that is no candidate adds zeros.
__device__ __forceinline__ void fe_lpc_sums(const int *s, uint32_t *Sall, const int (*qs)[FE_MAXO], const int *shs,
                                            const int *cand_ok, int *toobig, int ob, int Mp, int t, int plen,
                                            int tpp) {
    int cq[FE_LB][FE_MAXO], csh[FE_LB];
    bool cok[FE_LB];
#pragma unroll
    for (int a = 0; a < FE_LB; a++) {
        cok[a] = ob + a < Mp && cand_ok[ob + a];
        csh[a] = cok[a] ? shs[ob + a] : 0;
#pragma unroll
        for (int j = 0; j < FE_MAXO; j++) cq[a][j] = cok[a] ? qs[ob + a][j] : 0;
    }
    uint32_t acc[FE_LB][FE_NK], umax[FE_LB];
#pragma unroll
    for (int a = 0; a < FE_LB; a++) {
        umax[a] = 0;
#pragma unroll
        for (int k = 0; k < FE_NK; k++) acc[a][k] = 0;
    }
    // (each partition's lanes start rot samples in and wrap: with every partition starting at
    // its first sample, a wave's reads lie a partition length apart, 64 words in a block of 4096)
    const int j = t / tpp, q = t - j * tpp, rot = (j * tpp) % plen;
    for (int m = q; m < plen; m += tpp) {
        const int i = j * plen + (m + rot < plen ? m + rot : m + rot - plen);
        int x[FE_MAXO + 1];
#pragma unroll
        for (int d = 0; d <= FE_MAXO; d++) x[d] = s[max(i - d, 0)];
#pragma unroll
        for (int a = 0; a < FE_LB; a++) {
            // (taps beyond the order have coefficient 0; |sum| <= 8 * 2048 * 65535 < 2^30)
            int sum = 0;
#pragma unroll
            for (int d = 0; d < FE_MAXO; d++) sum += __mul24(cq[a][d], x[d + 1]);
            const uint32_t u = cok[a] && i >= ob + a + 1 ? fe_fold(x[0] - (sum >> csh[a])) : 0u;
            umax[a] = u > umax[a] ? u : umax[a];
#pragma unroll
            for (int k = 0; k < FE_NK; k++) acc[a][k] += u >> k;
        }
    }
    const int width = tpp < 64 ? tpp : 64;
#pragma unroll
    for (int a = 0; a < FE_LB; a++) {
        if (umax[a] >= FE_TCAP) toobig[ob + a] = 1;
#pragma unroll
        for (int k = 0; k < FE_NK; k++) {
            uint32_t v = acc[a][k] < FE_TCAP ? acc[a][k] : FE_TCAP;
            for (int d = 1; d < width; d <<= 1) v += __shfl_xor(v, d);
            if ((t & (width - 1)) == 0) atomicAdd(&Sall[a * FE_MAXP * FE_NK + j * FE_NK + k], v);
        }
    }
}

__global__ void __launch_bounds__(FE_NT) k_flac_lpc(const int16_t *__restrict__ pcm, int64_t frames, int C, int B,
                                                    int ncand, int M, FeWs ws, FeLpcWs lw) {
    __shared__ int s[4608];
    __shared__ int buf[4608];                       // the windowed samples, then the batch's sums
    __shared__ long long Rw[FE_NT / 64][FE_MAXO + 1];
    __shared__ int qs[FE_MAXO][FE_MAXO];
    __shared__ int shs[FE_MAXO], cand_ok[FE_MAXO], toobig[FE_MAXO];
    __shared__ uint32_t obest[FE_MAXO][2];
    __shared__ uint8_t ordk[FE_MAXO][FE_MAXP];
    int *xw = buf;
    uint32_t *Sall = reinterpret_cast<uint32_t *>(buf);   // [FE_LB][FE_MAXP * FE_NK]

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t slot = (int64_t)blockIdx.x;
    const int64_t f = slot / ncand;
    const int cand = (int)(slot - f * ncand);
    const int64_t i0 = f * B;
    const int n = (int)(frames - i0 < B ? frames - i0 : B);
    const int w = (C == 2 && cand == 3) ? 17 : 16;
    const int Mp = M < n - 1 ? M : n - 1;
    const uint32_t current = ws.cbits[slot];        // (read before anything here writes it)
    if (Mp < 1) return;

    if (t < FE_MAXO) { cand_ok[t] = 0; toobig[t] = 0; obest[t][0] = 0xffffffffu; obest[t][1] = 0; }
    // W[i] = 1020 (i + 1) (n - i) / (n + 1)^2, floored.  Numerator (< 2^33) and denominator
    // (< 2^25) are exact doubles and a quotient that is no integer lies at least 2^-25 from
    // one, far more than the correctly rounded division's error: the floor is the integer's.
    const double den = (double)((n + 1) * (n + 1));
    for (int i = t; i < n; i += FE_NT) {
        const int x = fe_sample(pcm, i0 + i, C, cand);
        const int win = (int)(1020.0 * (double)((i + 1) * (n - i)) / den);
        s[i] = x;
        xw[i] = x * win;                            // |x| <= 65535, win <= 255: below 2^24
    }
    __syncthreads();

    // R[l] = sum xw[i] xw[i - l]: products below 2^48, at most 4608 of them
    long long R[FE_MAXO + 1];
#pragma unroll
    for (int l = 0; l <= FE_MAXO; l++) R[l] = 0;
    for (int i = t; i < n; i += FE_NT) {
        const long long a = xw[i];
#pragma unroll
        for (int l = 0; l <= FE_MAXO; l++)
            if (l <= Mp && i >= l) R[l] += a * (long long)xw[i - l];
    }
#pragma unroll
    for (int l = 0; l <= FE_MAXO; l++) {
        long long v = R[l];
        for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
        if (lane == 0) Rw[wv][l] = v;
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l <= FE_MAXO; l++) R[l] = Rw[0][l] + Rw[1][l] + Rw[2][l] + Rw[3][l];
    if (R[0] == 0) return;                          // (the same R in every lane)

    // Levinson and the quantisation of every order: wave 0 alone (the other waves' SIMDs are
    // free for other workgroups meanwhile), the same in each of its lanes; lane 0 stores
    if (wv == 0) {
        double Rf[FE_MAXO + 1], lpc[FE_MAXO], nw[FE_MAXO];
#pragma unroll
        for (int l = 0; l <= FE_MAXO; l++) Rf[l] = (double)R[l];
#pragma unroll
        for (int j = 0; j < FE_MAXO; j++) lpc[j] = 0.0;
        double err = Rf[0];
        bool alive = true;
#pragma unroll
        for (int i = 0; i < FE_MAXO; i++) {
            if (i < Mp && alive) {
                double acc = Rf[i + 1];
#pragma unroll
                for (int j = 0; j < i; j++) acc = acc - lpc[j] * Rf[i - j];
                const double k = acc / err;
#pragma unroll
                for (int j = 0; j < i; j++) nw[j] = lpc[j] - k * lpc[i - 1 - j];
                nw[i] = k;
#pragma unroll
                for (int j = 0; j <= i; j++) lpc[j] = nw[j];
                err = err * (1.0 - k * k);
                if (!(err > 0.0)) alive = false;    // this order still counts, higher ones do not

                // 12-bit coefficients: the largest shift that keeps them within 2047, error feedback
                bool ok = true;
                double cmax = 0.0;
#pragma unroll
                for (int j = 0; j <= i; j++) {
                    const double a = fabs(lpc[j]);
                    if (!(a <= 2047.0)) ok = false;
                    if (a > cmax) cmax = a;
                }
                if (cmax == 0.0) ok = false;
                int sh = -1;
                for (int e = 15; e >= 0; e--)
                    if (sh < 0 && cmax * (double)(1 << e) <= 2047.0) sh = e;
                if (sh < 0) ok = false;
                if (ok) {
                    const double scale = (double)(1 << sh);
                    double e = 0.0;
#pragma unroll
                    for (int j = 0; j <= i; j++) {
                        e = e + lpc[j] * scale;
                        int q = (int)floor(e + 0.5);
                        q = q < -2048 ? -2048 : q > 2047 ? 2047 : q;
                        e = e - (double)q;
                        if (t == 0) qs[i][j] = q;
                    }
                    if (t == 0) {
#pragma unroll
                        for (int j = i + 1; j < FE_MAXO; j++) qs[i][j] = 0;
                        shs[i] = sh;
                        cand_ok[i] = 1;
                    }
                }
            }
        }
    }

    const int pmax = min(6, __ffs(n) - 1);
    const int P = 1 << pmax, plen = n >> pmax, tpp = FE_NT / P;
    for (int ob = 0; ob < Mp; ob += FE_LB) {
        __syncthreads();                            // xw / the last batch's sums are done with; qs is there
        for (int i = t; i < FE_LB * FE_MAXP * FE_NK; i += FE_NT) Sall[i] = 0;
        __syncthreads();
        fe_lpc_sums(s, Sall, qs, shs, cand_ok, toobig, ob, Mp, t, plen, tpp);
        __syncthreads();
        const int o = ob + wv + 1;                  // one wave per order of the batch
        if (o <= Mp && cand_ok[o - 1] && !toobig[o - 1])
            fe_partition_search(Sall + wv * FE_MAXP * FE_NK, lane, n, pmax, o,
                                8u + (uint32_t)(o * w) + 4u + 5u + 12u * (uint32_t)o + 6u, ordk[o - 1],
                                obest[o - 1]);
    }
    __syncthreads();

    uint32_t best = current;
    int bo = 0;
    for (int o = 1; o <= Mp; o++)
        if (cand_ok[o - 1] && !toobig[o - 1] && obest[o - 1][0] < best) { best = obest[o - 1][0]; bo = o; }
    if (bo == 0) return;
    const int bp = (int)obest[bo - 1][1];
    if (t == 0) {
        ws.cbits[slot] = best;
        ws.cinfo[slot] = (uint32_t)(FE_LPC0 + bo - 1) | ((uint32_t)bp << 8);
        lw.lsh[slot] = (uint32_t)shs[bo - 1];
    }
    if (t < FE_MAXO) lw.lq[slot * FE_MAXO + t] = (int16_t)qs[bo - 1][t];
    if (t < FE_MAXP) ws.ck[slot * FE_MAXP + t] = t < (1 << bp) ? ordk[bo - 1][t] : (uint8_t)0;
}

// ------------------------------------------------------------------ frame header
// sample-rate code of the frame header and its extra bytes (0: from STREAMINFO)
__host__ __device__ static inline int fe_rate_code(int fs, int *extra_bytes, int *extra_val) {
    *extra_bytes = 0;
    *extra_val = 0;
    switch (fs) {
    case 88200: return 1;
    case 176400: return 2;
    case 192000: return 3;
    case 8000: return 4;
    case 16000: return 5;
    case 22050: return 6;
    case 24000: return 7;
    case 32000: return 8;
    case 44100: return 9;
    case 48000: return 10;
    case 96000: return 11;
    default: break;
    }
    if (fs < 65536) { *extra_bytes = 2; *extra_val = fs; return 13; }
    // (below 655 350: tens of Hz up to 65 534, the all-ones value is left alone)
    if (fs % 10 == 0 && fs < 655350) { *extra_bytes = 2; *extra_val = fs / 10; return 14; }
    return 0;
}
__host__ __device__ static inline int fe_block_code(int n, int *extra_bytes) {
    *extra_bytes = 0;
    if (n == 192) return 1;
    for (int c = 2; c <= 5; c++)
        if (n == 576 << (c - 2)) return c;
    for (int c = 8; c <= 15; c++)
        if (n == 256 << (c - 8)) return c;
    if (n <= 256) { *extra_bytes = 1; return 6; }
    *extra_bytes = 2;
    return 7;
}
// the frame number, coded UTF-8 style (up to 36 bits, 7 bytes)
__host__ __device__ static inline int fe_utf8(uint64_t v, uint8_t *out) {
    if (v < 0x80) { out[0] = (uint8_t)v; return 1; }
    int nb = 2;
    while (nb < 7 && v >= (1ull << (5 * nb + 1))) nb++;
    for (int i = nb - 1; i >= 1; i--) { out[i] = (uint8_t)(0x80 | (v & 0x3f)); v >>= 6; }
    out[0] = (uint8_t)((nb < 7 ? (0xff << (8 - nb)) & 0xff : 0xfe) | v);
    return nb;
}
// the header's bytes with its CRC-8 (at most 16); returns the length
__host__ __device__ static inline int fe_header(uint64_t fno, int n, int fs, int assign, uint8_t *h) {
    int bx, rx, rv;
    const int bc = fe_block_code(n, &bx), rc = fe_rate_code(fs, &rx, &rv);
    int len = 0;
    h[len++] = 0xff;
    h[len++] = 0xf8;                                   // sync, blocking strategy 0
    h[len++] = (uint8_t)(bc << 4 | rc);
    h[len++] = (uint8_t)(assign << 4 | 4 << 1);        // sample size code 100 = 16 bits
    len += fe_utf8(fno, h + len);
    if (bx == 1) h[len++] = (uint8_t)(n - 1);
    if (bx == 2) { h[len++] = (uint8_t)((n - 1) >> 8); h[len++] = (uint8_t)(n - 1); }
    if (rx == 2) { h[len++] = (uint8_t)(rv >> 8); h[len++] = (uint8_t)rv; }
    uint32_t c = 0;
    for (int i = 0; i < len; i++) {
        c ^= h[i];
        for (int b = 0; b < 8; b++) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xff : (c << 1) & 0xff;
    }
    h[len++] = (uint8_t)c;
    return len;
}
__host__ __device__ static inline int fe_header_len(uint64_t fno, int n, int fs) {
    uint8_t h[16];
    return fe_header(fno, n, fs, 0, h);
}

// ------------------------------------------------------------------ placement
#define FE_PL 1024
__global__ void __launch_bounds__(FE_PL) k_flac_place(int64_t frames, int C, int B, int fs, int ncand, int64_t nf,
                                                      FeWs ws, uint32_t *__restrict__ frame_bytes,
                                                      uint32_t *__restrict__ sub_bits,
                                                      int64_t *__restrict__ total) {
    __shared__ unsigned long long sc[FE_PL];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nf; base += FE_PL) {
        const int64_t f = base + t;
        unsigned long long bytes = 0;
        if (f < nf) {
            const int n = (int)(frames - f * B < B ? frames - f * B : B);
            const uint32_t *cb = ws.cbits + f * ncand;
            uint32_t bits = 0, assign = (uint32_t)(C - 1);
            if (C == 2) {
                const uint32_t a[4] = {cb[0] + cb[1], cb[0] + cb[3], cb[3] + cb[1], cb[2] + cb[3]};
                int m = 0;
                for (int q = 1; q < 4; q++)
                    if (a[q] < a[m]) m = q;
                bits = a[m];
                assign = m == 0 ? 1u : (uint32_t)(7 + m);
                if (sub_bits) {
                    sub_bits[f * 2] = m == 0 || m == 1 ? cb[0] : m == 2 ? cb[3] : cb[2];
                    sub_bits[f * 2 + 1] = m == 0 || m == 2 ? cb[1] : cb[3];
                }
            } else {
                for (int c = 0; c < C; c++) {
                    bits += cb[c];
                    if (sub_bits) sub_bits[f * C + c] = cb[c];
                }
            }
            bytes = (unsigned long long)fe_header_len((uint64_t)f, n, fs) + (bits + 7) / 8 + 2;
            ws.assign[f] = assign;
            frame_bytes[f] = (uint32_t)bytes;
        }
        sc[t] = bytes;
        __syncthreads();
        for (int d = 1; d < FE_PL; d <<= 1) {
            const unsigned long long x = t >= d ? sc[t - d] : 0;
            __syncthreads();
            sc[t] += x;
            __syncthreads();
        }
        if (f < nf) ws.off[f] = (int64_t)(carry + sc[t] - bytes);
        __syncthreads();
        if (t == FE_PL - 1) carry += sc[t];
        __syncthreads();
    }
    if (t == 0) *total = (int64_t)carry;
}

// ------------------------------------------------------------------ packing
// nb (1..32) low bits of v at bit `pos` of the big-endian word buffer W (pre-zeroed, lim
// words: a write past it is dropped -- the sizes are exact, so none is)
__device__ __forceinline__ void fe_put(uint32_t *W, uint32_t lim, uint32_t pos, uint32_t v, int nb) {
    const uint32_t wi = pos >> 5;
    if (wi + 1 >= lim) return;
    const int sh = 32 - (int)(pos & 31) - nb;
    if (sh >= 0) {
        atomicOr(&W[wi], v << sh);
    } else {
        atomicOr(&W[wi], v >> (-sh));
        atomicOr(&W[wi + 1], v << (32 + sh));
    }
}
__device__ __forceinline__ uint32_t fe_byte(const uint32_t *W, uint32_t i) {
    return (W[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
}
// a * b mod x^16 + x^15 + x^2 + 1
__device__ __forceinline__ uint32_t fe_gf16_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 16; i++) {
        if ((b >> i) & 1) r ^= a;
        a <<= 1;
        if (a & 0x10000u) a ^= 0x18005u;
    }
    return r;
}

// dynamic LDS: W [wwords] | s [B] | scan [FE_NT] | crc table [256] | misc [4]
// LPC false: the lpc_order == 0 encoder's kernel, with no LPC branch in it
template <bool LPC>
__global__ void __launch_bounds__(FE_NT) k_flac_pack(const int16_t *__restrict__ pcm, int64_t frames, int C, int B,
                                                     int fs, int ncand, FeWs ws,
                                                     const uint32_t *__restrict__ frame_bytes,
                                                     uint8_t *__restrict__ out, int64_t capacity, int wwords,
                                                     FeLpcWs lw) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fe_lds[];
    uint32_t *W = fe_lds;
    int *s = reinterpret_cast<int *>(fe_lds + wwords);
    uint32_t *scan = fe_lds + wwords + B;
    uint32_t *tab = scan + FE_NT;
    uint32_t *misc = tab + 256;

    const int t = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int64_t i0 = f * B;
    const int n = (int)(frames - i0 < B ? frames - i0 : B);
    const uint32_t fb = frame_bytes[f];
    const int64_t off = ws.off[f];
    const uint32_t assign = ws.assign[f];
    // (never taken: the capacity holds every frame at its bound and the staging buffer one)
    if ((fb + 3) / 4 + 1 > (uint32_t)wwords || off + fb > capacity) return;

    for (int i = t; i < wwords; i += FE_NT) W[i] = 0;
    {
        uint32_t c = (uint32_t)t << 8;
        for (int b = 0; b < 8; b++) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1) & 0xffffu;
        tab[t] = c;
    }
    if (t == 0) misc[0] = 0;
    __syncthreads();

    uint8_t hdr[16];
    const int hlen = fe_header((uint64_t)f, n, fs, (int)assign, hdr);
    if (t < hlen) fe_put(W, (uint32_t)wwords, 8u * t, hdr[t], 8);
    uint32_t pos = 8u * hlen;

    for (int c = 0; c < C; c++) {
        int cand = c;
        if (C == 2 && assign >= 8)   // left/side, side/right, mid/side
            cand = assign == 8 ? (c == 0 ? 0 : 3) : assign == 9 ? (c == 0 ? 3 : 1) : (c == 0 ? 2 : 3);
        const int w = (C == 2 && cand == 3) ? 17 : 16;
        const uint32_t wmask = (1u << w) - 1;
        const int64_t slot = f * ncand + cand;
        const uint32_t info = ws.cinfo[slot], bits = ws.cbits[slot];
        const int type = (int)(info & 0xff), p = (int)(info >> 8);
        for (int i = t; i < n; i += FE_NT) s[i] = fe_sample(pcm, i0 + i, C, cand);
        __syncthreads();
        if (t == 0) fe_put(W, (uint32_t)wwords, pos, (uint32_t)type << 1, 8);   // padding 0, type, no wasted bits
        if (type == 0) {
            if (t == 0) fe_put(W, (uint32_t)wwords, pos + 8, (uint32_t)s[0] & wmask, w);
        } else if (type == 1) {
            for (int i = t; i < n; i += FE_NT)
                fe_put(W, (uint32_t)wwords, pos + 8 + (uint32_t)i * w, (uint32_t)s[i] & wmask, w);
        } else {
            // FIXED, or LPC: after the warm-up samples the precision (12 bits: 0b1011), the
            // 5-bit shift and o 12-bit coefficients, then the residual as for FIXED
            const bool lpc = LPC && type >= FE_LPC0;
            const int o = lpc ? type - FE_LPC0 + 1 : type - 8;
            const uint8_t *kk = ws.ck + slot * FE_MAXP;
            int qv[FE_MAXO], lsh = 0;
#pragma unroll
            for (int j = 0; j < FE_MAXO; j++) qv[j] = 0;
            if (lpc) {
                lsh = (int)lw.lsh[slot];
#pragma unroll
                for (int j = 0; j < FE_MAXO; j++) qv[j] = lw.lq[slot * FE_MAXO + j];
            }
            if (t < o) fe_put(W, (uint32_t)wwords, pos + 8 + (uint32_t)t * w, (uint32_t)s[t] & wmask, w);
            const uint32_t coef = pos + 8 + (uint32_t)o * w;
            if (lpc && t == 0) fe_put(W, (uint32_t)wwords, coef, (11u << 5) | (uint32_t)lsh, 9);
            if (lpc && t < o) fe_put(W, (uint32_t)wwords, coef + 9 + 12u * t, (uint32_t)lw.lq[slot * FE_MAXO + t] & 0xfffu, 12);
            const uint32_t base = coef + (lpc ? 9u + 12u * o : 0u) + 6;
            if (t == 0) {
                fe_put(W, (uint32_t)wwords, base - 6, (uint32_t)p, 6);           // coding method 00, partition order
                fe_put(W, (uint32_t)wwords, base, kk[0], 4);
            }
            // this lane's residuals [a, b): their code lengths, then the codes
            const int plen = n >> p;
            const int R = n - o, per = (R + FE_NT - 1) / FE_NT;
            const int a = o + min(R, t * per), b = o + min(R, (t + 1) * per);
            uint32_t mine = 0;
            for (int i = a; i < b; i++) {
                const int k = kk[i / plen];
                mine += (fe_fold(LPC && lpc ? fe_lpc_residual(s, i, o, qv, lsh) : fe_residual(s, i, o)) >> k) + 1u + k;
            }
            scan[t] = mine;
            __syncthreads();
            for (int d = 1; d < FE_NT; d <<= 1) {
                const uint32_t x = t >= d ? scan[t - d] : 0;
                __syncthreads();
                scan[t] += x;
                __syncthreads();
            }
            uint32_t at = scan[t] - mine;
            for (int i = a; i < b; i++) {
                const int j = i / plen, k = kk[j];
                const uint32_t u = fe_fold(LPC && lpc ? fe_lpc_residual(s, i, o, qv, lsh) : fe_residual(s, i, o));
                const uint32_t q = u >> k;
                const uint32_t cp = base + 4u * (j + 1) + at;   // after the j + 1 parameters before it
                if (j > 0 && i == j * plen) fe_put(W, (uint32_t)wwords, cp - 4, (uint32_t)k, 4);
                // q zeros need no write: the stop bit and the k low bits
                fe_put(W, (uint32_t)wwords, cp + q, (1u << k) | (u & ((1u << k) - 1)), k + 1);
                at += q + 1u + k;
            }
        }
        pos += bits;
        __syncthreads();   // s and scan are reused by the next subframe
    }

    // CRC-16 of the frame up to the CRC: per-lane chunks, combined as polynomials
    const uint32_t nbody = (pos + 7) / 8;
    {
        const uint32_t chunk = (nbody + FE_NT - 1) / FE_NT;
        const uint32_t a = min(nbody, t * chunk), b = min(nbody, (t + 1) * chunk);
        if (a < b) {
            uint32_t c = 0;
            for (uint32_t i = a; i < b; i++) c = ((c << 8) ^ tab[((c >> 8) ^ fe_byte(W, i)) & 0xffu]) & 0xffffu;
            uint32_t e = nbody - b, x = 0x100u, r = 1;   // x^(8 e)
            while (e) {
                if (e & 1) r = fe_gf16_mul(r, x);
                x = fe_gf16_mul(x, x);
                e >>= 1;
            }
            atomicXor(&misc[0], fe_gf16_mul(c, r));
        }
    }
    __syncthreads();
    if (t == 0) fe_put(W, (uint32_t)wwords, 8u * nbody, misc[0] & 0xffffu, 16);
    __syncthreads();

    // copy out: bytes up to the first aligned word, aligned words, the rest
    uint8_t *dst = out + off;
    const uint32_t head = min(fb, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
    const uint32_t nw = (fb - head) / 4;
    if ((uint32_t)t < head) dst[t] = (uint8_t)fe_byte(W, t);
    const int sh = 8 * (int)(head & 3);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t j = t; j < nw; j += FE_NT) {
        const uint32_t wi = (head + 4 * j) >> 2;
        const uint32_t be = sh == 0 ? W[wi] : (W[wi] << sh) | (W[wi + 1] >> (32 - sh));
        dw[j] = __builtin_bswap32(be);
    }
    const uint32_t done = head + 4 * nw;
    if (done + t < fb) dst[done + t] = (uint8_t)fe_byte(W, done + t);
}

// ------------------------------------------------------------------ host side
// the largest frame in bytes: a 16-byte header, every subframe VERBATIM at 17 bits, CRC-16
static int64_t fe_frame_bound(int C, int n) { return 16 + ((int64_t)C * (8 + 17 * (int64_t)n) + 7) / 8 + 2; }

void flac_encode_size(int64_t frames, int C, int B, int lpc_order, int64_t *nf, int64_t *max_out,
                      int64_t *ws_bytes) {
    const int64_t n = (frames + B - 1) / B;
    const int last = (int)(frames - (n - 1) * B);
    const int ncand = C == 2 ? 4 : C;
    *nf = n;
    // (rounded up to whole words: the pack kernel's word stores stay inside the frame,
    // the slack only keeps the buffer's end aligned)
    *max_out = ((n - 1) * fe_frame_bound(C, B) + fe_frame_bound(C, last) + 3) / 4 * 4;
    *ws_bytes = n * 8 + n * 4 + 2 * n * ncand * 4 + n * ncand * FE_MAXP;
    // (an LPC subframe is chosen only below VERBATIM: the frame bound stands)
    if (lpc_order > 0) *ws_bytes += n * ncand * (FE_MAXO * 2 + 4);
}

hipError_t launch_flac_encode(const int16_t *pcm, int64_t frames, int C, int fs, int B, int lpc_order, uint8_t *out,
                              int64_t capacity, uint32_t *frame_bytes, uint32_t *sub_bits, int64_t *total,
                              void *wsp, hipStream_t st) {
    const int64_t nf = (frames + B - 1) / B;
    const int ncand = C == 2 ? 4 : C;
    if (nf * ncand > 0x7fffffffLL) return hipErrorInvalidValue;
    const FeWs ws = fe_ws(wsp, nf, ncand);
    const FeLpcWs lw = fe_lpc_ws(ws, nf, ncand);
    hipLaunchKernelGGL(k_flac_analyze, dim3((unsigned)(nf * ncand)), dim3(FE_NT), 0, st, pcm, frames, C, B, ncand,
                       ws);
    if (lpc_order > 0)
        hipLaunchKernelGGL(k_flac_lpc, dim3((unsigned)(nf * ncand)), dim3(FE_NT), 0, st, pcm, frames, C, B, ncand,
                           lpc_order, ws, lw);
    hipLaunchKernelGGL(k_flac_place, dim3(1), dim3(FE_PL), 0, st, frames, C, B, fs, ncand, nf, ws, frame_bytes,
                       sub_bits, total);
    const int wwords = (int)((fe_frame_bound(C, (int)(frames < B ? frames : B)) + 3) / 4 + 1);
    const size_t lds = (size_t)(wwords + B + FE_NT + 256 + 4) * 4;
    const void *pack = lpc_order > 0 ? reinterpret_cast<const void *>(k_flac_pack<true>)
                                     : reinterpret_cast<const void *>(k_flac_pack<false>);
    if (lds > 64 * 1024) {
        // one workgroup may hold up to a CU's whole LDS (160 KiB on gfx950); the largest
        // request here (8 channels, block 4608) is 98 KiB
        const hipError_t e = hipFuncSetAttribute(pack, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (lpc_order > 0)
        hipLaunchKernelGGL(k_flac_pack<true>, dim3((unsigned)nf), dim3(FE_NT), lds, st, pcm, frames, C, B, fs,
                           ncand, ws, frame_bytes, out, capacity, wwords, lw);
    else
        hipLaunchKernelGGL(k_flac_pack<false>, dim3((unsigned)nf), dim3(FE_NT), lds, st, pcm, frames, C, B, fs,
                           ncand, ws, frame_bytes, out, capacity, wwords, lw);
    return hipGetLastError();
}

}  // namespace amx
