// amx_flacdec_core.hpp -- the FLAC frame decoder the device path runs (amx_flacdec.hip), in
// plain C++ that also compiles for the host: tests/flacdec_host_main.cpp runs this text on
// the CPU against the host decoder (amx_flac.cpp, the independent yardstick, which does not
// use it) and under ASan / UBSan, before any of it runs on a GPU.
//
// One call decodes one candidate frame whose header the host scan has parsed
// (amx_flac_scan): the C subframes in stream order, the frame's end and its CRC-16.
// No allocation, no recursion, no exceptions; every buffer is the caller's.
//
// Widths.  Stream depths 4..24, so an effective subframe width of 1..25
// bits (a side channel carries one more).  Samples, warm-ups and residuals are int32; the
// FIXED predictors wrap in 32 bits; the LPC sum is a wrapping 64-bit accumulate with an
// arithmetic shift.  A reconstructed sample that does not fit the subframe's effective
// width, or a residual that does not fit int32, makes the frame NOT OK, like a failed
// CRC-16: RFC 9639 calls such a stream invalid (the host decoder decodes it in wrapping
// int64, so on invalid streams this decoder is the stricter one; on valid streams the
// two agree bit for bit).
//
// Bounds.  Reads stop at `end` = min(size, frame start + limit) (the host's limit rule):
// a read past it sets `bad` and yields zeros, a unary run ends there.  Partition counts
// come from the block size, every sample loop runs `block` times at most, and samples
// leave through the caller's Store, which owns the bounds of what it writes.
//
// Store (lane-private state the caller places where it wants -- registers, LDS, memory):
//   void begin(int channel, int wasted)   a subframe starts; put() takes unshifted samples
//   void put(int i, int32_t v)            sample i of the subframe (i ascending from 0)
//   int32_t get(int i)                    an earlier sample, i within the last 32 put
//   void finish(int n)                    the subframe's n samples are all put
//   void coef_set(int k, int32_t c), int32_t coef(int k)     LPC coefficients, k < 32
//   void out_of_width()                   the frame is refused for a width rule (a note for
//                                         the CPU test; the frame is simply not ok)
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FLACD_HD __host__ __device__
#else
#define FLACD_HD
#endif

namespace flacd {

// CRC-16 (poly 0x8005, MSB first, initial 0): entry i of the byte table
FLACD_HD inline uint16_t crc16_entry(int i) {
    uint16_t w = (uint16_t)(i << 8);
    for (int k = 0; k < 8; k++) w = (uint16_t)((w & 0x8000) ? (w << 1) ^ 0x8005 : (w << 1));
    return w;
}

FLACD_HD inline uint32_t load_be32(const uint8_t *p) {   // p 4-byte aligned
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
    return __builtin_bswap32(w);
}

FLACD_HD inline uint16_t crc16(const uint8_t *d, int64_t n, const uint16_t *tab) {
    uint16_t c = 0;
    int64_t i = 0;
    while (i < n && ((uintptr_t)(d + i) & 3)) c = (uint16_t)((c << 8) ^ tab[(c >> 8) ^ d[i++]]);
    for (; i + 4 <= n; i += 4) {
        const uint32_t w = load_be32(d + i);
        c = (uint16_t)((c << 8) ^ tab[(c >> 8) ^ (w >> 24)]);
        c = (uint16_t)((c << 8) ^ tab[(c >> 8) ^ ((w >> 16) & 0xFF)]);
        c = (uint16_t)((c << 8) ^ tab[(c >> 8) ^ ((w >> 8) & 0xFF)]);
        c = (uint16_t)((c << 8) ^ tab[(c >> 8) ^ (w & 0xFF)]);
    }
    for (; i < n; i++) c = (uint16_t)((c << 8) ^ tab[(c >> 8) ^ d[i]]);
    return c;
}

// MSB-first bit reader over a 64-bit window (valid bits left-aligned, the rest zero),
// refilled by aligned 32-bit loads where the position and the bound allow, else by bytes
struct Bits {
    const uint8_t *p;
    int64_t end;     // reads stop here (bytes)
    int64_t byte;    // next byte to load
    uint64_t cache;
    int nb;
    bool bad;
    FLACD_HD Bits(const uint8_t *d, int64_t end_, int64_t byte0)
        : p(d), end(end_), byte(byte0 < end_ ? byte0 : end_), cache(0), nb(0), bad(byte0 > end_ || byte0 < 0) {}
    FLACD_HD int64_t pos() const { return byte * 8 - nb; }
    FLACD_HD void refill() {   // every turn advances `byte`: at most 8 turns
        while (nb <= 32 && byte < end) {
            if (byte + 4 <= end && ((uintptr_t)(p + byte) & 3) == 0) {
                cache |= (uint64_t)load_be32(p + byte) << (32 - nb);
                nb += 32;
                byte += 4;
            } else {
                cache |= (uint64_t)p[byte++] << (56 - nb);
                nb += 8;
            }
        }
    }
    FLACD_HD uint32_t bits(int k) {   // k in 0..32
        if (k == 0) return 0;
        if (nb < k) {
            refill();
            if (nb < k) {
                bad = true;
                nb = 0;
                cache = 0;
                return 0;
            }
        }
        const uint32_t v = (uint32_t)(cache >> (64 - k));
        cache <<= k;
        nb -= k;
        return v;
    }
    FLACD_HD int32_t sbits(int k) {   // two's complement, k in 0..32
        if (k == 0) return 0;
        const uint32_t v = bits(k);
        return (int32_t)(v << (32 - k)) >> (32 - k);
    }
    // zeros before the next 1 (consumed); the run ends at `end` with bad set.  Every turn
    // that does not return consumes at least one bit, so the turns are bounded by the input
    FLACD_HD uint32_t unary() {
        uint32_t q = 0;
        for (;;) {
            if (nb == 0) {
                refill();
                if (nb == 0) {
                    bad = true;
                    return q;
                }
            }
            if (cache == 0) {
                q += (uint32_t)nb;
                nb = 0;
                continue;
            }
            const int z = __builtin_clzll(cache);   // < nb: the bits past nb are zero
            q += (uint32_t)z;
            cache = z + 1 < 64 ? cache << (z + 1) : 0;
            nb -= z + 1;
            return q;
        }
    }
};

FLACD_HD inline bool fits(int64_t v, int width) {   // v is a `width`-bit two's complement value
    const int64_t t = v >> (width - 1);
    return t == 0 || t == -1;
}

// one subframe of `block` samples at depth bps (1 more for a side channel) through st
template <class Store>
FLACD_HD inline bool subframe(Bits &br, int block, int bps, int channel, Store &st) {
    if (br.bits(1) != 0) return false;
    const int type = (int)br.bits(6);
    int wasted = 0;
    if (br.bits(1)) {
        const uint32_t w = br.unary();
        if (w >= (uint32_t)bps) return false;
        wasted = (int)w + 1;
    }
    if (wasted >= bps || br.bad) return false;
    const int eb = bps - wasted;   // 1..25
    st.begin(channel, wasted);
    int order = 0, shift = 0;
    bool lpc = false;
    if (type == 0) {
        const int32_t v = br.sbits(eb);
        for (int i = 0; i < block; i++) st.put(i, v);
        st.finish(block);
        return !br.bad;
    } else if (type == 1) {
        for (int i = 0; i < block; i++) {
            st.put(i, br.sbits(eb));
            if (br.bad) return false;
        }
        st.finish(block);
        return true;
    } else if (type >= 8 && type <= 12) {
        order = type - 8;
    } else if (type >= 32) {
        order = type - 31;
        lpc = true;
    } else {
        return false;
    }
    if (order > block) return false;
    // the last four samples for the FIXED predictors (s1 the newest)
    uint32_t s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int i = 0; i < order; i++) {
        const int32_t v = br.sbits(eb);
        st.put(i, v);
        s4 = s3, s3 = s2, s2 = s1, s1 = (uint32_t)v;
    }
    if (lpc) {
        const int prec = (int)br.bits(4) + 1;
        if (prec == 16) return false;
        shift = br.sbits(5);
        if (shift < 0) return false;
        for (int k = 0; k < order; k++) st.coef_set(k, br.sbits(prec));
    }
    if (br.bad) return false;
    // partitioned Rice residual, predicted and stored sample by sample
    const int method = (int)br.bits(2);
    if (method > 1) return false;
    const int pbits = method == 0 ? 4 : 5, esc = (1 << pbits) - 1;
    const int porder = (int)br.bits(4);
    const int parts = 1 << porder;
    if ((block >> porder) < order || (block & (parts - 1)) != 0) return false;
    int i = order;
    for (int p = 0; p < parts; p++) {   // parts <= block
        const int cnt = (block >> porder) - (p == 0 ? order : 0);
        const int k = (int)br.bits(pbits);
        int raw = -1;
        if (k == esc) raw = (int)br.bits(5);
        if (br.bad) return false;
        for (int j = 0; j < cnt; j++) {
            int32_t r;
            if (raw >= 0) {
                r = br.sbits(raw);
            } else {
                const uint32_t q = br.unary();
                if (((uint64_t)q >> (32 - k)) != 0) {   // the folded value passes 32 bits (k <= 30)
                    st.out_of_width();
                    return false;
                }
                const uint32_t u = (q << k) | br.bits(k);
                r = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
            }
            if (br.bad) return false;
            int64_t v;
            if (lpc) {
                uint64_t acc = 0;
                for (int c = 0; c < order; c++)
                    acc += (uint64_t)(int64_t)st.coef(c) * (uint64_t)(int64_t)st.get(i - 1 - c);
                v = (int64_t)((uint64_t)(int64_t)r + (uint64_t)((int64_t)acc >> shift));
            } else {
                uint32_t pred = 0;
                switch (order) {
                case 1: pred = s1; break;
                case 2: pred = 2 * s1 - s2; break;
                case 3: pred = 3 * s1 - 3 * s2 + s3; break;
                case 4: pred = 4 * s1 - 6 * s2 + 4 * s3 - s4; break;
                default: break;
                }
                v = (int32_t)((uint32_t)r + pred);
                s4 = s3, s3 = s2, s2 = s1, s1 = (uint32_t)v;
            }
            if (!fits(v, eb)) {
                st.out_of_width();
                return false;
            }
            st.put(i++, (int32_t)v);
        }
    }
    st.finish(block);
    return true;
}

// The candidate frame at byte `off` of d[0 .. size): header fields from the scan (block
// 1..65535, bps 4..24, assign 0..10, C channels, data_byte = the header's length with its
// CRC-8, limit = the host's frame-length bound).  true: the frame decoded, its CRC-16
// matches, *end_out = the byte after it.  crc_tab: 256 entries of crc16_entry.
template <class Store>
FLACD_HD inline bool decode_frame(const uint8_t *d, int64_t size, int64_t off, int data_byte, int64_t limit,
                                  int block, int bps, int assign, int C, Store &st, const uint16_t *crc_tab,
                                  int64_t *end_out) {
    if (off < 0 || off >= size || data_byte < 5 || data_byte > 16 || limit < 0 || block < 1 || block > 65535 ||
        bps < 4 || bps > 24 || C < 1 || C > 8 || assign < 0 || assign > 10)
        return false;
    const int64_t end = limit < size - off ? off + limit : size;
    Bits br(d, end, off + data_byte);
    for (int c = 0; c < C; c++) {
        // the side channel carries one more bit (left/side: 1, side/right: 0, mid/side: 1)
        const bool side = (assign == 8 && c == 1) || (assign == 9 && c == 0) || (assign == 10 && c == 1);
        if (!subframe(br, block, bps + (side ? 1 : 0), c, st) || br.bad) return false;
    }
    const int64_t cb = (br.pos() + 7) >> 3;   // the byte after the padding
    if (cb + 2 > end) return false;
    if (crc16(d + off, cb - off, crc_tab) != (uint16_t)((d[cb] << 8) | d[cb + 1])) return false;
    *end_out = cb + 2;
    return true;
}

// stereo decorrelation of one sample pair (the subframes' values a, b), as the host does it
FLACD_HD inline void undo_stereo(int assign, int32_t a, int32_t b, int32_t &l, int32_t &r) {
    l = a;
    r = b;
    if (assign == 8) {
        r = (int32_t)((uint32_t)a - (uint32_t)b);
    } else if (assign == 9) {
        l = (int32_t)((uint32_t)a + (uint32_t)b);
    } else if (assign == 10) {
        const int32_t m = (int32_t)(((uint32_t)a << 1) | ((uint32_t)b & 1));
        l = (int32_t)((uint32_t)m + (uint32_t)b) >> 1;
        r = (int32_t)((uint32_t)m - (uint32_t)b) >> 1;
    }
}

// plane stride of a candidate's scratch slot: the block rounded up to whole 16-sample runs
FLACD_HD inline int64_t plane_stride(int block) { return ((int64_t)block + 15) & ~(int64_t)15; }

// The chain that tiles the stream from candidate 0: flag[k] 1 = ok, nxt[k] = the candidate
// starting at frame k's end (-1: none).  Writes chain[], first[] (exclusive scan of the
// blocks) and blocks[] for q < the returned count; *samples the running total.  Stops at
// the first candidate that is not ok or missing, or when max_blocks is reached
// (*stop = the candidate the walk stopped at, -1 at a clean end).
template <class GetFlag, class GetNext, class GetBlock>
FLACD_HD inline int64_t walk_chain(int64_t nc, GetFlag flag, GetNext nxt, GetBlock blk, int64_t max_blocks,
                                   int32_t *chain, int64_t *first, int32_t *blocks, int64_t *samples,
                                   int64_t *stop) {
    int64_t k = 0, n = 0, total = 0;
    *stop = -1;
    while (k >= 0 && k < nc) {   // k strictly ascends: at most nc turns
        if (flag(k) != 1 || n >= max_blocks) {
            *stop = k;
            break;
        }
        const int b = blk(k);
        chain[n] = (int32_t)k;
        first[n] = total;
        blocks[n] = b;
        n++;
        total += b;
        const int64_t j = nxt(k);
        if (j <= k) break;
        k = j;
    }
    *samples = total;
    return n;
}

}  // namespace flacd
