// amx_tables.hpp -- the plain tables a plan holds: the structs the kernels read, the
// constants that size them, and the two small host helpers that tie a table's size to a
// kernel's form.  No HIP: amx_plan_build.cpp (host-only plan construction) and the kernel
// files (through amx_internal.hpp) both include it.
#pragma once
#include <stdint.h>

#define AMX_MAX_EQ_DIM 20
#define AMX_XO_DIM 8      // crossover: 2 low-pass + 2 high-pass SOS sections
#define AMX_KW_DIM 4      // K-weighting 4th-order DF-II state (v1..v4)
#define AMX_TF_FRAMES 16  // LDS tile frames (AMX_TF in amx_dev.hpp)
#define AMX_SCAN_S 16     // segments per scan block
#define AMX_ENV_MAX_ROUNDS 16  // envelope fix-up flag words (k_env0 clears them)
#define AMX_ENV_NCTR 4         // fix-up diagnostic counters per round (after the flags; k_envchain)
#define AMX_ENV_BACT (AMX_ENV_MAX_ROUNDS * (1 + AMX_ENV_NCTR))  // band-activity words after the counters
#define AMX_ENV_LIST (AMX_ENV_BACT + 4)  // re-run list length, chain-head list length, k_envseq's flag
#define AMX_RMS_MAXLOOK 1024   // the compressor detector's longest window (k_rms<1024>): rates to 204.8 kHz
#define AMX_EQC 64        // compact EQ coefficient block (see ChainDev::eqc)
#define AMX_MEAS_RATE 192000  // loudnorm pass 1 measures at 192 kHz (af_loudnorm dynamic mode)
#define AMX_SWR_MAX_ALLOC 144   // the widest resampler row (filter_alloc) restated
#define AMX_RS_MAX_ALLOC 256    // the output resampler's widest row (amx_resample.hip; factor >= 1 / 8)
#define AMX_RS_TILE 256         // output frames per workgroup of k_resample
// pass 1 for float32 stereo input with the analog stage: k_analog_h + k_gemv16 (the odd
// tanh table's half in LDS; default), or k_front1s with the full table in global memory
// (a table that is not odd; AMX_F1 = 2 forces it, for tests)
#define AMX_F1_SPLIT 0
#define AMX_F1_FULL 2

// One EQ stage of _apply_eq_to_channel (audio_mastering_engine.py:277-282).
struct EqStageDev {
    int32_t kind;    // 0 skipped, 1 shelf (lfilter ba, :283-289), 2 peak (4 SOS, :290-298)
    int32_t neg;     // shelf with gain_db < 0 (:289)
    double g;        // 10**(gain_db/20)
    double gm1;      // g - 1
    float gf;        // float32(g): the float32 product of :289 on a float32 input
    float pad_;
    double c[24];    // shelf: b0 b1 b2 a0 a1 a2 ; peak: 4 x [b0 b1 b2 a0 a1 a2]
};

struct ChainDev {
    int32_t fs, chin;
    int32_t in_s16, pad0_;
    int32_t analog_on, has_lut;
    int32_t eq_mask, eq_dim;
    int32_t width_on, mb_on;
    float width, drive;
    double an_lo[6];
    double an_glo1;   // analog low shelf g - 1
    double an_hi[6];
    double an_ghi1;
    EqStageDev st[4];
    double xlo[12], xhi[12];
    // compressor (pydub compress_dynamic_range, :306-308)
    int32_t look;          // int(5 ms * fs)
    int32_t rthr[3];       // smallest integer rms with rms > thresh_rms
    int32_t rq[3];         // first table index r with m(r) != 0 (32769: none); r < rq is quiet
    int32_t pad_rq_;
    double kw1[6], kw2[6]; // K-weighting as two DF-II-T biquads (libebur128 pb/pa, rb/ra)
    // Active EQ stages packed in order for register-resident use (amx_dev.hpp eq_chain):
    //   shelf: b0 b1 b2 a1 a2 gx     (gx = g-1, or the negative-gain factor g / f32(g))
    //   peak : 4 x [b0 b1 b2 a1 a2] gm1
    double eqc[AMX_EQC];
    // envelope divisions inc = m / A, dec = m / R (pydub frame counts): env_rcp = 1
    // when the reciprocal-multiply with one FMA correction was checked on the host to
    // equal the IEEE quotient for every table value m (amx_dyn.hip env_div)
    double env_A, env_R, env_rA, env_rR;
    int32_t env_rcp;
    int32_t pad1_;         // (the struct's size is recorded: tests/golden/plan_build.txt)
    // envelope segment tables by active-band count (amx_dyn.hip): table t (1..3) cuts
    // the chunks into segments of Le frames so that t bands' segments fill the CUs as
    // one resident wave set; k_rms flags the bands with a frame over the threshold and
    // the envelope kernels take the table of that count.  Offsets index the plan's
    // concatenated segment array and per-chunk (first, count) arrays; the per-band
    // segment arrays (s, e, act, prev) have stride es_ld = the largest n_es
    int32_t es_ld;
    struct { int32_t es_off, n_es, ch_off, Le; } etab[4];
    // exp10 constants of the gain (amx_dyn.hip exp10_gain): read through the plan so
    // they are scalar operands of the FMAs (a 64-bit literal is not encodable)
    double exc[16];
};

// A ~30 s chunk (ffmpeg segment, :178).  loc_off indexes chunk-local scratch.
struct ChunkDev {
    int64_t in_off;    // first input frame in d_in
    int64_t loc_off;   // offset in per-frame scratch arrays (sum of previous chunk lengths)
    int64_t out_off;   // offset in d_out (frames)
    int64_t n;         // input frames
    int64_t out_n;     // output frames (n, or pydub overlay ms-rounded length when multiband)
    int32_t seg0, nseg;
    int32_t track, pad_;
};

// IIR / envelope segment: `len` frames from chunk-local frame `pos`.
struct SegDev {
    int64_t pos;
    int32_t chunk;
    int32_t len;
    int32_t first;     // global index of the first segment of the same chunk
    int32_t last;      // 1 if last segment of its chunk
};

// K-weighting segment over a track span of d_out.
struct KwSegDev {
    int64_t out_pos;     // frame in d_out
    int64_t tframe;      // frame in the whole-track timeline
    int32_t track;
    int32_t len;
    int32_t first;       // global index of the span's first segment (the scan stream)
    int32_t last;        // 1 if last segment of its span
};

// A block of up to AMX_SCAN_S consecutive segments of one stream (amx_scan.hip).
struct ScanBlk {
    int32_t seg0, nseg;
    int32_t first;       // index of the stream's first block
    int32_t last;        // 1 if the stream's last block
    int32_t stream, pad_;
};

struct SpanDev {
    int64_t out_off, out_n, tframe0, ttotal;   // chain-output frames (d_out) of the span
    int32_t kseg0, nkseg;
    // the loudness measurement's stream (192 kHz when resampled, else == the chain's):
    // first frame of the span in the whole track, frames of the span, of the track
    int64_t m_tframe0, m_n, m_total;
    int32_t edge_lo, edge_hi;   // resampler window past the span start / end reads the
                                // neighbour rank's frames (edge buffer), else mirrors
};

namespace amx {
// k_up_poly's template form as one code (launch switch, plan), and the (CMIN, CMAX, TB)
// forms the kernel is built for (amx_loud192.hip)
#define AMX_UP_POLY(cmin, cmax, tb) ((cmin) * 256 + (cmax) * 16 + (tb))
#define AMX_UP_POLY_FORMS(X) X(4, 5, 7) X(2, 3, 7) X(1, 2, 7) X(6, 6, 8) X(3, 3, 8)
inline int up_poly_form(int cmin, int cmax, int tb) {   // the code if that form is built, else 0
#define AMX_UP_POLY_HAS(c0, c1, t) if (cmin == c0 && cmax == c1 && tb == t) return AMX_UP_POLY(c0, c1, t);
    AMX_UP_POLY_FORMS(AMX_UP_POLY_HAS)
#undef AMX_UP_POLY_HAS
    return 0;
}

// k_peak_reduce (amx_loud.hip): segments per workgroup = threads x per thread; the plan
// sizes the per-block partial maxima by the same count
#define AMX_PEAK_THREADS 1024
#define AMX_PEAK_PER_THREAD 8
inline int peak_reduce_blocks(int64_t max_nkseg) {
    const int64_t per = (int64_t)AMX_PEAK_THREADS * AMX_PEAK_PER_THREAD;
    return (int)((max_nkseg + per - 1) / per);
}
}  // namespace amx
