// amx_plan_build.hpp -- host-only plan construction: every table and scalar of a plan
// from the chain description, the chunk list and the knobs.  No HIP: amx_plan.cpp
// uploads what build_plan_host leaves in PlanHost.
#pragma once
#include "../../include/amx.h"
#include "amx_tables.hpp"

#include <stddef.h>
#include <algorithm>
#include <string>
#include <vector>

namespace amx {

// libswresample's resampler geometry and filter bank for the 192 kHz measurement stream.
// max_alloc: the widest row (filter_alloc) the caller takes; the measurement kernels hold
// AMX_SWR_MAX_ALLOC, the output resampler (amx_resample.hip) AMX_RS_MAX_ALLOC
int swr_geometry(int in_rate, int out_rate, int *L, int *M);
int swr_filter(int in_rate, int out_rate, int *taps, int *alloc, double *factor,
               int max_alloc = AMX_SWR_MAX_ALLOC);
int swr_phases(int in_rate, int out_rate, int max_alloc = AMX_SWR_MAX_ALLOC);
int swr_incr(int in_rate, int out_rate, int64_t *src_incr, int64_t *dst_incr);
int swr_bank(int in_rate, int out_rate, float *bank, int max_alloc = AMX_SWR_MAX_ALLOC);

using Mat = std::vector<double>;        // row-major D x D
using MatL = std::vector<long double>;

// A linear time-invariant model s' = A s + B x of a chain, derived (in long double) by
// stepping a host copy of the chain from unit states / a unit input.
struct Lti {
    int D = 0;
    MatL A;
    std::vector<long double> B;
    template <class Step>
    void derive(int dim, Step step) {
        D = dim;
        A.assign((size_t)D * D, 0.0L);
        B.assign(D, 0.0L);
        std::vector<long double> s(D);
        for (int k = 0; k < D; k++) {
            std::fill(s.begin(), s.end(), 0.0L);
            s[k] = 1.0L;
            step(s.data(), 0.0L);
            for (int i = 0; i < D; i++) A[(size_t)i * D + k] = s[i];
        }
        std::fill(s.begin(), s.end(), 0.0L);
        step(s.data(), 1.0L);
        for (int i = 0; i < D; i++) B[i] = s[i];
    }
    Mat pow(int64_t p) const;
    // G[n][d] = (A^{L-1-n} B)[d]
    std::vector<double> gemv_table(int L) const;
    // window powers Mb^k, k = 1 .. K-1, of Mb = A^LS; K = the first k with
    // ||Mb^k|| <= tol (the block scan sums the previous K-1 blocks' contributions).
    int window_powers(int64_t LS, double tol, int max_k, std::vector<double> &out) const;
};

// the GEMV rows over int16 input: Gx scaled by 2^-15 in place, true, when no scaled entry
// of G or Gx would be subnormal; else both untouched, false (amx_plan_build.cpp)
bool scale_gemv_rows(const std::vector<double> &G, std::vector<double> &Gx);

// The two environment switches of plan construction, both for tests, with their
// defaults.  from_env() is the only reader of the variables.
struct PlanKnobs {
    int up_poly = 1;              // AMX_UP_POLY: 0 turns k_up_poly off
    int f1 = AMX_F1_SPLIT;        // AMX_F1: 2 (AMX_F1_FULL) forces the full-table pass-1 form
    static PlanKnobs from_env();
    // the envelope sizing reads the device's CU count (build_plan_host's ncu)
    static bool needs_ncu(bool multiband_on) { return multiband_on; }
};

// Every host-side field of a plan.  amx_plan (amx_plan.hpp) derives from it and adds the
// device pointers.
struct PlanHost {
    amx_chain_desc desc;
    ChainDev cd;
    int L = 256, Lkw = 512, hop = 0;
    // loudness measurement stream: ffmpeg's pass 1 resamples to 192 kHz (L phases,
    // step M; Lin chain frames = Lout 192 kHz frames per K segment); resamp = 0 when
    // the track already is at 192 kHz (the measurement runs on d_out itself)
    int resamp = 0, upL = 1, upM = 1, upLin = 0, upLout = 0, up_static = 0, up_ok = 1;
    int meas_native = 0;    // no 192 kHz resampler for this rate: peaks only, no loudnorm
    // libswresample's phase count (L, or 1024 when L > 1024), phase step dst / src per
    // output; up_lin: the step is not an integer, every output interpolates between rows
    // ph and ph + 1 (bank row pc = row 0 one tap later) with weight owt[n]
    int up_pc = 1, up_lin = 0;
    int up_taps = 32, up_alloc = 32;   // filter_length / filter_alloc (> 32: downsampling)
    int64_t up_src = 1, up_dst = 1;
    int up_poly = 0;             // k_up_poly's form (AMX_UP_POLY) when the rate has one
    int64_t n_slow = 0;          // K segments k_up_wave<false> takes (static / poly path): slow
    double kdf_b[5] = {0, 0, 0, 0, 0}, kdf_a[5] = {0, 0, 0, 0, 0};   // K filter, fused direct form (192 kHz)
    int mask = 0, D = 0;
    int lev_eq = 0, lev_x = 0, lev_kw = 0;
    int mb = 0;
    int Le = 1024, warm = 2304, rounds = 2;   // compressor envelope segments (amx_dyn.hip)
    int Le_t[4] = {0, 0, 0, 0};               // segment length of the table for t active bands
    int env_wg = 1, env_pin = 0;              // k_env0 placement (amx_dyn.hip launch_env)
    int f1_mode = AMX_F1_SPLIT;               // pass-1 form for float32 stereo + analog
    int n_es = 0;
    int fuse_kw = 0;        // loudness pass-1 GEMV + peak run inside k_front2
    int kw_aligned = 0;     // K-filter hop pieces split only at 16-frame tile boundaries
    int n_tracks = 0, n_chunks = 0, n_seg = 0, n_kseg = 0, n_blk = 0, n_kblk = 0;
    int64_t max_nkseg = 0;
    int64_t nloc = 0, out_frames = 0, max_chunk_out = 0, max_span = 0, max_chunk_n = 0;
    int64_t an_blocks = 0;      // k_analog_h's 4096-frame blocks over all chunks
    // 1: the crossover GEMV rows (Gx) hold g 2^-15 and k_gemv16 scales its G tiles the
    // same way, so both feed the int16 sample as (double)q (lti_models checks that no
    // scaled entry is subnormal; 0 keeps q / 32768 as the input)
    int gin_scaled = 0;
    int an_vec = 1;             // k_analog_h<true>: every chunk at an even input frame, >= 4 frames
    int64_t in_frames = 0;  // input frames the chunks read (max in_offset + frames)
    int64_t max_hops = 1;   // 100 ms hops of the longest track's measurement stream
    int mono16 = 0;         // mono int16 input: duplicated to stereo into ws o_dup first
    int sc = 0;             // a stream chain (amx_chain_desc.stream_chain)
    int any_empty_span = 0;           // a span with no K segment: its peak is zeroed directly
    // tables later entry points read on the host
    std::vector<ChunkDev> chunks;
    std::vector<KwSegDev> ksegs;
    std::vector<SpanDev> spans;
    Lti kw_model;
    std::vector<double> tail_pow;  // per span: A_kw^{len_last} (16 doubles)
    // tables only the upload reads
    std::vector<SegDev> segs, esegs;
    std::vector<int> eseg0, neseg;
    std::vector<ScanBlk> blks, kblks;
    std::vector<int64_t> n1tab;
    std::vector<float> bank, owt, bankn;          // resampler bank, weights; k_up_poly: rows in output order
    std::vector<int32_t> obase, oph, fcnt, slow;  // per output: frame, phase; k_up_poly: outputs per frame
    std::vector<double> tabs;                     // compressor tables [3][3][32769]
    std::vector<double> G, M, Mp, Gx, Mx, Mpx, Gkw, Mkw, Mpkw, qh, qt;
    std::vector<double> bounds, energies;         // libebur128 histogram
    std::vector<float> lut_half;   // the odd tanh table's half [0, 32768] (k_analog_h), or empty
    // workspace offsets
    size_t ws_bytes = 0;
    size_t o_a16 = 0, o_e = 0, o_s = 0, o_p16 = 0, o_ex = 0, o_sx = 0, o_bands = 0, o_m = 0, o_gain = 0, o_esv = 0,
           o_ee0 = 0, o_eflags = 0, o_eact = 0, o_ehead = 0, o_elist = 0, o_eprev = 0, o_elist0 = 0;
    size_t o_ekw = 0, o_skw = 0, o_parts = 0, o_phop = 0, o_eterms = 0;
    size_t o_eb = 0, o_ebx = 0, o_ebk = 0, o_pk = 0, o_dup = 0;
};

// Fills `h` from the arguments of amx_plan_create.  ncu: the device's CU count (read
// only when knobs.needs_ncu).  Returns AMX_OK, or the error code with its text in `err`.
int build_plan_host(const amx_chain_desc *desc, const amx_chunk *chunks, int32_t n_chunks,
                    const int64_t *track_frame0, const int64_t *track_total_frames, int32_t seg_frames,
                    const PlanKnobs &knobs, int ncu, PlanHost &h, std::string &err);

}  // namespace amx
