// amx_plan.hpp -- the plan objects behind include/amx.h's opaque handles (private to
// amx_plan.cpp and the plan harness): the host fields build_plan_host fills, plus the
// device copies of its tables, which the plan owns.
#pragma once
#include "amx_internal.hpp"
#include "amx_plan_build.hpp"

#include <vector>

struct amx_plan : amx::PlanHost {
    // every device allocation the plan owns: upload() and replace() record here,
    // amx_plan_free releases what is recorded
    std::vector<void *> owned;
    const int32_t *gate = nullptr;   // amx_plan_set_gate: the per-sample kernels' mode word
    int32_t *publish = nullptr;      // amx_plan_set_publish: pinned host words k_decide also stores
    hipStream_t up_aux = nullptr;            // k_up_wave<false>'s stream, forked from / joined to the caller's
    hipEvent_t up_fork = nullptr, up_join = nullptr;
    int kw_rest_states = 0;  // the last amx_loudness_pass1 left the K-filter start states from rest
    int kw_eb_ready = 0;     // the K scan's block sums (o_ebk) are those of the current e
    // device constant tables
    ChainDev *d_cd = nullptr;
    ChunkDev *d_chunks = nullptr;
    SegDev *d_segs = nullptr;
    KwSegDev *d_ksegs = nullptr;
    SpanDev *d_spans = nullptr;
    ScanBlk *d_blks = nullptr, *d_kblks = nullptr;
    SegDev *d_esegs = nullptr;
    int *d_eseg0 = nullptr, *d_neseg = nullptr;
    int64_t *d_n1 = nullptr;
    double *d_G = nullptr, *d_M = nullptr, *d_Mp = nullptr;
    double *d_Gx = nullptr, *d_Mx = nullptr, *d_Mpx = nullptr;
    double *d_Gkw = nullptr, *d_Mkw = nullptr, *d_Mpkw = nullptr;
    double *d_qh = nullptr, *d_qt = nullptr;
    double *d_tabs = nullptr, *d_bounds = nullptr, *d_energies = nullptr;
    double *d_tailpow = nullptr;
    int32_t *d_obase = nullptr, *d_oph = nullptr;
    float *d_owt = nullptr;
    int32_t *d_slow = nullptr;   // K segments k_up_wave<false> takes (static / poly path); n_slow of them
    int32_t *d_fcnt = nullptr;   // k_up_poly: outputs per segment frame
    float *d_bankn = nullptr;    // k_up_poly: bank rows in output order
    float *d_bank = nullptr;
    float *d_lut = nullptr;
    float *d_in_lut = nullptr;     // a stream chain's input table (amx_chain_desc.eq_in_lut), or NULL
    float *d_lut_half = nullptr;   // the odd tanh table's half [0, 32768] (k_analog_h), or NULL
    unsigned int *d_pcnt = nullptr;   // k_peak_reduce's per-track block counter (self re-arming)
    int *d_ppart = nullptr;           // its per-block partial maxima
    double *d_carryP = nullptr;       // amx_kw_carry_setup
    int n_prev = 0;
    double *lim_att = nullptr;     // amx_plan_set_limiter_trace
    int32_t lim_channels = 2;      // amx_plan_set_limiter_channels
    amx::LimScratch lim;              // general alimiter segments (amx_limiter_prepare)
    amx::ScanPlan scan_eq() const { return {D, n_blk, lev_eq, d_blks, d_M, d_Mp}; }
    amx::ScanPlan scan_xo() const { return {AMX_XO_DIM, mb ? n_blk : 0, lev_x, d_blks, d_Mx, d_Mpx}; }
    amx::ScanPlan scan_kw() const { return {AMX_KW_DIM, n_kblk, lev_kw, d_kblks, d_Mkw, d_Mpkw}; }
};

// A 3..8-channel plan (amx_mc_plan_create): up to three stereo plans over the interleaved
// stream and the real frames
struct amx_mc_plan {
    int C = 0, mb = 0, in_s16 = 0;
    amx_plan *pa = nullptr, *pb = nullptr, *pc = nullptr;
    int64_t M = 0;                 // stream samples the pack covers
    int64_t out_frames = 0;
    size_t o_pack = 0, o_outa = 0, o_outb = 0, o_wa = 0, o_wb = 0, o_wc = 0, ws_bytes = 0;
};
