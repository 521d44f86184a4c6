// amx_plan.cpp -- host side of libamx.so: the C ABI of include/amx.h.  A plan's tables
// are built by amx_plan_build.cpp (host arithmetic only); amx_plan_create uploads them
// and the plan owns the device copies (amx_plan.hpp).
#include "../../include/amx.h"
#include "amx_internal.hpp"
#include "amx_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHK(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) return fail(AMX_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

using amx::Mat;

// One device allocation of n elements (an empty table: one element), filled from src
// when given.  The plan owns it: amx_plan_free releases what is recorded in p->owned.
template <class T>
int upload(amx_plan *p, T **dst, const T *src, size_t n) {
    if (n == 0) n = 1;
    HIPCHK(hipMalloc((void **)dst, n * sizeof(T)));
    p->owned.push_back(*dst);
    if (src) HIPCHK(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return AMX_OK;
}
template <class T>
int upload(amx_plan *p, T **dst, const std::vector<T> &v) {
    return upload(p, dst, v.empty() ? (const T *)nullptr : v.data(), v.size());
}
// Puts `fresh` (an allocation the plan takes over, or NULL) in the place of the owned
// allocation *slot, which is released.
template <class T>
void replace(amx_plan *p, T *&slot, T *fresh) {
    auto it = std::find(p->owned.begin(), p->owned.end(), (void *)slot);
    if (slot && it != p->owned.end()) {
        (void)hipFree(slot);
        p->owned.erase(it);
    }
    if (fresh) p->owned.push_back(fresh);
    slot = fresh;
}
template <class T>
T *wsp(void *ws, size_t off) {
    return reinterpret_cast<T *>(reinterpret_cast<char *>(ws) + off);
}

struct PlanFree {
    void operator()(amx_plan *p) const { amx_plan_free(p); }
    void operator()(amx_mc_plan *m) const { amx_mc_plan_free(m); }
};

// the device copies of the tables build_plan_host made
int upload_tables(amx_plan *p) {
#define UP(dst, ...)                                             \
    do {                                                         \
        if (int rc_ = upload(p, &p->dst, __VA_ARGS__)) return rc_; \
    } while (0)
    UP(d_cd, &p->cd, 1);
    UP(d_chunks, p->chunks);
    UP(d_segs, p->segs);
    UP(d_ksegs, p->ksegs);
    UP(d_spans, p->spans);
    UP(d_blks, p->blks);
    UP(d_kblks, p->kblks);
    UP(d_n1, p->n1tab);
    UP(d_esegs, p->esegs);
    UP(d_eseg0, p->eseg0);
    UP(d_neseg, p->neseg);
    UP(d_G, p->G);
    UP(d_M, p->M);
    UP(d_Mp, p->Mp);
    UP(d_Gx, p->Gx);
    UP(d_Mx, p->Mx);
    UP(d_Mpx, p->Mpx);
    UP(d_Gkw, p->Gkw);
    UP(d_Mkw, p->Mkw);
    UP(d_Mpkw, p->Mpkw);
    UP(d_tabs, p->tabs);
    UP(d_bounds, p->bounds);
    UP(d_energies, p->energies);
    UP(d_tailpow, p->tail_pow);
    UP(d_obase, p->obase);
    UP(d_qh, p->qh);
    UP(d_qt, p->qt);
    UP(d_oph, p->oph);
    UP(d_owt, p->owt);
    if (!p->slow.empty()) UP(d_slow, p->slow);
    UP(d_bank, p->bank);
    if (p->up_poly) {
        UP(d_fcnt, p->fcnt);
        UP(d_bankn, p->bankn);
    }
    {   // k_peak_reduce's counters (zero between launches) and partial maxima
        const size_t nt = (size_t)(p->n_tracks > 0 ? p->n_tracks : 1);
        const size_t nb = (size_t)amx::peak_reduce_blocks(p->max_nkseg);
        UP(d_pcnt, std::vector<unsigned int>(nt, 0u));
        UP(d_ppart, (const int *)nullptr, nt * (nb ? nb : 1) * 4);
    }
    if (p->desc.tanh_lut) UP(d_lut, p->desc.tanh_lut, 65536);
    if (p->sc && p->desc.eq_in_lut) UP(d_in_lut, p->desc.eq_in_lut, 65536);
    if (!p->lut_half.empty()) UP(d_lut_half, p->lut_half);
#undef UP
    return AMX_OK;
}

// the host tables only upload_tables reads (later entry points read chunks, ksegs,
// spans, kw_model and tail_pow)
template <class... V>
void drop(V &...v) {
    (V().swap(v), ...);
}
void drop_uploaded(amx::PlanHost &h) {
    drop(h.segs, h.esegs, h.eseg0, h.neseg, h.blks, h.kblks, h.n1tab, h.bank, h.owt, h.bankn);
    drop(h.obase, h.oph, h.fcnt, h.slow, h.tabs, h.G, h.M, h.Mp, h.Gx, h.Mx, h.Mpx, h.Gkw, h.Mkw, h.Mpkw);
    drop(h.qh, h.qt, h.bounds, h.energies, h.lut_half);
}

// the stereo int16 plan a 3..8-channel plan runs a part of its chain on: the caller's
// settings without the analog stage, the width and the tables (amx_mc_plan_create)
amx_chain_desc mc_sub_desc(const amx_chain_desc &desc, int stream_chain) {
    amx_chain_desc d = desc;
    d.channels_in = 2;
    d.input_s16 = 1;
    d.analog_on = 0;
    d.tanh_lut = nullptr;
    d.width_on = 0;
    d.measure_only = 0;
    d.stream_chain = stream_chain;
    d.eq_in_lut = nullptr;
    return d;
}

}  // namespace

extern "C" {

int amx_abi_version(void) { return AMX_ABI_VERSION; }
const char *amx_last_error(void) { return g_err.c_str(); }
#ifndef AMX_SRC_HASH
#define AMX_SRC_HASH "unstamped"
#endif
// "AMX_SRC_HASH=<hex>" in the binary: amx/build.py reads it from the file without
// loading the library (no HIP runtime before torch's)
static const char amx_stamp[] = "AMX_SRC_HASH=" AMX_SRC_HASH;
const char *amx_build_id(void) { return amx_stamp + 13; }

int amx_plan_create(const amx_chain_desc *desc, const amx_chunk *chunks, int32_t n_chunks,
                    const int64_t *track_frame0, const int64_t *track_total_frames,
                    int32_t seg_frames, amx_plan **out) {
    if (!desc || !out || (n_chunks > 0 && !chunks) || n_chunks < 0)
        return fail(AMX_EINVAL, "amx_plan_create: null argument");
    *out = nullptr;
    const amx::PlanKnobs knobs = amx::PlanKnobs::from_env();
    // k_env0's segments are sized to the device: its CU count (256 when the query fails)
    int ncu = 256;
    if (knobs.needs_ncu(desc->multiband_on != 0)) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 3)
            ncu = 256;
    }
    std::unique_ptr<amx_plan, PlanFree> p(new (std::nothrow) amx_plan());
    if (!p) return fail(AMX_ENOMEM, "out of memory");
    std::string err;
    int rc = amx::build_plan_host(desc, chunks, n_chunks, track_frame0, track_total_frames, seg_frames, knobs, ncu,
                                  *p, err);
    if (rc) return fail(rc, "%s", err.c_str());
    if ((rc = upload_tables(p.get())) != AMX_OK) return rc;
    drop_uploaded(*p);
    if (p->resamp && (p->up_static || p->up_poly) && p->n_slow > 0) {
        if (hipStreamCreateWithFlags(&p->up_aux, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&p->up_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&p->up_join, hipEventDisableTiming) != hipSuccess)
            return fail(AMX_EHIP, "stream / event creation failed");
    }
    *out = p.release();
    return AMX_OK;
}

void amx_plan_free(amx_plan *p) {
    if (!p) return;
    for (void *q : p->owned) (void)hipFree(q);
    if (p->up_fork) (void)hipEventDestroy(p->up_fork);
    if (p->up_join) (void)hipEventDestroy(p->up_join);
    if (p->up_aux) (void)hipStreamDestroy(p->up_aux);
    delete p;
}

int amx_plan_get_info(const amx_plan *p, amx_plan_info *info) {
    if (!p || !info) return fail(AMX_EINVAL, "null argument");
    memset(info, 0, sizeof *info);
    info->workspace_bytes = (int64_t)p->ws_bytes;
    info->out_frames = p->out_frames;
    info->n_tracks = p->n_tracks;
    info->n_chunks = p->n_chunks;
    info->n_segments = p->n_seg;
    info->seg_frames = p->L;
    info->scan_levels_eq = p->lev_eq;
    info->scan_levels_xover = p->lev_x;
    info->scan_levels_kw = p->lev_kw;
    info->eq_dim = p->D;
    info->hop_frames = p->hop;
    info->meas_rate = p->meas_native ? p->cd.fs : AMX_MEAS_RATE;
    info->max_hops = p->max_hops;
    return AMX_OK;
}

int amx_plan_track_span(const amx_plan *p, int32_t track, amx_track_span *span) {
    if (!p || !span || track < 0 || track >= p->n_tracks) return fail(AMX_EINVAL, "bad track");
    const SpanDev &s = p->spans[track];
    span->out_offset = s.out_off;
    span->out_frames = s.out_n;
    span->track_frame0 = s.tframe0;
    span->track_frames_total = s.ttotal;
    return AMX_OK;
}

int amx_run_stage(amx_plan *p, int32_t stage, const float *d_in, int16_t *d_out, void *d_ws,
                  void *stream) {
    if (!p || (p->nloc > 0 && (!d_in || !d_out || !d_ws))) return fail(AMX_EINVAL, "null argument");
    if (stage < 0 || stage >= AMX_STAGE_COUNT) return fail(AMX_EINVAL, "bad stage %d", stage);
    if (p->n_seg == 0) return AMX_OK;
    hipStream_t st = (hipStream_t)stream;
    amx::Launch l{p->d_cd, p->d_chunks, p->d_segs, p->n_chunks, p->n_seg, p->L, st, p->d_lut_half,
                  p->f1_mode, p->max_chunk_n, p->an_blocks, p->an_vec, p->gin_scaled};
    int16_t *a16 = wsp<int16_t>(d_ws, p->o_a16);
    double *e = wsp<double>(d_ws, p->o_e), *s = wsp<double>(d_ws, p->o_s);
    int16_t *p16 = p->mb ? wsp<int16_t>(d_ws, p->o_p16) : nullptr;
    double *ex = p->mb ? wsp<double>(d_ws, p->o_ex) : nullptr;
    double *sx = p->mb ? wsp<double>(d_ws, p->o_sx) : nullptr;
    int16_t *bands = p->mb ? wsp<int16_t>(d_ws, p->o_bands) : nullptr;
    double *ck = p->mb ? wsp<double>(d_ws, p->o_gain) : nullptr;
    uint16_t *mframe = p->mb ? wsp<uint16_t>(d_ws, p->o_m) : nullptr;
    double *esv = p->mb ? wsp<double>(d_ws, p->o_esv) : nullptr;
    double *ee0 = p->mb ? wsp<double>(d_ws, p->o_ee0) : nullptr;
    int *eflags = p->mb ? wsp<int>(d_ws, p->o_eflags) : nullptr;
    int *eact = p->mb ? wsp<int>(d_ws, p->o_eact) : nullptr;
    int *ehead = p->mb ? wsp<int>(d_ws, p->o_ehead) : nullptr;
    int *elist = p->mb ? wsp<int>(d_ws, p->o_elist) : nullptr;
    int *eprev = p->mb ? wsp<int>(d_ws, p->o_eprev) : nullptr;
    int *elist0 = p->mb ? wsp<int>(d_ws, p->o_elist0) : nullptr;
    amx::DynLaunch dl{p->d_cd,    p->d_chunks, p->n_chunks, p->d_esegs, p->n_es,
                      p->d_eseg0, p->d_neseg,  p->nloc,     p->max_chunk_n, p->cd.look,
                      p->warm,    p->Le,       p->cd.env_rcp, p->d_tabs, st,
                      p->env_wg};
    switch (stage) {
    case AMX_STAGE_FRONT1:
        if (p->mono16) {
            int16_t *dup = wsp<int16_t>(d_ws, p->o_dup);
            HIPCHK(amx::launch_pcm_to_s16(d_in, p->in_frames, 1, AMX_PCM_S16, dup, st));
            d_in = reinterpret_cast<const float *>(dup);
        }
        HIPCHK(amx::launch_front1(l, p->D, (p->cd.chin == 2 && !p->cd.in_s16) ? 2 : 1,
                                  p->cd.analog_on != 0, d_in, p->sc ? p->d_in_lut : p->d_lut, a16, p->d_G, e,
                                  p->sc != 0));
        break;
    case AMX_STAGE_SCAN_EQ:
        if (p->D > 0)
            HIPCHK(amx::launch_scan(p->scan_eq(), e, s, nullptr, wsp<double>(d_ws, p->o_eb), st));
        break;
    case AMX_STAGE_FRONT2:
        if (p->mb)
            HIPCHK(amx::launch_front2(l, p->mask, a16, s, p16, 0, p->d_Gx, ex, nullptr, nullptr,
                                      nullptr, p->sc != 0, p->d_in_lut));
        else if (p->sc)
            HIPCHK(amx::launch_front2(l, p->mask, a16, s, d_out, 1, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, true, p->d_in_lut));
        else if (p->fuse_kw)
            HIPCHK(amx::launch_front2(l, p->mask, a16, s, d_out, 1, nullptr, nullptr, p->d_Gkw,
                                      wsp<double>(d_ws, p->o_ekw), wsp<uint32_t>(d_ws, p->o_pk)));
        else
            HIPCHK(amx::launch_front2(l, p->mask, a16, s, d_out, 1, nullptr, nullptr, nullptr,
                                      nullptr, nullptr));
        break;
    case AMX_STAGE_SCAN_XO:
        if (p->mb)
            HIPCHK(amx::launch_scan(p->scan_xo(), ex, sx, nullptr, wsp<double>(d_ws, p->o_ebx), st));
        break;
    case AMX_STAGE_XOVER:
        if (p->mb) HIPCHK(amx::launch_xover2(l, p16, sx, bands, p->nloc, eflags + AMX_ENV_BACT));
        break;
    case AMX_STAGE_RMS:
        if (p->mb) HIPCHK(amx::launch_rms(dl, bands, mframe, eflags + AMX_ENV_BACT));
        break;
    case AMX_STAGE_ENV:
        if (p->mb)
            HIPCHK(amx::launch_env(dl, mframe, ck, esv, ee0, eact, elist, ehead, eprev, elist0, eflags, p->rounds, 0));
        break;
    case AMX_STAGE_FIX:
        if (p->mb) {
            HIPCHK(amx::launch_env(dl, mframe, ck, esv, ee0, eact, elist, ehead, eprev, elist0, eflags, p->rounds, 1));
            HIPCHK(amx::launch_envseq(dl, mframe, ck, esv, ee0, eact, eflags, p->rounds));
        }
        break;
    case AMX_STAGE_APPLY:
        if (p->mb)
            HIPCHK(amx::launch_gain_overlay(dl, mframe, ck, bands, d_out, p->max_chunk_out, p->d_n1, eact,
                                            eflags + AMX_ENV_BACT));
        break;
    }
    return AMX_OK;
}

int amx_run_chunks(amx_plan *p, const float *d_in, int16_t *d_out, void *d_ws, void *stream) {
    for (int s = 0; s < AMX_STAGE_COUNT; s++) {
        int rc = amx_run_stage(p, s, d_in, d_out, d_ws, stream);
        if (rc) return rc;
    }
    return AMX_OK;
}

}  // extern "C"

namespace {
amx::UpArgs up_args(const amx_plan *p, const int16_t *d_out, const int16_t *d_edge, void *d_ws) {
    amx::UpArgs a{};
    a.cd = p->d_cd;
    a.ks = p->d_ksegs;
    a.n_kseg = p->n_kseg;
    a.spans = p->d_spans;
    a.Lin = p->upLin;
    a.Lout = p->upLout;
    a.static_l = p->up_static;
    a.poly = p->up_poly;
    a.fcnt = p->d_fcnt;
    a.bankn = p->d_bankn;
    a.hop = p->hop;
    a.obase = p->d_obase;
    a.oph = p->d_oph;
    a.owt = p->d_owt;
    a.lin = p->up_lin;
    a.slow = p->d_slow;
    a.n_slow = p->n_slow;
    a.bank = p->d_bank;
    a.taps = p->up_taps;
    a.alloc = p->up_alloc;
    a.x = reinterpret_cast<const uint32_t *>(d_out);
    a.edge = reinterpret_cast<const uint32_t *>(d_edge);
    a.G = p->d_Gkw;
    a.qh = p->d_qh;
    a.qt = p->d_qt;
    a.eterms = wsp<double>(d_ws, p->o_eterms);
    a.e = wsp<double>(d_ws, p->o_ekw);
    a.s = wsp<double>(d_ws, p->o_skw);
    a.parts = wsp<double>(d_ws, p->o_parts);
    a.part_hop = wsp<int64_t>(d_ws, p->o_phop);
    a.pk = wsp<uint32_t>(d_ws, p->o_pk);
    return a;
}
// the plan's resampler to 192 kHz as loudnorm's upsamplers take it
amx::SwrDev swr_dev(const amx_plan *p) {
    return amx::SwrDev{p->up_pc, p->up_lin, p->up_src, p->up_dst, p->d_bank, p->up_taps, p->up_alloc};
}
// ---- loudnorm's 192 kHz modes: scratch layout (amx_loudnorm.hip)
#define LN_FIRST_FRAMES 576000     // frame_size(192000, 3000)
struct LnLayout {
    int T = 0, nb_last = 0, Fs = 4, Wf = 3, J = 0, M = 0, K = 0, P = 0;
    int64_t o_u = 0, o_ring = 0, o_ctl = 0, o_dctl = 0, o_v = 0, o_hold = 0, o_D = 0, o_G = 0, o_ramp = 0;
    int64_t o_recG = 0, o_recE = 0, o_wrec = 0, o_cnt = 0, o_match = 0, o_rings = 0, o_wring = 0, o_bm = 0;
    int64_t o_bmF = 0;
    int64_t total = 0;
};
// INNER frames, segments of Fs frames each warmed up Wf frames (AMX_LN_WARM, default 2)
// before its start, at most P persistent k_lp_seg workgroups of AMX_LP_NT lanes (3072
// waves: three per SIMD, k_lp_seg's register budget).  Fs (AMX_LN_SEG overrides) is the
// smallest >= 2 whose segments fit the P waves: a
// wave then runs one segment, Fs + Wf frames (r04m: a 5-min track 11.9 -> 9.1 ms per
// dynamic step from Fs 4 / Wf 3 / 1024 waves); a longer track takes longer segments, so
// the warm-up share Wf / Fs shrinks instead of waves running several segments each.
LnLayout ln_layout(int64_t n192, int64_t u_frames = -1, int p_cap = -1) {
    LnLayout l;
    l.Wf = 2;
    const int pmax = 3072 / (AMX_LP_NT / 64);
    if (n192 >= LN_FIRST_FRAMES) {
        l.T = (int)((n192 - LN_FIRST_FRAMES + 19199) / 19200);
        l.nb_last = l.T > 0 ? (int)(n192 - LN_FIRST_FRAMES - 19200LL * (l.T - 1)) : 0;
    }
    l.Fs = std::max(2, (l.T + (pmax - 32) - 1) / (pmax - 32));
    if (const char *ev = std::getenv("AMX_LN_SEG")) l.Fs = std::max(1, std::atoi(ev));
    if (const char *ev = std::getenv("AMX_LN_WARM")) l.Wf = std::max(0, std::atoi(ev));
    // boundaries only at full INNER frames (a partial last frame's wrap reads reach the
    // frame before it), at FINAL's start and inside FINAL
    const int t_ok = (l.T > 0 && l.nb_last == 19200) ? l.T : l.T - 1;
    l.J = t_ok >= 1 + l.Fs ? (t_ok - 1) / l.Fs : 0;
    l.M = (29 + l.Fs - 1) / l.Fs;
    l.K = 1 + l.J + l.M;
    l.P = std::min(l.K, pmax);
    if (p_cap > 0) l.P = std::min(l.P, p_cap);     // a window's segments need no more waves
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += ((bytes + 255) / 256) * 256; return at; };
    l.o_u = take((u_frames < 0 ? n192 : u_frames) * 2 * (int64_t)sizeof(float));
    l.o_ring = take(AMX_LN_MC_RING(2) * (int64_t)sizeof(double));
    l.o_ctl = take(16 * sizeof(int));
    l.o_dctl = take(8 * sizeof(double));
    l.o_v = take((int64_t)l.T * sizeof(double));
    l.o_hold = take((int64_t)l.T * sizeof(int));
    l.o_D = take((int64_t)l.T * sizeof(double));
    l.o_G = take((int64_t)(l.T + 1) * sizeof(double));
    l.o_ramp = take(19200 * sizeof(double));
    l.o_recG = take((int64_t)l.K * AMX_LN_REC * sizeof(double));
    l.o_recE = take((int64_t)l.K * AMX_LN_REC * sizeof(double));
    l.o_wrec = take(2 * AMX_LN_REC * sizeof(double));
    l.o_cnt = take((int64_t)(l.K + 1) * sizeof(int));
    l.o_match = take((int64_t)(l.K + 1) * sizeof(int));
    l.o_rings = take((int64_t)l.P * AMX_LN_RING * 2 * sizeof(double));
    l.o_wring = take((int64_t)AMX_LN_RING * 2 * sizeof(double));
    l.o_bm = take((n192 / 64 + 2) * (int64_t)sizeof(double));
    l.o_bmF = take((n192 / 64 + 2) * (int64_t)sizeof(double));
    l.total = o;
    return l;
}
// the 192 kHz stream's frames of a whole track (the resampler's output, or the track
// itself when it already is 192 kHz)
int ln_frames(const amx_plan *p, int32_t track, int64_t *n192) {
    if (p->meas_native || (p->resamp && !p->up_ok))
        return fail(AMX_ERANGE, "loudnorm's 192 kHz modes need a 192 kHz upsampler (input above 192 kHz)");
    const SpanDev &sp = p->spans[track];
    *n192 = p->resamp ? (sp.out_n * p->upL + p->upM - 1) / p->upM : sp.out_n;
    return AMX_OK;
}
// the first output position of segment k: its frame (k_lp_*'s lp_seg_start) and that
// frame's base (lp_frame: INNER frames from 0, FINAL's from S0)
int64_t ln_seg_base(const LnLayout &lo, int64_t n192, int k) {
    const int phi = k == 0 ? 0 : (k <= lo.J ? 1 + k * lo.Fs : lo.T + 1 + (k - lo.J - 1) * lo.Fs);
    const int64_t S0 = n192 - (LN_FIRST_FRAMES - 19200);
    return phi <= lo.T ? (int64_t)19200 * phi : S0 + (int64_t)19200 * (phi - lo.T - 1);
}
// af_loudnorm's init_gaussian_filter: the 21 weights of its gain smoothing
void ln_gaussian_weights(double *weights) {
    double total = 0.0;
    const double sigma = 3.5;
    const int off = 21 / 2;
    const double c1 = 1.0 / (sigma * std::sqrt(2.0 * M_PI));
    const double c2 = 2.0 * std::pow(sigma, 2.0);
    for (int i = 0; i < 21; i++) {
        const int x = i - off;
        weights[i] = c1 * std::exp(-(std::pow(x, 2.0) / c2));
        total += weights[i];
    }
    const double adjust = 1.0 / total;
    for (int i = 0; i < 21; i++) weights[i] *= adjust;
}
int check_edges(const amx_plan *p, const int16_t *d_edge) {
    if (!p->resamp || d_edge) return AMX_OK;
    for (const SpanDev &sp : p->spans)
        if (sp.out_n > 0 && (sp.edge_lo || sp.edge_hi))
            return fail(AMX_EINVAL, "a span inside its track needs the neighbour frames (d_edge)");
    return AMX_OK;
}
}  // namespace

extern "C" {

int amx_loudness_pass1_part(amx_plan *p, int32_t part, const int16_t *d_out, const int16_t *d_edge,
                            double *d_kw_tail, double *d_peak, void *d_ws, void *stream) {
    if (!p || !d_peak || (p->n_kseg > 0 && (!d_out || !d_ws)))
        return fail(AMX_EINVAL, "null argument");
    if (part != 0 && part != 1) return fail(AMX_EINVAL, "bad part %d", part);
    if (p->resamp && !p->up_ok)
        return fail(AMX_ERANGE, "%d Hz has no 192 kHz upsampler (loudnorm pass 1)",
                    p->cd.fs);
    if (int rc = check_edges(p, d_edge)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *e = wsp<double>(d_ws, p->o_ekw), *s = wsp<double>(d_ws, p->o_skw);
    uint32_t *pk = wsp<uint32_t>(d_ws, p->o_pk);
    if (part == 0) {
        // the pass over the samples: per K segment the zero-state end state (and, at
        // 192 kHz, the peaks and energy terms; amx_loud192.hip)
        p->kw_rest_states = 0;
        p->kw_eb_ready = 0;
        if (p->n_kseg == 0) return AMX_OK;
        if (p->resamp)
            HIPCHK(amx::launch_up1(up_args(p, d_out, d_edge, d_ws), st, p->up_aux, p->up_fork, p->up_join));
        else if (!p->fuse_kw)  // else the GEMV + per-segment peaks were made by k_front2 (amx_run_chunks)
            HIPCHK(amx::launch_kw1(p->d_cd, p->d_ksegs, p->n_kseg, p->Lkw, d_out, p->d_Gkw, e, pk, p->gate, st));
        return AMX_OK;
    }
    // k_peak_reduce writes every track's peak; only tracks without a K segment (empty
    // spans) need the zero written here
    if (p->any_empty_span || p->n_kseg == 0)
        HIPCHK(amx::launch_zero(d_peak, sizeof(double) * 4 * (size_t)p->n_tracks, st));
    if (p->n_kseg == 0) {
        if (d_kw_tail) HIPCHK(amx::launch_zero(d_kw_tail, sizeof(double) * 8 * (size_t)p->n_tracks, st));
        return AMX_OK;
    }
    HIPCHK(amx::launch_peak_reduce(p->d_spans, p->n_tracks, p->max_nkseg, pk, d_peak, p->d_pcnt,
                                   p->d_ppart, p->d_ksegs, p->Lkw, d_out, p->d_Gkw, e, p->fuse_kw,
                                   p->resamp, st));
    // the span tails from the scan's own down sweep unless a span is empty (its tail is 0:
    // k_kw_tail writes it)
    const bool tail_fused = d_kw_tail && !p->any_empty_span;
    HIPCHK(amx::launch_scan(p->scan_kw(), e, s, nullptr, wsp<double>(d_ws, p->o_ebk), st, true,
                            tail_fused ? p->d_tailpow : nullptr, tail_fused ? d_kw_tail : nullptr));
    p->kw_rest_states = 1;   // s = the start states from rest: pass 2 without a carry reuses them
    p->kw_eb_ready = 1;      // and the block sums: pass 2 with a carry runs the down sweep only
    if (d_kw_tail && !tail_fused)
        HIPCHK(amx::launch_kw_tail(p->d_spans, p->n_tracks, s, e, p->d_tailpow, d_kw_tail, st));
    return AMX_OK;
}

int amx_loudness_pass1(amx_plan *p, const int16_t *d_out, const int16_t *d_edge, double *d_kw_tail,
                       double *d_peak, void *d_ws, void *stream) {
    int rc = amx_loudness_pass1_part(p, 0, d_out, d_edge, d_kw_tail, d_peak, d_ws, stream);
    if (rc) return rc;
    return amx_loudness_pass1_part(p, 1, d_out, d_edge, d_kw_tail, d_peak, d_ws, stream);
}

int amx_loudnorm_192k_size(const amx_plan *p, int32_t track, int64_t *frames, int64_t *ws_bytes) {
    if (!p || !frames || !ws_bytes || track < 0 || track >= p->n_tracks) return fail(AMX_EINVAL, "bad argument");
    int64_t n192 = 0;
    if (int rc = ln_frames(p, track, &n192)) return rc;
    *frames = n192;
    *ws_bytes = ln_layout(n192).total;
    return AMX_OK;
}

}  // extern "C"

namespace {
// af_loudnorm init / config_input for k_ln_dyn: the tables, the dB options as the linear
// factors it keeps, the Gaussian weights and the K filter at 192 kHz
void ln_options(const amx_plan *p, const amx_loudnorm_desc *d, amx::LnArgs &a) {
    a.energies = p->d_energies;
    a.bounds = p->d_bounds;
    a.target_i = d->target_i;
    a.target_lra = d->target_lra;
    a.target_tp = std::pow(10., d->target_tp / 20.);
    a.measured_i = d->measured_i;
    a.measured_thresh = d->measured_thresh;
    a.offset = std::pow(10., d->offset / 20.);
    ln_gaussian_weights(a.weights);
    for (int k = 0; k < 5; k++) { a.kb[k] = p->kdf_b[k]; a.ka[k] = p->kdf_a[k]; }
}
// the kernels' arguments of one filter run of track `track` (amx_loudnorm_192k_ex / _shard)
int ln_args(amx_plan *p, int32_t track, const amx_loudnorm_desc *d, const double *d_measured,
            const double *d_offset_i, const int32_t *d_gate, const int16_t *d_out, const double *d_hops,
            int64_t max_hops, const double *d_peak, int16_t *d_y192, double *d_summary, void *d_ws2,
            amx::LnArgs &a, amx::LpArgs &q, int64_t &n192, int64_t u_lo = 0, int64_t u_frames = -1,
            int64_t y_lo = 0, int p_cap = -1) {
    if (!p || track < 0 || track >= p->n_tracks) return fail(AMX_EINVAL, "bad argument");
    n192 = 0;
    if (int rc = ln_frames(p, track, &n192)) return rc;
    if (!d || !d_out || !d_hops || !d_peak || !d_y192 || !d_summary || !d_ws2)
        return fail(AMX_EINVAL, "null argument");
    const SpanDev &sp = p->spans[track];
    if (sp.tframe0 != 0 || sp.ttotal != sp.out_n)
        return fail(AMX_EINVAL, "loudnorm's 192 kHz modes run on whole tracks (one plan holds the track)");
    if (max_hops < n192 / 19200 + 1) return fail(AMX_EINVAL, "d_hops holds %lld hops", (long long)max_hops);
    const LnLayout lo = ln_layout(n192, u_frames, p_cap);
    char *w = reinterpret_cast<char *>(d_ws2);
    a = amx::LnArgs{};
    a.n192 = n192;
    // a window (amx_ln_shard.windowed): u holds positions [u_lo, ..) and d_y192 starts at
    // position y_lo; the kernels index whole-track positions, so the bases move back
    // (only positions inside the windows are ever touched)
    a.u = reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(w + lo.o_u) - (uintptr_t)u_lo * 2 * sizeof(float));
    a.ring = reinterpret_cast<double *>(w + lo.o_ring);
    a.y = reinterpret_cast<int16_t *>(reinterpret_cast<uintptr_t>(d_y192) - (uintptr_t)y_lo * 2 * sizeof(int16_t));
    a.summary = d_summary;
    a.hops = d_hops + (int64_t)track * max_hops * 2;
    a.peak = d_peak + (int64_t)track * 4;
    ln_options(p, d, a);
    q = amx::LpArgs{};
    q.n = n192;
    q.S0 = n192 - (LN_FIRST_FRAMES - 19200);
    q.T = lo.T;
    q.nb_last = lo.nb_last;
    q.Fs = lo.Fs;
    q.Wf = lo.Wf;
    q.J = lo.J;
    q.M = lo.M;
    q.K = lo.K;
    q.P = lo.P;
    q.u = a.u;
    q.hops = a.hops;
    q.energies = a.energies;
    q.bounds = a.bounds;
    q.target_i = a.target_i;
    q.target_lra = a.target_lra;
    q.ceiling = a.target_tp;
    q.measured_i = a.measured_i;
    q.measured_thresh = a.measured_thresh;
    q.offset = a.offset;
    q.measured_src = d_measured;
    q.offset_src = d_offset_i;
    q.gate = d_gate;
    for (int i = 0; i < 21; i++) q.weights[i] = a.weights[i];
    q.v = reinterpret_cast<double *>(w + lo.o_v);
    q.hold = reinterpret_cast<int *>(w + lo.o_hold);
    q.D = reinterpret_cast<double *>(w + lo.o_D);
    q.G = reinterpret_cast<double *>(w + lo.o_G);
    q.ramp = reinterpret_cast<double *>(w + lo.o_ramp);
    q.recG = reinterpret_cast<double *>(w + lo.o_recG);
    q.recE = reinterpret_cast<double *>(w + lo.o_recE);
    q.wrec = reinterpret_cast<double *>(w + lo.o_wrec);
    q.cnt = reinterpret_cast<int *>(w + lo.o_cnt);
    q.match = reinterpret_cast<int *>(w + lo.o_match);
    q.rings = reinterpret_cast<double *>(w + lo.o_rings);
    q.wring = reinterpret_cast<double *>(w + lo.o_wring);
    q.ctl = reinterpret_cast<int *>(w + lo.o_ctl);
    q.dctl = reinterpret_cast<double *>(w + lo.o_dctl);
    q.y = a.y;
    q.summary = d_summary;
    a.lp_ctl = q.ctl;
    a.lp_dctl = q.dctl;
    a.lp_D = q.D;
    a.lp_recG = q.recG;
    a.lp_Fs = q.Fs;
    a.lp_J = q.J;
    a.lp_tstop = INT_MAX;
    q.kb = 0;
    q.ke = q.K;
    // k_lp_fill + the skipping scan + the sparse emit (AMX_LP_FILL=0: the dense form, the
    // tests' cross-check of the sparse one), with FINAL's bound
    const char *fe = std::getenv("AMX_LP_FILL");
    q.bm = (fe && std::atoi(fe) == 0) ? nullptr : reinterpret_cast<double *>(w + lo.o_bm);
    q.bmF = q.bm ? reinterpret_cast<double *>(w + lo.o_bmF) : nullptr;
    return AMX_OK;
}
}  // namespace

extern "C" {

int amx_loudnorm_192k_ex(amx_plan *p, int32_t track, const amx_loudnorm_desc *d, const double *d_measured,
                         const double *d_offset_i, const int32_t *d_gate, const int16_t *d_out, const double *d_hops,
                         int64_t max_hops, const double *d_peak, int16_t *d_y192, double *d_summary,
                         void *d_ws2, void *stream) {
    amx::LnArgs a;
    amx::LpArgs q;
    int64_t n192 = 0;
    if (int rc = ln_args(p, track, d, d_measured, d_offset_i, d_gate, d_out, d_hops, max_hops, d_peak, d_y192,
                         d_summary, d_ws2, a, q, n192))
        return rc;
    const SpanDev &sp = p->spans[track];
    const amx::SwrDev r = swr_dev(p);
    HIPCHK(amx::launch_loudnorm(a, q, reinterpret_cast<const uint32_t *>(d_out) + sp.out_off, sp.out_n, r,
                                d->reuse_stream == 0, (hipStream_t)stream));
    return AMX_OK;
}

int amx_loudnorm_192k_shard(amx_plan *p, int32_t track, const amx_loudnorm_desc *d, const double *d_measured,
                            const double *d_offset_i, const amx_ln_shard *sh, const int16_t *d_out,
                            const double *d_hops, int64_t max_hops, const double *d_peak, int16_t *d_y192,
                            double *d_summary, void *d_ws2, void *stream) {
    if (!sh || sh->part < 0 || sh->part > 3) return fail(AMX_EINVAL, "bad shard");
    if (sh->part == 3 && sh->kb != 0) return fail(AMX_EINVAL, "part 3 (a quiet start) runs on the first segments' rank");
    amx::LnArgs a;
    amx::LpArgs q;
    int64_t n192 = 0;
    if (!p || track < 0 || track >= p->n_tracks) return fail(AMX_EINVAL, "bad argument");
    if (int rc = ln_frames(p, track, &n192)) return rc;
    int64_t win[9] = {0, 0, sh->u_lo, sh->u_hi, 0, 0, 0, 0, 0};
    if (sh->windowed || sh->u_lo < 0) {
        int64_t wsb = 0;
        if (int rc = amx_loudnorm_192k_shard_window(p, track, sh->kb, sh->ke, win, &wsb)) return rc;
    }
    const int64_t u_lo = win[2], u_hi = win[3];
    if (int rc = ln_args(p, track, d, d_measured, d_offset_i, nullptr, d_out, d_hops, max_hops, d_peak, d_y192,
                         d_summary, d_ws2, a, q, n192, sh->windowed ? u_lo : 0, sh->windowed ? u_hi - u_lo : -1,
                         sh->windowed ? win[4] : 0, sh->windowed ? sh->ke - sh->kb : -1))
        return rc;
    if (sh->kb < 0 || sh->ke > q.K || sh->kb > sh->ke) return fail(AMX_EINVAL, "segments [%d, %d) of %d", sh->kb, sh->ke, q.K);
    if (u_hi > n192 || u_lo > u_hi) return fail(AMX_EINVAL, "bad 192 kHz range");
    if (sh->part == 2 && sh->kb > 0 && !sh->d_rec_in) return fail(AMX_EINVAL, "segment %d needs the true state", sh->kb);
    q.kb = sh->kb;
    q.ke = sh->ke;
    // part 3: a hand-over at segment k needs the INNER frames < k Fs; the last segment this
    // rank may hand over at is ke - 1 (a later lift: the replicated form)
    if (sh->part == 3) a.lp_tstop = sh->ke - 1 > 0 ? (sh->ke - 1) * q.Fs : 0;
    q.rec_in = sh->kb > 0 ? sh->d_rec_in : nullptr;
    q.rec_out = sh->ke < q.K ? sh->d_rec_out : nullptr;
    const SpanDev &sp = p->spans[track];
    const amx::SwrDev r = swr_dev(p);
    // the positions segments [kb, ke) emit
    const LnLayout lo = ln_layout(n192);
    const int64_t y_lo = ln_seg_base(lo, n192, sh->kb), y_hi = sh->ke < lo.K ? ln_seg_base(lo, n192, sh->ke) : n192;
    // windowed: d_out holds track frames [x_lo, x_hi) (the base moves back to frame 0)
    const uint32_t *x = sh->windowed
                            ? reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(d_out) -
                                                                 (uintptr_t)win[0] * sizeof(uint32_t))
                            : reinterpret_cast<const uint32_t *>(d_out) + sp.out_off;
    HIPCHK(amx::launch_loudnorm_shard(a, q, x, sp.out_n, r, u_lo, u_hi, y_lo, y_hi, sh->part, d->reuse_stream == 0,
                                      (hipStream_t)stream));
    return AMX_OK;
}

int amx_loudnorm_192k_shard_window(const amx_plan *p, int32_t track, int32_t kb, int32_t ke, int64_t *win,
                                   int64_t *ws_bytes) {
    if (!p || track < 0 || track >= p->n_tracks || !win || !ws_bytes) return fail(AMX_EINVAL, "bad argument");
    int64_t n192 = 0;
    if (int rc = ln_frames(p, track, &n192)) return rc;
    const LnLayout lo = ln_layout(n192);
    if (kb < 0 || ke > lo.K || kb >= ke) return fail(AMX_EINVAL, "segments [%d, %d) of %d", kb, ke, lo.K);
    // what segments [kb, ke) read: from Wf + 2 frames before the first one's start (its
    // warm-up) to a ring and two frames past the last one's end
    const int64_t u_lo = std::max<int64_t>(0, ln_seg_base(lo, n192, kb) - (int64_t)19200 * (lo.Wf + 2));
    const int64_t u_hi = ke < lo.K ? std::min<int64_t>(n192, ln_seg_base(lo, n192, ke) + AMX_LN_RING + 2 * 19200) : n192;
    // the chain frames the resampler reads for them: output j's window starts at frame
    // floor(j M / L) - 15 (32 taps), with a margin; 192 kHz input: the positions themselves
    const SpanDev &sp = p->spans[track];
    int64_t x_lo = u_lo, x_hi = u_hi;
    if (p->resamp) {
        const int64_t m = p->up_alloc + 8;       // the window's reach (center + the row)
        x_lo = std::max<int64_t>(0, (int64_t)((__int128)u_lo * p->upM / p->upL) - m);
        x_hi = std::min<int64_t>(sp.out_n, (int64_t)(((__int128)u_hi * p->upM + p->upL - 1) / p->upL) + m);
    }
    win[0] = x_lo;
    win[1] = x_hi;
    win[2] = u_lo;
    win[3] = u_hi;
    win[4] = ln_seg_base(lo, n192, kb);
    win[5] = ke < lo.K ? ln_seg_base(lo, n192, ke) : n192;
    const LnLayout lw = ln_layout(n192, u_hi - u_lo, ke - kb);
    win[6] = lw.o_ctl;
    win[7] = lw.o_D;       // (ABI 4) the INNER frames' deltas, T doubles (a quiet start's hand-over)
    win[8] = lw.T;
    *ws_bytes = lw.total;
    return AMX_OK;
}

int amx_loudnorm_192k_segments(const amx_plan *p, int32_t track, int64_t *starts, int32_t cap, int32_t *K,
                               int32_t *k_fin, int32_t *rec_doubles, int64_t *ctl_offset) {
    if (!p || track < 0 || track >= p->n_tracks || !K) return fail(AMX_EINVAL, "bad argument");
    int64_t n192 = 0;
    if (int rc = ln_frames(p, track, &n192)) return rc;
    const LnLayout lo = ln_layout(n192);
    *K = lo.K;
    if (k_fin) *k_fin = lo.J + 1;
    if (rec_doubles) *rec_doubles = AMX_LN_REC;
    if (ctl_offset) *ctl_offset = lo.o_ctl;
    if (starts) {
        if (cap < lo.K + 1) return fail(AMX_EINVAL, "starts holds %d, needs %d", cap, lo.K + 1);
        for (int k = 0; k < lo.K; k++) starts[k] = ln_seg_base(lo, n192, k);
        starts[lo.K] = n192;
    }
    return AMX_OK;
}

int amx_loudnorm_192k(amx_plan *p, int32_t track, const amx_loudnorm_desc *d, const int16_t *d_out,
                      const double *d_hops, int64_t max_hops, const double *d_peak, int16_t *d_y192,
                      double *d_summary, void *d_ws2, void *stream) {
    return amx_loudnorm_192k_ex(p, track, d, nullptr, nullptr, nullptr, d_out, d_hops, max_hops, d_peak, d_y192,
                                d_summary, d_ws2, stream);
}

int amx_pcm_to_s16(const void *d_raw, int64_t frames, int32_t channels, int32_t format,
                   int16_t *d_out, void *stream) {
    if (frames < 0 || (frames > 0 && (!d_raw || !d_out))) return fail(AMX_EINVAL, "null argument");
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "channels must be 1..8");
    if (format < AMX_PCM_U8 || format > AMX_PCM_F64BE) return fail(AMX_EINVAL, "bad PCM format %d", format);
    HIPCHK(amx::launch_pcm_to_s16(d_raw, frames, channels, format, d_out, (hipStream_t)stream));
    return AMX_OK;
}

static int flac_encode_args(int64_t frames, int32_t channels, int32_t block, int32_t lpc_order) {
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "channels must be 1..8");
    if (frames < 1) return fail(AMX_EINVAL, "frames must be >= 1");
    if (block < 16 || block > 4608) return fail(AMX_ERANGE, "block size %d outside 16..4608", block);
    if (lpc_order < 0 || lpc_order > 8) return fail(AMX_ERANGE, "lpc_order %d outside 0..8", lpc_order);
    return AMX_OK;
}

int amx_flac_encode_size_ex(int64_t frames, int32_t channels, int32_t block, int32_t lpc_order,
                            int64_t *n_frames, int64_t *max_out_bytes, int64_t *workspace_bytes) {
    if (!n_frames || !max_out_bytes || !workspace_bytes) return fail(AMX_EINVAL, "null argument");
    const int rc = flac_encode_args(frames, channels, block, lpc_order);
    if (rc != AMX_OK) return rc;
    amx::flac_encode_size(frames, channels, block, lpc_order, n_frames, max_out_bytes, workspace_bytes);
    return AMX_OK;
}

int amx_flac_encode_size(int64_t frames, int32_t channels, int32_t block, int64_t *n_frames,
                         int64_t *max_out_bytes, int64_t *workspace_bytes) {
    return amx_flac_encode_size_ex(frames, channels, block, 0, n_frames, max_out_bytes, workspace_bytes);
}

int amx_flac_encode(const int16_t *d_pcm, int64_t frames, int32_t channels, int32_t sample_rate,
                    int32_t block, uint8_t *d_out, int64_t out_capacity, uint32_t *d_frame_bytes,
                    uint32_t *d_sub_bits, int64_t *d_total_bytes, void *workspace,
                    int64_t workspace_bytes, void *stream) {
    return amx_flac_encode_ex(d_pcm, frames, channels, sample_rate, block, 0, d_out, out_capacity, d_frame_bytes,
                              d_sub_bits, d_total_bytes, workspace, workspace_bytes, stream);
}

int amx_flac_encode_ex(const int16_t *d_pcm, int64_t frames, int32_t channels, int32_t sample_rate,
                       int32_t block, int32_t lpc_order, uint8_t *d_out, int64_t out_capacity,
                       uint32_t *d_frame_bytes, uint32_t *d_sub_bits, int64_t *d_total_bytes, void *workspace,
                       int64_t workspace_bytes, void *stream) {
    if (!d_pcm || !d_out || !d_frame_bytes || !d_total_bytes || !workspace)
        return fail(AMX_EINVAL, "null argument");
    const int rc = flac_encode_args(frames, channels, block, lpc_order);
    if (rc != AMX_OK) return rc;
    if (sample_rate < 1 || sample_rate > 1048575)
        return fail(AMX_ERANGE, "sample rate %d outside 1..1048575", sample_rate);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(AMX_EINVAL, "workspace must be 8-byte aligned");
    int64_t nf, max_out, ws_bytes;
    amx::flac_encode_size(frames, channels, block, lpc_order, &nf, &max_out, &ws_bytes);
    if (out_capacity < max_out)
        return fail(AMX_ERANGE, "out_capacity %lld < %lld (amx_flac_encode_size)", (long long)out_capacity,
                    (long long)max_out);
    if (workspace_bytes < ws_bytes)
        return fail(AMX_ERANGE, "workspace_bytes %lld < %lld (amx_flac_encode_size)", (long long)workspace_bytes,
                    (long long)ws_bytes);
    HIPCHK(amx::launch_flac_encode(d_pcm, frames, channels, sample_rate, block, lpc_order, d_out, out_capacity,
                                   d_frame_bytes, d_sub_bits, d_total_bytes, workspace, (hipStream_t)stream));
    return AMX_OK;
}

int amx_flac_decode_device(const uint8_t *d_data, int64_t size, const amx_flac_cand_t *d_cand,
                           const amx_flac_scan_t *scan, int32_t *d_out, int64_t out_frames, int32_t *d_blocks,
                           int64_t max_blocks, int64_t *d_result, void *d_workspace, int64_t workspace_bytes,
                           void *stream) {
    if (!d_data || !d_cand || !scan || !d_out || !d_blocks || !d_result || !d_workspace)
        return fail(AMX_EINVAL, "null argument");
    if (size < 42 || scan->n_cand < 1 || scan->n_cand > INT32_MAX || scan->channels < 1 || scan->channels > 8 ||
        scan->total_frames < 1 || scan->scratch_samples < 0 || scan->first_frame < 42 || scan->first_frame >= size ||
        scan->bits_per_sample < 4 || scan->bits_per_sample > 24)
        return fail(AMX_EINVAL, "not a scan amx_flac_scan accepted");
    if (reinterpret_cast<uintptr_t>(d_workspace) & 15) return fail(AMX_EINVAL, "workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & 3 || reinterpret_cast<uintptr_t>(d_blocks) & 3 ||
        reinterpret_cast<uintptr_t>(d_result) & 7 || reinterpret_cast<uintptr_t>(d_cand) & 7)
        return fail(AMX_EINVAL, "misaligned argument");
    if (out_frames < scan->total_frames)
        return fail(AMX_ERANGE, "out_frames %lld < %lld", (long long)out_frames, (long long)scan->total_frames);
    if (max_blocks < 1) return fail(AMX_ERANGE, "max_blocks %lld < 1", (long long)max_blocks);
    const int64_t need = amx::flac_decode_ws_bytes(scan->n_cand, scan->scratch_samples);
    if (workspace_bytes < need)
        return fail(AMX_ERANGE, "workspace_bytes %lld < %lld (amx_flac_scan)", (long long)workspace_bytes,
                    (long long)need);
    HIPCHK(amx::launch_flac_decode(d_data, size, d_cand, scan->n_cand, scan->channels, scan->total_frames,
                                   scan->first_frame, scan->scratch_samples, d_out, d_blocks, max_blocks, d_result,
                                   d_workspace, (hipStream_t)stream));
    return AMX_OK;
}

int amx_plan_set_gate(amx_plan *p, const int32_t *d_gate) {
    if (!p) return fail(AMX_EINVAL, "null plan");
    p->gate = d_gate;
    return AMX_OK;
}

int amx_plan_set_limiter_trace(amx_plan *p, double *d_att) {
    if (!p) return fail(AMX_EINVAL, "null plan");
    p->lim_att = d_att;
    return AMX_OK;
}

int amx_plan_set_limiter_channels(amx_plan *p, int32_t channels) {
    if (!p) return fail(AMX_EINVAL, "null plan");
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "%d channels", channels);
    p->lim_channels = channels < 2 ? 2 : channels;     // mono is limited as stereo (:190)
    return AMX_OK;
}

int amx_plan_set_publish(amx_plan *p, int32_t *h_ctl) {
    if (!p) return fail(AMX_EINVAL, "null plan");
    p->publish = h_ctl;
    return AMX_OK;
}

int amx_env_counters(const amx_plan *p, const void *d_ws, int32_t *out, int32_t n) {
    if (!p || !out || n < 0) return fail(AMX_EINVAL, "null argument");
    const int32_t have = AMX_ENV_MAX_ROUNDS * AMX_ENV_NCTR;
    for (int32_t i = 0; i < n; i++) out[i] = 0;
    if (!p->mb) return AMX_OK;
    // the word after the counters: the plan's division form (ChainDev::env_rcp; a host value)
    if (n > have) out[have] = p->cd.env_rcp;
    if (p->n_es == 0) return AMX_OK;
    if (!d_ws) return fail(AMX_EINVAL, "null workspace");
    const int32_t k = n < have ? n : have;
    HIPCHK(hipMemcpy(out, reinterpret_cast<const char *>(d_ws) + p->o_eflags + AMX_ENV_MAX_ROUNDS * 4,
                     (size_t)k * 4, hipMemcpyDeviceToHost));
    return AMX_OK;
}

int amx_kw_propagate(const amx_plan *p, int64_t frames, const double *in8, double *out8) {
    if (!p || !in8 || !out8 || frames < 0) return fail(AMX_EINVAL, "bad argument");
    Mat P = p->kw_model.pow(frames);
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < AMX_KW_DIM; i++) {
            double acc = 0.0;
            for (int k = 0; k < AMX_KW_DIM; k++) acc += P[(size_t)i * AMX_KW_DIM + k] * in8[c * 4 + k];
            out8[c * 4 + i] = acc;
        }
    return AMX_OK;
}

int amx_loudness_pass2(amx_plan *p, const int16_t *d_out, const int16_t *d_edge,
                       const double *d_kw_carry, double *d_hops, int64_t max_hops, void *d_ws,
                       void *stream) {
    if (!p || !d_hops || max_hops <= 0 || (p->n_kseg > 0 && (!d_out || !d_ws)))
        return fail(AMX_EINVAL, "null argument");
    if (p->resamp && !p->up_ok)
        return fail(AMX_ERANGE, "%d Hz has no 192 kHz upsampler (loudnorm pass 1)",
                    p->cd.fs);
    if (max_hops < p->max_hops) return fail(AMX_EINVAL, "max_hops %lld < %lld", (long long)max_hops,
                                            (long long)p->max_hops);
    if (int rc = check_edges(p, d_edge)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->n_kseg == 0) {
        HIPCHK(amx::launch_zero(d_hops, sizeof(double) * 2 * (size_t)max_hops * p->n_tracks, st));
        return AMX_OK;
    }
    double *e = wsp<double>(d_ws, p->o_ekw), *s = wsp<double>(d_ws, p->o_skw);
    double *parts = wsp<double>(d_ws, p->o_parts);
    int64_t *phop = wsp<int64_t>(d_ws, p->o_phop);
    if (d_kw_carry || !p->kw_rest_states) {
        // the block sums do not depend on the carry: after pass 1 only the down sweep runs
        HIPCHK(amx::launch_scan(p->scan_kw(), e, s, d_kw_carry, wsp<double>(d_ws, p->o_ebk), st, !p->kw_eb_ready));
        p->kw_eb_ready = 1;
        p->kw_rest_states = d_kw_carry ? 0 : 1;
    }
    if (p->resamp)
        HIPCHK(amx::launch_up2(up_args(p, d_out, d_edge, d_ws), st));
    else
        HIPCHK(amx::launch_kw2(p->d_cd, p->d_ksegs, p->n_kseg, p->Lkw, p->hop, d_out, s, parts, phop,
                               p->kw_aligned, p->gate, st));
    HIPCHK(amx::launch_hops(p->d_spans, p->n_tracks, p->d_ksegs, p->resamp ? p->upLout : p->Lkw,
                            p->hop, parts, phop, d_hops, max_hops, st));
    return AMX_OK;
}

int amx_loudness_histograms(amx_plan *p, const double *d_hops, int64_t max_hops, uint64_t *d_hist,
                            uint64_t *d_st_hist, void *d_ws, void *stream) {
    (void)d_ws;
    if (!p || !d_hops || !d_hist || !d_st_hist || max_hops <= 0)
        return fail(AMX_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(amx::launch_hist(p->d_spans, p->n_tracks, p->hop, d_hops, max_hops, p->d_bounds,
                            reinterpret_cast<unsigned long long *>(d_hist),
                            reinterpret_cast<unsigned long long *>(d_st_hist), st));
    return AMX_OK;
}

int amx_limiter_geometry(const amx_plan *p, const amx_final_desc *fd, int32_t *buffer_size,
                         int32_t *halo_frames, int64_t *state_doubles) {
    if (!p || !fd) return fail(AMX_EINVAL, "null argument");
    const int channels = 2;
    double attack = fd->attack_ms / 1000.0;
    int bs = (int)(p->cd.fs * attack * channels);   // af_alimiter config_input
    bs -= bs % channels;
    if (bs <= 0) return fail(AMX_EINVAL, "Attack is too small.");
    if (buffer_size) *buffer_size = bs;
    if (halo_frames) *halo_frames = bs / channels - 1;
    if (state_doubles) *state_doubles = 8 + 3 * (int64_t)bs;
    return AMX_OK;
}

int amx_limiter_prepare(amx_plan *p, const amx_final_desc *fd, int32_t seg_frames,
                        int32_t warm_frames) {
    if (!p || !fd) return fail(AMX_EINVAL, "null argument");
    int32_t bs = 0, halo = 0;
    int64_t sd = 0;
    int rc = amx_limiter_geometry(p, fd, &bs, &halo, &sd);
    if (rc) return rc;
    if (seg_frames <= 0) seg_frames = p->lim.seg_frames > 0 ? p->lim.seg_frames : AMX_LIM_SEG_DEFAULT;
    if (seg_frames < 64 || seg_frames < bs / 2)
        return fail(AMX_EINVAL, "limiter segments of %d frames: need >= 64 and >= the ring (%d frames)",
                    seg_frames, bs / 2);
    if (amx::limiter_lds_bytes(bs) > AMX_LIM_LDS_MAX)
        return fail(AMX_ERANGE, "Attack is too large: the alimiter's %d-sample look-ahead ring does not fit "
                    "a CU's LDS (inputs above ~670 kHz)", bs);
    if (amx::limiter_lds_bytes(bs) > 64 * 1024) HIPCHK(amx::limiter_allow_lds(amx::limiter_lds_bytes(bs)));
    const int64_t max_segs64 = p->max_span > 0 ? (p->max_span + seg_frames - 1) / seg_frames : 1;
    if (max_segs64 > INT32_MAX / 2) return fail(AMX_EINVAL, "limiter: too many segments");
    const int max_segs = (int)max_segs64;
    if (warm_frames < 0) {
        // three releases plus the ring: a limiter that rested anywhere in the
        // warm-up has forgotten everything before it
        const double rel = p->cd.fs * (fd->release_ms / 1000.0);
        warm_frames = (int)std::min(1e9, std::ceil(3.0 * rel)) + bs / 2;
    }
    p->lim.warm_frames = warm_frames;
    // warm-ups reach back over active stretches up to 10 s (longer ones are left to
    // the in-order repair); warm_frames 0 disables the search (tests)
    p->lim.warm_cap = warm_frames > 0 ? (int64_t)p->cd.fs * 10 : 0;
    if (p->lim.seg_state && p->lim.buffer_size == bs && p->lim.seg_frames == seg_frames &&
        p->lim.max_segs == max_segs)
        return AMX_OK;
    const int T = p->n_tracks > 0 ? p->n_tracks : 1;
    // the new scratch is allocated before the old is released, so a failed
    // allocation leaves the plan's previous (consistent) limiter scratch in place
    double *seg_state = nullptr;
    unsigned *cnt = nullptr;
    if (hipMalloc(&seg_state, (size_t)T * max_segs * 2 * sd * sizeof(double)) != hipSuccess ||
        hipMalloc(&cnt, (size_t)T * sizeof(unsigned)) != hipSuccess ||
        hipMemset(cnt, 0, (size_t)T * sizeof(unsigned)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        if (seg_state) (void)hipFree(seg_state);
        if (cnt) (void)hipFree(cnt);
        return fail(AMX_EHIP, "limiter scratch allocation failed");
    }
    replace(p, p->lim.seg_state, seg_state);
    replace(p, p->lim.cnt, cnt);
    const int64_t cap = p->lim.warm_cap;
    p->lim = amx::LimScratch{};
    p->lim.warm_frames = warm_frames;
    p->lim.warm_cap = cap;
    p->lim.seg_state = seg_state;
    p->lim.cnt = cnt;
    p->lim.seg_frames = seg_frames;
    p->lim.max_segs = max_segs;
    p->lim.buffer_size = bs;
    return AMX_OK;
}

int amx_publish_ctl(const int32_t *d_ctl, int32_t *h_ctl, int32_t n, void *stream) {
    if (n < 0 || (n > 0 && (!d_ctl || !h_ctl))) return fail(AMX_EINVAL, "null argument");
    HIPCHK(amx::launch_publish(d_ctl, h_ctl, n, (hipStream_t)stream));
    return AMX_OK;
}

int amx_loudness_decide(amx_plan *p, const amx_decide_desc *dd, const amx_final_desc *fd,
                        const uint64_t *d_hist, const uint64_t *d_st_hist, const double *d_peak,
                        double *d_stats, double *d_gains, int32_t *d_ctl, void *stream) {
    if (!p || !dd || !fd || !d_peak || !d_stats || !d_gains || !d_ctl ||
        (dd->lufs_on && (!d_hist || !d_st_hist)))
        return fail(AMX_EINVAL, "null argument");
    if (dd->lufs_on && p->meas_native)
        return fail(AMX_ERANGE, "%d Hz: loudnorm measures the track resampled to 192 kHz with an "
                    "interpolating downsampler (not restated); lufs=None works", p->cd.fs);
    amx::DecideArgs a{};
    a.n_tracks = p->n_tracks;
    a.lufs_on = dd->lufs_on ? 1 : 0;
    a.hist = reinterpret_cast<const unsigned long long *>(d_hist);
    a.st_hist = reinterpret_cast<const unsigned long long *>(d_st_hist);
    a.peak = d_peak;
    a.energies = p->d_energies;
    a.bounds = p->d_bounds;
    a.target_i = dd->target_i;
    a.target_tp = dd->target_tp;
    a.target_lra = dd->target_lra;
    a.level_in = fd->level_in;
    a.limit = fd->limit;
    a.stats = d_stats;
    a.gains = d_gains;
    a.ctl = d_ctl;
    a.host_ctl = p->publish;
    HIPCHK(amx::launch_decide(a, (hipStream_t)stream));
    return AMX_OK;
}

int amx_kw_carry_setup(amx_plan *p, int32_t n_prev, const int64_t *frames_after) {
    if (!p || n_prev < 0 || (n_prev > 0 && !frames_after)) return fail(AMX_EINVAL, "bad argument");
    std::vector<double> P((size_t)(n_prev > 0 ? n_prev : 1) * 16, 0.0);
    for (int q = 0; q < n_prev; q++) {
        if (frames_after[q] < 0) return fail(AMX_EINVAL, "frames_after[%d] < 0", q);
        // the gap on the measurement stream: J(f0) - J(f0 - frames_after), J(f) = ceil(f L / M)
        int64_t gap = frames_after[q];
        if (p->resamp && p->n_tracks > 0) {
            const int64_t f0 = p->spans[0].tframe0, L = p->upL, M = p->upM;
            auto J = [&](int64_t f) { return (f * L + M - 1) / M; };
            gap = J(f0) - J(f0 - frames_after[q]);
        }
        Mat m = p->kw_model.pow(gap);
        for (int k = 0; k < 16; k++) P[(size_t)q * 16 + k] = m[k];
    }
    replace(p, p->d_carryP, (double *)nullptr);
    int rc = upload(p, &p->d_carryP, P);
    if (rc) return rc;
    p->n_prev = n_prev;
    return AMX_OK;
}

int amx_kw_carry(amx_plan *p, const double *d_tails, double *d_carry, void *stream) {
    if (!p || !d_carry || (p->n_prev > 0 && !d_tails)) return fail(AMX_EINVAL, "null argument");
    if (!p->d_carryP) return fail(AMX_EINVAL, "amx_kw_carry: call amx_kw_carry_setup first");
    HIPCHK(amx::launch_kw_carry(d_tails, p->d_carryP, p->n_prev, d_carry, (hipStream_t)stream));
    return AMX_OK;
}

int amx_kw_carry_rows(amx_plan *p, const double *d_rows, int32_t world, int32_t ld, double *d_carry,
                      double *d_peak, void *stream) {
    if (!p || !d_rows || !d_carry || !d_peak) return fail(AMX_EINVAL, "null argument");
    if (!p->d_carryP) return fail(AMX_EINVAL, "amx_kw_carry_rows: call amx_kw_carry_setup first");
    if (world < 1 || ld < 12 || p->n_prev >= world)
        return fail(AMX_EINVAL, "amx_kw_carry_rows: %d rows of %d doubles for %d previous spans", world, ld,
                    p->n_prev);
    HIPCHK(amx::launch_kw_carry_rows(d_rows, world, ld, p->d_carryP, p->n_prev, d_carry, d_peak,
                                     (hipStream_t)stream));
    return AMX_OK;
}

int amx_finalize(amx_plan *p, const amx_final_desc *fd, const int16_t *d_x,
                 const double *d_gains, const int32_t *d_ctl, int32_t fast,
                 const int16_t *d_halo, int16_t *d_y, double *d_lim_state, void *d_ws,
                 void *stream) {
    (void)d_ws;
    if (!p || !fd || !d_gains || (p->out_frames > 0 && (!d_x || !d_y)))
        return fail(AMX_EINVAL, "null argument");
    if (p->out_frames == 0) return AMX_OK;
    int32_t bs = 0, halo = 0;
    int64_t sd = 0;
    int rc = amx_limiter_geometry(p, fd, &bs, &halo, &sd);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const double level = fd->auto_level ? 1 / fd->limit : 1;
    if ((d_ctl || !fast) && !d_lim_state) return fail(AMX_EINVAL, "general limiter needs d_lim_state");
    if ((d_ctl || !fast) && (!p->lim.seg_state || p->lim.buffer_size != bs)) {
        // amx_limiter_prepare allocates: not while the stream is being captured into a
        // graph (callers that capture call it first)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIPCHK(hipStreamIsCapturing(st, &cs));
        if (cs != hipStreamCaptureStatusNone)
            return fail(AMX_EINVAL, "amx_finalize: call amx_limiter_prepare before capturing the stream");
        rc = amx_limiter_prepare(p, fd, 0, -1);
        if (rc) return rc;
    }
    p->lim.gate = p->gate;
    p->lim.att = p->lim_att;
    p->lim.slope_channels = p->lim_channels;
    HIPCHK(amx::launch_final(p->d_spans, p->n_tracks, p->max_span, d_x, d_halo, halo, d_gains, d_ctl,
                             fast ? 1 : 0, p->cd.fs, fd->level_in, level, fd->level_out, fd->limit,
                             fd->release_ms / 1000.0, bs, d_lim_state, sd, fd->from_rest, p->lim, d_y, st));
    return AMX_OK;
}

}  // extern "C"

// ==================================================================================
// More than two channels (round 6).  audio_segment_to_float_array only reshapes a
// stereo chunk (:252), so a 3..8-channel chunk goes through the chain as ONE
// interleaved 1-D stream: analog character (its shelves along the stream, :264-265),
// EQ (:274, float64 result), no width (:268), the crossover along the stream (:303);
// pydub's compressor and overlay then work on frames of C samples (:306-309).
//   pa (analog on): a stream chain (stream in L of int16 pairs) whose "EQ" is the
//      analog character's two shelves, the input through the float32 tanh table;
//   pb: the stream chain of the EQ (and the crossover bands when multiband);
//   pc (multiband): a stereo plan over the chunks' real frames whose envelope kernels
//      (k_env0 + fix-up) run on the C-sample r that k_mc_rms forms from pb's bands;
//      k_mc_gain_overlay writes the C-channel output.
extern "C" {

void amx_mc_plan_free(amx_mc_plan *m) {
    if (!m) return;
    amx_plan_free(m->pa);
    amx_plan_free(m->pb);
    amx_plan_free(m->pc);
    delete m;
}

int amx_mc_plan_create(const amx_chain_desc *desc, const amx_chunk *chunks, int32_t n_chunks, int32_t seg_frames,
                       amx_mc_plan **out) {
    if (!desc || !out || n_chunks < 0 || (n_chunks > 0 && !chunks)) return fail(AMX_EINVAL, "null argument");
    *out = nullptr;
    const int C = desc->channels_in;
    if (C < 3 || C > 8) return fail(AMX_EINVAL, "amx_mc_plan_create: %d channels (3..8; 1 or 2: amx_plan_create)", C);
    if (desc->analog_on && !desc->tanh_lut)
        return fail(AMX_EINVAL, "analog character needs the float32 tanh table (tanh_lut)");
    std::unique_ptr<amx_mc_plan, PlanFree> m(new (std::nothrow) amx_mc_plan());
    if (!m) return fail(AMX_ENOMEM, "out of memory");
    m->C = C;
    m->mb = desc->multiband_on ? 1 : 0;
    m->in_s16 = desc->input_s16 ? 1 : 0;
    std::vector<amx_chunk> sch((size_t)n_chunks), ach((size_t)n_chunks);
    int64_t in_end = 0, acc = 0, sum_n = 0;
    for (int32_t k = 0; k < n_chunks; k++) {
        if (chunks[k].frames < 0 || chunks[k].in_offset < 0)
            return fail(AMX_EINVAL, "chunk %d: negative offset or length", k);
        sch[k] = chunks[k];
        sch[k].in_offset = chunks[k].in_offset * C;
        sch[k].frames = chunks[k].frames * C;
        ach[k] = sch[k];
        ach[k].in_offset = acc;                       // pb reads pa's output, chunks back to back
        acc += sch[k].frames;
        in_end = std::max(in_end, chunks[k].in_offset + chunks[k].frames);
        sum_n += chunks[k].frames;
    }
    m->M = in_end * C;
    // the stream chains: int16 pairs, the stream in L
    const amx_chain_desc ds = mc_sub_desc(*desc, 1);
    int rc = AMX_OK;
    if (desc->analog_on) {
        // x = tanh(float32 s / 32768 * drive) (the table), then low shelf 120 Hz with g =
        // 10^(cf/20) and high shelf 12 kHz with 10^(1.5 cf/20), both gains > 0: the EQ's
        // positive-gain shelf form x + (y - x)(g - 1) at stages 0 and 3 (:264-265, :288)
        amx_chain_desc da = ds;
        da.multiband_on = 0;
        for (int s = 0; s < 4; s++) { da.eq_kind[s] = 0; da.eq_gain_db[s] = 0.0; da.eq_gain[s] = 1.0; }
        da.eq_kind[0] = 1;
        da.eq_gain[0] = desc->analog_lo_gain;
        da.eq_gain_db[0] = 20.0 * std::log10(desc->analog_lo_gain);
        da.eq_kind[3] = 1;
        da.eq_gain[3] = desc->analog_hi_gain;
        da.eq_gain_db[3] = 20.0 * std::log10(desc->analog_hi_gain);
        for (int k = 0; k < 6; k++) {
            da.eq_coef[0][k] = desc->analog_lo_ba[k];
            da.eq_coef[3][k] = desc->analog_hi_ba[k];
        }
        if (!(da.eq_gain_db[0] > 0.0 && da.eq_gain_db[3] > 0.0))
            return fail(AMX_EINVAL, "analog character gains must be > 1");
        da.eq_in_lut = desc->tanh_lut;
        rc = amx_plan_create(&da, sch.data(), n_chunks, nullptr, nullptr, seg_frames, &m->pa);
        if (rc) return rc;
    }
    rc = amx_plan_create(&ds, desc->analog_on ? ach.data() : sch.data(), n_chunks, nullptr, nullptr, seg_frames,
                         &m->pb);
    if (rc) return rc;
    if (m->mb) {
        amx_chain_desc dc = mc_sub_desc(*desc, 0);
        for (int s = 0; s < 4; s++) { dc.eq_kind[s] = 0; dc.eq_gain_db[s] = 0.0; dc.eq_gain[s] = 1.0; }
        rc = amx_plan_create(&dc, chunks, n_chunks, nullptr, nullptr, seg_frames, &m->pc);
        if (rc) return rc;
        m->out_frames = m->pc->out_frames;
    } else {
        m->out_frames = sum_n;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    m->o_pack = take((size_t)std::max<int64_t>(m->M, 1) * 4);
    if (m->pa) m->o_outa = take((size_t)std::max<int64_t>(m->pa->out_frames, 1) * 4);
    if (!m->mb) m->o_outb = take((size_t)std::max<int64_t>(m->pb->out_frames, 1) * 4);
    if (m->pa) m->o_wa = take(m->pa->ws_bytes);
    m->o_wb = take(m->pb->ws_bytes);
    if (m->pc) m->o_wc = take(m->pc->ws_bytes);
    m->ws_bytes = off;
    *out = m.release();
    return AMX_OK;
}

int amx_mc_plan_get_info(const amx_mc_plan *m, int64_t *workspace_bytes, int64_t *out_frames) {
    if (!m || !workspace_bytes || !out_frames) return fail(AMX_EINVAL, "null argument");
    *workspace_bytes = (int64_t)m->ws_bytes;
    *out_frames = m->out_frames;
    return AMX_OK;
}

int amx_mc_run_chunks(amx_mc_plan *m, const void *d_in, int16_t *d_out, void *d_ws, void *stream) {
    if (!m || (m->M > 0 && (!d_in || !d_out || !d_ws))) return fail(AMX_EINVAL, "null argument");
    if (m->M == 0) return AMX_OK;
    hipStream_t st = (hipStream_t)stream;
    char *w = reinterpret_cast<char *>(d_ws);
    uint32_t *pack = reinterpret_cast<uint32_t *>(w + m->o_pack);
    HIPCHK(amx::launch_mc_pack(d_in, m->M, m->in_s16, pack, st));
    const float *src = reinterpret_cast<const float *>(pack);
    if (m->pa) {
        int16_t *outa = reinterpret_cast<int16_t *>(w + m->o_outa);
        int rc = amx_run_chunks(m->pa, src, outa, w + m->o_wa, stream);
        if (rc) return rc;
        src = reinterpret_cast<const float *>(outa);
    }
    amx_plan *pb = m->pb;
    void *wb = w + m->o_wb;
    if (!m->mb) {
        int16_t *outb = reinterpret_cast<int16_t *>(w + m->o_outb);
        int rc = amx_run_chunks(pb, src, outb, wb, stream);
        if (rc) return rc;
        HIPCHK(amx::launch_mc_unpack(reinterpret_cast<const uint32_t *>(outb), m->out_frames * m->C, d_out, st));
        return AMX_OK;
    }
    // the stream's EQ and crossover bands (pb), then the compressor on C-sample frames
    for (int s = AMX_STAGE_FRONT1; s <= AMX_STAGE_XOVER; s++) {
        int rc = amx_run_stage(pb, s, src, d_out, wb, stream);
        if (rc) return rc;
    }
    amx_plan *pc = m->pc;
    void *wc = w + m->o_wc;
    amx::DynLaunch dl{pc->d_cd,    pc->d_chunks, pc->n_chunks, pc->d_esegs, pc->n_es,
                      pc->d_eseg0, pc->d_neseg,  pc->nloc,     pc->max_chunk_n, pc->cd.look,
                      pc->warm,    pc->Le,       pc->cd.env_rcp, pc->d_tabs, st,
                      pc->env_wg};
    const int16_t *bands = wsp<int16_t>(wb, pb->o_bands);
    uint16_t *mframe = wsp<uint16_t>(wc, pc->o_m);
    int *bact = wsp<int>(wc, pc->o_eflags) + AMX_ENV_BACT;
    HIPCHK(amx::launch_mc_rms(dl, pb->d_chunks, bands, pb->nloc, m->C, mframe, bact));
    for (int s : {AMX_STAGE_ENV, AMX_STAGE_FIX}) {
        int rc = amx_run_stage(pc, s, reinterpret_cast<const float *>(d_in), d_out, wc, stream);
        if (rc) return rc;
    }
    HIPCHK(amx::launch_mc_gain_overlay(dl, pb->d_chunks, mframe, wsp<double>(wc, pc->o_gain), bands, pb->nloc,
                                       m->C, pc->max_chunk_out, pc->d_n1, bact, d_out));
    return AMX_OK;
}

int amx_mc_split_pairs(const int16_t *d_y, int64_t frames, int32_t channels, int16_t *d_pairs, void *stream) {
    if (frames > 0 && (!d_y || !d_pairs)) return fail(AMX_EINVAL, "null argument");
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "%d channels", channels);
    HIPCHK(amx::launch_mc_split_pairs(d_y, frames, channels, d_pairs, (hipStream_t)stream));
    return AMX_OK;
}

int amx_mc_loudness_combine(const double *d_hops, int64_t max_hops, const double *d_peak, int32_t channels,
                            double *d_hops1, double *d_peak1, void *stream) {
    if (!d_hops || !d_peak || !d_hops1 || !d_peak1 || max_hops <= 0) return fail(AMX_EINVAL, "null argument");
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "%d channels", channels);
    HIPCHK(amx::launch_mc_loudness_combine(d_hops, max_hops, d_peak, channels, d_hops1, d_peak1,
                                           (hipStream_t)stream));
    return AMX_OK;
}

int amx_mc_peak_pick(const int16_t *d_y, int64_t frames, int32_t channels, const double *d_gain, int16_t *d_syn,
                     void *stream) {
    if (frames > 0 && (!d_y || !d_gain || !d_syn)) return fail(AMX_EINVAL, "null argument");
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "%d channels", channels);
    HIPCHK(amx::launch_mc_peak_pick(d_y, frames, channels, d_gain, d_syn, (hipStream_t)stream));
    return AMX_OK;
}

int amx_mc_limiter_out(const amx_plan *p, const amx_final_desc *fd, const int16_t *d_y, int32_t channels,
                       const double *d_gains, const int32_t *d_ctl, const double *d_att, int16_t *d_out,
                       void *stream) {
    if (!p || !fd || !d_gains || !d_ctl || (p->out_frames > 0 && (!d_y || !d_att || !d_out)))
        return fail(AMX_EINVAL, "null argument");
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "%d channels", channels);
    if (p->n_tracks != 1 || p->spans[0].tframe0 != 0) return fail(AMX_EINVAL, "one whole track per plan");
    int32_t bs = 0, halo = 0;
    int64_t sd = 0;
    if (int rc = amx_limiter_geometry(p, fd, &bs, &halo, &sd)) return rc;
    const double level = fd->auto_level ? 1 / fd->limit : 1;
    HIPCHK(amx::launch_mc_limiter_out(d_y, p->out_frames, channels, halo, d_gains, d_ctl, d_att, fd->level_in,
                                      level, fd->level_out, fd->limit, d_out, (hipStream_t)stream));
    return AMX_OK;
}

}  // extern "C"

namespace {
// amx_mc_loudnorm_192k's plan: ceil(C / 2) equal whole tracks (the channel pairs); *n192
// the 192 kHz frames of each (AMX_ERANGE as ln_frames)
int ln_mc_frames(const amx_plan *p, int32_t channels, int64_t *n192) {
    if (channels < 3 || channels > 8) return fail(AMX_EINVAL, "%d channels (3..8; 1 or 2: amx_loudnorm_192k)", channels);
    const int P = (channels + 1) / 2;
    if (p->n_tracks != P) return fail(AMX_EINVAL, "the pairs' plan holds %d tracks, %d channels need %d", p->n_tracks, channels, P);
    for (int t = 0; t < P; t++) {
        const SpanDev &sp = p->spans[t];
        if (sp.tframe0 != 0 || sp.ttotal != sp.out_n || sp.out_n != p->spans[0].out_n)
            return fail(AMX_EINVAL, "the pairs' plan holds one whole track of the same length per channel pair");
    }
    return ln_frames(p, 0, n192);
}
int64_t ln_mc_plane_bytes(int64_t n192) { return ((n192 * 2 * (int64_t)sizeof(float) + 255) / 256) * 256; }
}  // namespace

extern "C" {

int amx_mc_loudnorm_192k_size(const amx_plan *p, int32_t channels, int64_t *frames, int64_t *ws_bytes) {
    if (!p || !frames || !ws_bytes) return fail(AMX_EINVAL, "null argument");
    int64_t n192 = 0;
    if (int rc = ln_mc_frames(p, channels, &n192)) return rc;
    *frames = n192;
    *ws_bytes = ((channels + 1) / 2) * ln_mc_plane_bytes(n192) + AMX_LN_MC_RING(channels) * (int64_t)sizeof(double);
    return AMX_OK;
}

int amx_mc_loudnorm_192k(amx_plan *p, int32_t channels, const amx_loudnorm_desc *d, const int16_t *d_pairs,
                         const double *d_hops1, int64_t max_hops, const double *d_peak1, int16_t *d_y192,
                         double *d_summary, void *d_ws, void *stream) {
    if (!p || !d || !d_pairs || !d_hops1 || !d_peak1 || !d_y192 || !d_summary || !d_ws)
        return fail(AMX_EINVAL, "null argument");
    int64_t n192 = 0;
    if (int rc = ln_mc_frames(p, channels, &n192)) return rc;
    if (max_hops < n192 / 19200 + 1) return fail(AMX_EINVAL, "d_hops1 holds %lld hops", (long long)max_hops);
    if (n192 <= 0) return AMX_OK;
    const int P = (channels + 1) / 2;
    const int64_t plane = ln_mc_plane_bytes(n192);
    char *w = reinterpret_cast<char *>(d_ws);
    amx::LnArgs a{};
    a.n192 = n192;
    a.u = reinterpret_cast<float *>(w);
    a.plane = plane / (int64_t)sizeof(float);
    a.ring = reinterpret_cast<double *>(w + (int64_t)P * plane);
    a.y = d_y192;
    a.summary = d_summary;
    a.hops = d_hops1;
    a.peak = d_peak1;
    ln_options(p, d, a);
    hipStream_t st = (hipStream_t)stream;
    if (d->reuse_stream == 0) {
        // each channel pair through the stereo upsampler into its plane
        const amx::SwrDev r = swr_dev(p);
        for (int t = 0; t < P; t++) {
            const SpanDev &sp = p->spans[t];
            HIPCHK(amx::launch_ln_upsample(reinterpret_cast<const uint32_t *>(d_pairs) + sp.out_off, sp.out_n, r, 0,
                                           n192, reinterpret_cast<float *>(w + (int64_t)t * plane), nullptr, st));
        }
    }
    HIPCHK(amx::launch_ln_dyn(a, channels, 0, st));
    return AMX_OK;
}

}  // extern "C"

// ==================================================================================
// The output resampler (amx_resample.hip): the finished master at the
// rate the caller asks for.  Replaces no reference line (the reference writes the master
// at the rate the last filter leaves it, :223); it is the `-ar R` of a loudnorm recipe.
struct amx_resampler {
    int32_t in_rate = 0, out_rate = 0, channels = 0;
    int32_t L = 1, M = 1, taps = 0, alloc = 0, phases = 0;
    int32_t ncu = 1;           // the device's CUs (the persistent form's grid)
    float *d_bank = nullptr;
};

namespace {
// the pair's geometry, or the error: phases = L (no output interpolates)
int resample_geometry(int32_t in_rate, int32_t out_rate, int *L, int *M, int *taps, int *alloc) {
    if (in_rate <= 0 || out_rate <= 0) return fail(AMX_EINVAL, "rates must be positive (%d -> %d)", in_rate, out_rate);
    if (in_rate == out_rate) return fail(AMX_EINVAL, "equal rates (%d): nothing to resample", in_rate);
    amx::swr_geometry(in_rate, out_rate, L, M);
    if (*L > 1024 || amx::swr_phases(in_rate, out_rate, AMX_RS_MAX_ALLOC) < 0 ||
        amx::swr_filter(in_rate, out_rate, taps, alloc, nullptr, AMX_RS_MAX_ALLOC))
        return fail(AMX_ERANGE, "%d -> %d Hz is outside the resampler's pairs (%d phases; at most 1024, filter rows "
                    "of at most %d taps)", in_rate, out_rate, *L, AMX_RS_MAX_ALLOC);
    return AMX_OK;
}
}  // namespace

extern "C" {

int amx_resample_size(int32_t in_rate, int32_t out_rate, int64_t frames, int64_t *out_frames, int32_t *taps,
                      int32_t *alloc, int32_t *phases) {
    if (frames < 0) return fail(AMX_EINVAL, "frames must be >= 0");
    int L = 1, M = 1, t = 0, al = 0;
    if (int rc = resample_geometry(in_rate, out_rate, &L, &M, &t, &al)) return rc;
    if (frames > (INT64_MAX - M) / L) return fail(AMX_ERANGE, "%lld frames", (long long)frames);
    if (out_frames) *out_frames = (frames * L + M - 1) / M;
    if (taps) *taps = t;
    if (alloc) *alloc = al;
    if (phases) *phases = L;
    return AMX_OK;
}

void amx_resampler_free(amx_resampler *h) {
    if (!h) return;
    if (h->d_bank) (void)hipFree(h->d_bank);
    delete h;
}

int amx_resampler_create(int32_t in_rate, int32_t out_rate, int32_t channels, amx_resampler **out) {
    if (!out) return fail(AMX_EINVAL, "null argument");
    *out = nullptr;
    if (channels < 1 || channels > 8) return fail(AMX_EINVAL, "channels must be 1..8");
    std::unique_ptr<amx_resampler, void (*)(amx_resampler *)> h(new (std::nothrow) amx_resampler, amx_resampler_free);
    if (!h) return fail(AMX_ENOMEM, "out of host memory");
    int L = 1, M = 1, t = 0, al = 0;
    if (int rc = resample_geometry(in_rate, out_rate, &L, &M, &t, &al)) return rc;
    h->in_rate = in_rate;
    h->out_rate = out_rate;
    h->channels = channels;
    h->L = L;
    h->M = M;
    h->taps = t;
    h->alloc = al;
    h->phases = L;
    std::vector<float> bank((size_t)L * al), dev;
    if (amx::swr_bank(in_rate, out_rate, bank.data(), AMX_RS_MAX_ALLOC)) return fail(AMX_ERANGE, "no filter bank");
    if (L == 1) {
        dev = bank;
    } else {
        // tap-major: the lanes of a wave read one tap of their own rows
        dev.resize(bank.size());
        for (int ph = 0; ph < L; ph++)
            for (int i = 0; i < al; i++) dev[(size_t)i * L + ph] = bank[(size_t)ph * al + i];
    }
    int device = 0, ncu = 0;
    HIPCHK(hipGetDevice(&device));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    h->ncu = ncu > 0 ? ncu : 1;
    HIPCHK(amx::resample_prepare(L, M, al, channels));
    HIPCHK(hipMalloc((void **)&h->d_bank, dev.size() * sizeof(float)));
    HIPCHK(hipMemcpy(h->d_bank, dev.data(), dev.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = h.release();
    return AMX_OK;
}

int amx_resampler_run(const amx_resampler *h, const int16_t *d_in, int64_t frames, int16_t *d_out,
                      int64_t out_capacity_frames, void *stream) {
    if (!h) return fail(AMX_EINVAL, "null resampler");
    if (frames < 0) return fail(AMX_EINVAL, "frames must be >= 0");
    if (frames == 0) return AMX_OK;
    if (!d_in || !d_out) return fail(AMX_EINVAL, "null argument");
    if (frames > (INT64_MAX - h->M) / h->L) return fail(AMX_EINVAL, "%lld frames", (long long)frames);
    const int64_t n_out = (frames * h->L + h->M - 1) / h->M;
    if (out_capacity_frames < n_out)
        return fail(AMX_EINVAL, "out_capacity_frames %lld < %lld (amx_resample_size)", (long long)out_capacity_frames,
                    (long long)n_out);
    if ((n_out + AMX_RS_TILE - 1) / AMX_RS_TILE > INT32_MAX) return fail(AMX_EINVAL, "%lld frames", (long long)frames);
    HIPCHK(amx::launch_resample(h->L, h->M, h->alloc, (h->taps - 1) / 2, h->channels, h->d_bank, h->ncu, d_in, frames,
                                d_out, n_out, (hipStream_t)stream));
    return AMX_OK;
}

}  // extern "C"
