// plan_harness.cpp -- plan construction on the CPU (tests/test_plan_build.py).
//
// Links csrc/amx_plan.cpp + csrc/amx_plan_build.cpp against hip_standin.cpp and runs
// amx_plan_create / amx_mc_plan_create over a list of cases.  Per case it prints the
// return code and error text, amx_plan_info, the track spans, the workspace offsets, a
// digest of every integer table the plan uploaded, size and finiteness of the floating
// ones, and (--full) the multiset of (bytes, FNV-1a) of all uploads; it checks the
// tables' invariants on the "device" copies and the ownership rules (allocation
// failures, the re-allocating entry points).  No kernel is launched.
#include "../../include/amx.h"
#include "amx_plan.hpp"
#include "hip_standin.hpp"

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace ph {

const char *const KNOBS[] = {"AMX_UP_POLY", "AMX_F1"};

struct Case {
    std::string name;
    amx_chain_desc d;
    std::vector<amx_chunk> ch;
    std::vector<int64_t> f0, tot;   // empty: NULL
    int seg = 0, ncu = 256;
    std::vector<std::pair<const char *, const char *>> env;
    bool null_desc = false, null_out = false, null_chunks = false, mc = false;
    int n_chunks = INT_MIN;         // INT_MIN: ch.size()
};

// a stable biquad row b0 b1 b2 a0 a1 a2, poles at radius 0.95 (r^2 = 0.9025)
void sos(double *c, int q) {
    const double v[6] = {0.05 + 0.01 * q, 0.1, 0.05, 1.0, -1.8 + 0.05 * q, 0.9025};
    for (int k = 0; k < 6; k++) c[k] = v[k];
}
// the same with a pole pair at radius 1 - 5e-10: decays too slowly for any scan window
void sos_slow(double *c) {
    sos(c, 0);
    c[4] = -1.9;
    c[5] = 0.999999999;
}

std::vector<float> tanh_like() {   // an odd float32 table (no libm): x / (1 + |x|)
    std::vector<float> t(65536);
    for (int k = 0; k <= 32768; k++) {
        const float x = (float)k / 32768.0f * 1.5f, y = x / (1.0f + x);
        if (k < 32768) t[32768 + k] = y;
        if (k > 0) t[32768 - k] = -y;
    }
    return t;
}
const std::vector<float> g_lut = tanh_like();
std::vector<float> g_lut_broken = [] { auto t = tanh_like(); t[32768 - 77] = 0.25f; return t; }();

amx_chain_desc desc(int fs, int mb = 0) {
    amx_chain_desc d{};
    d.sample_rate = fs;
    d.channels_in = 2;
    d.input_s16 = 1;
    d.analog_drive = 1.2f;
    sos(d.analog_lo_ba, 1);
    sos(d.analog_hi_ba, 2);
    d.analog_lo_gain = 1.5;
    d.analog_hi_gain = 1.75;
    for (int s = 0; s < 4; s++) d.eq_gain[s] = 1.0;
    d.width = 1.3f;
    d.multiband_on = mb;
    for (int q = 0; q < 2; q++) {
        sos(d.xover_lo_sos + 6 * q, q);
        sos(d.xover_hi_sos + 6 * q, q + 2);
    }
    const double thr[3] = {-25.0, -20.0, -15.0}, ratio[3] = {6.0, 3.0, 4.0};
    for (int b = 0; b < 3; b++) {
        d.comp_threshold_db[b] = thr[b];
        d.comp_ratio[b] = ratio[b];
    }
    d.env_warm_frames = -1;
    d.env_rounds = -1;
    return d;
}
// EQ stage s with a gain of +2 dB or -1.5 dB
void eq(amx_chain_desc &d, int s, bool neg = false) {
    d.eq_kind[s] = (s == 0 || s == 3) ? 1 : 2;
    d.eq_gain_db[s] = neg ? -1.5 : 2.0;
    d.eq_gain[s] = neg ? 0.8413951416451951 : 1.2589254117941673;
    for (int q = 0; q < (d.eq_kind[s] == 1 ? 1 : 4); q++) sos(d.eq_coef[s] + 6 * q, (s + q) % 4);
}
amx_chain_desc desc_eq(int fs, int mb = 0) {
    amx_chain_desc d = desc(fs, mb);
    for (int s = 0; s < 4; s++) eq(d, s);
    return d;
}
amx_chain_desc desc_f32(int fs, int mb, const std::vector<float> &lut) {
    amx_chain_desc d = desc_eq(fs, mb);
    d.input_s16 = 0;
    d.analog_on = 1;
    d.width_on = 1;
    d.tanh_lut = lut.data();
    return d;
}
std::vector<amx_chunk> chunks(std::initializer_list<std::array<int64_t, 3>> l) {
    std::vector<amx_chunk> v;
    for (const auto &c : l) {
        amx_chunk k{};
        k.track = (int32_t)c[0];
        k.in_offset = c[1];
        k.frames = c[2];
        v.push_back(k);
    }
    return v;
}
const std::vector<amx_chunk> TWO = chunks({{0, 0, 3000}, {0, 3000, 2501}});

std::vector<Case> cases() {
    std::vector<Case> v;
    auto add = [&](std::string name, amx_chain_desc d, std::vector<amx_chunk> ch) -> Case & {
        Case c;
        c.name = std::move(name);
        c.d = d;
        c.ch = std::move(ch);
        v.push_back(c);
        return v.back();
    };
    // rates: the unrolled forms L = 4 / 2 / 1, the five k_up_poly forms and a rate without
    // one (24 kHz), the 1024-phase interpolating rates, a downsampling rate (> 32 taps), and
    // rates the resampler restatement refuses (the measurement at the track's own rate)
    const int rates[] = {48000, 96000, 192000, 44100, 88200, 176400, 32000, 64000, 24000, 22050, 11025, 384000,
                         200001, 352800};
    for (int fs : rates) add("rate_" + std::to_string(fs), desc_eq(fs), TWO);
    // (above 204.8 kHz the compressor's detector window passes k_rms's tile: AMX_ERANGE)
    for (int fs : {48000, 96000, 192000, 44100, 22050, 384000, 352800})
        add("mb_" + std::to_string(fs), desc_eq(fs, 1), TWO);
    // multiband on few CUs over ~200 k frames: Le grows past its floor, the Le_t tables differ
    const std::vector<amx_chunk> big = chunks({{0, 0, 100000}, {0, 100000, 70001}, {1, 170001, 30000}});
    add("mb_ncu4", desc_eq(44100, 1), big).ncu = 4;
    add("mb_ncu4_48k", desc(48000, 1), big).ncu = 4;
    add("mb_ncu_fallback", desc_eq(44100, 1), big).ncu = 2;       // < 3: the 256 fallback
    add("mb_ncu_error", desc_eq(44100, 1), big).ncu = -1;         // the query fails: 256
    {
        amx_chain_desc d = desc_eq(48000, 1);
        d.env_warm_frames = 1000;
        d.env_rounds = 5;
        add("mb_warm_rounds", d, TWO).seg = 100;
    }
    // EQ
    add("eq_none", desc(48000), TWO);
    {
        amx_chain_desc d = desc(48000);
        eq(d, 0, true);
        eq(d, 2);
        add("eq_neg_first", d, TWO);
        d = desc(48000);
        eq(d, 3, true);
        add("eq_neg_first_stage3", d, TWO);
        d = desc(48000);
        eq(d, 1);
        eq(d, 3, true);
        add("eq_neg_later", d, TWO);
    }
    // inputs
    {
        amx_chain_desc d = desc_eq(48000);
        d.channels_in = 1;
        add("in_mono16", d, TWO);
        add("in_f32_analog", desc_f32(48000, 0, g_lut), TWO);
        add("in_f32_analog_mb", desc_f32(44100, 1, g_lut), TWO);
        add("in_f32_broken_table", desc_f32(48000, 0, g_lut_broken), TWO);
        add("in_f32_AMX_F1=2", desc_f32(48000, 0, g_lut), TWO).env.push_back({"AMX_F1", "2"});
        add("in_f32_AMX_F1=1", desc_f32(48000, 0, g_lut), TWO).env.push_back({"AMX_F1", "1"});
        d = desc_eq(48000);
        d.tanh_lut = g_lut.data();                 // a table without the analog stage
        add("in_s16_lut_only", d, TWO);
        d = desc_eq(48000, 1);
        d.stream_chain = 1;
        d.eq_in_lut = g_lut.data();
        add("in_stream_chain", d, TWO);
        d.measure_only = 1;
        d.stream_chain = 0;
        d.eq_in_lut = nullptr;
        add("in_measure_only", d, TWO);
    }
    // chunks
    add("ch_none", desc_eq(48000, 1), {});
    add("ch_zero_len", desc_eq(48000, 1), chunks({{0, 0, 3000}, {0, 3000, 0}, {1, 3000, 700}}));
    add("ch_one_frame", desc_eq(44100, 1), chunks({{0, 0, 1}}));
    add("ch_L-1_L_L+1", desc_eq(48000), chunks({{0, 0, 255}, {0, 255, 256}, {0, 511, 257}}));
    add("ch_whole_segments", desc_eq(192000), chunks({{0, 0, 1024}, {0, 1024, 999}, {1, 2023, 512}}));
    add("ch_odd_offset", desc_f32(48000, 0, g_lut), chunks({{0, 0, 3001}, {0, 3001, 2000}}));
    add("ch_short", desc_f32(48000, 0, g_lut), chunks({{0, 0, 3}, {0, 4, 2000}}));
    add("ch_empty_track", desc_eq(44100, 1), chunks({{0, 0, 3000}, {2, 3000, 2501}}));
    {
        Case &c = add("ch_shards", desc_eq(48000, 1), chunks({{0, 0, 3000}, {0, 3000, 2000}, {1, 5000, 1600}}));
        c.f0 = {4800, 0};
        c.tot = {20000, 1600 + 320};
        Case &e = add("ch_shards_44k", desc_eq(44100), chunks({{0, 0, 3000}, {1, 3000, 2000}}));
        e.f0 = {147 * 16, 147 * 32};
        e.tot = {147 * 16 + 3000, 20000};
        Case &f = add("ch_shard_unaligned", desc_eq(200001), chunks({{0, 0, 3000}, {0, 3000, 500}}));
        f.f0 = {1001};
        f.tot = {9000};
        Case &g = add("ch_shard_unaligned_48k", desc_eq(48000), chunks({{0, 0, 3000}}));
        g.f0 = {1001};
        g.tot = {9000};
    }
    add("seg_100", desc_eq(96000, 1), TWO).seg = 100;
    // knobs
    add("AMX_UP_POLY=0", desc_eq(44100), TWO).env.push_back({"AMX_UP_POLY", "0"});
    add("AMX_UP_POLY=1", desc_eq(44100), TWO).env.push_back({"AMX_UP_POLY", "1"});
    // every fail exit
    add("err_null_desc", desc(48000), TWO).null_desc = true;
    add("err_null_out", desc(48000), TWO).null_out = true;
    add("err_null_chunks", desc(48000), TWO).null_chunks = true;
    add("err_neg_n_chunks", desc(48000), TWO).n_chunks = -1;
    add("err_rate_0", desc(0), TWO);
    add("err_channels_3", [] { auto d = desc(48000); d.channels_in = 3; return d; }(), TWO);
    add("err_analog_no_lut", [] { auto d = desc(48000); d.analog_on = 1; return d; }(), TWO);
    add("err_stream_analog", [] { auto d = desc_f32(48000, 0, g_lut); d.input_s16 = 1; d.stream_chain = 1; return d; }(), TWO);
    add("err_stream_f32", [] { auto d = desc(48000); d.input_s16 = 0; d.stream_chain = 1; return d; }(), TWO);
    add("err_eq_kind", [] { auto d = desc(48000); eq(d, 0); d.eq_kind[0] = 2; return d; }(), TWO);
    add("err_eq_kind_mid", [] { auto d = desc(48000); eq(d, 2); d.eq_kind[2] = 1; return d; }(), TWO);
    add("err_ratio_0", [] { auto d = desc(48000, 1); d.comp_ratio[1] = 0.0; return d; }(), TWO);
    add("err_neg_frames", desc(48000), chunks({{0, 0, 3000}, {0, 3000, -1}}));
    add("err_neg_offset", desc(48000), chunks({{0, -4, 3000}}));
    add("err_neg_track", desc(48000), chunks({{-1, 0, 3000}}));
    add("err_track_order", desc(48000), chunks({{1, 0, 3000}, {0, 3000, 100}}));
    add("err_2^31", desc(48000), chunks({{0, 0, (int64_t)1 << 30}, {0, 0, (int64_t)1 << 30}})).seg = 1 << 20;
    {
        Case &c = add("err_phase_patterns", desc_eq(44100), chunks({{0, 0, 3000}, {1, 3000, 2000}}));
        c.f0 = {0, 1};
        c.tot = {3000, 2001};
    }
    add("err_env_rounds", [] { auto d = desc(48000, 1); d.env_rounds = 17; return d; }(), TWO);
    add("err_eq_slow", [] { auto d = desc(48000); eq(d, 0); sos_slow(d.eq_coef[0]); return d; }(), TWO);
    add("err_xover_slow", [] { auto d = desc(48000, 1); sos_slow(d.xover_lo_sos); return d; }(), TWO);
    add("err_kw_slow", desc(8000001), TWO);   // measured at its own rate: the 38 Hz pole over 65536 frames
    // 3..8 channels
    for (int an = 0; an < 2; an++)
        for (int mb = 0; mb < 2; mb++) {
            amx_chain_desc d = an ? desc_f32(48000, mb, g_lut) : desc_eq(48000, mb);
            d.channels_in = 6;
            add(std::string("mc_6ch") + (an ? "_analog" : "") + (mb ? "_mb" : ""), d, TWO).mc = true;
        }
    add("mc_err_2ch", desc(48000), TWO).mc = true;
    add("mc_err_9ch", [] { auto d = desc(48000); d.channels_in = 9; return d; }(), TWO).mc = true;
    add("mc_err_analog_no_lut", [] { auto d = desc(48000); d.channels_in = 3; d.analog_on = 1; return d; }(), TWO).mc = true;
    add("mc_err_neg_chunk", [] { auto d = desc(48000); d.channels_in = 3; return d; }(), chunks({{0, 0, -5}})).mc = true;
    add("mc_err_null", [] { auto d = desc(48000); d.channels_in = 3; return d; }(), TWO).null_desc = true;
    v.back().mc = true;
    add("mc_err_analog_gain", [] { auto d = desc_f32(48000, 0, g_lut); d.channels_in = 4; d.analog_lo_gain = 1.0; return d; }(),
        TWO).mc = true;
    add("mc_err_sub_plan", [] { auto d = desc(48000, 1); d.channels_in = 4; d.comp_ratio[0] = 0.0; return d; }(), TWO).mc = true;
    return v;
}

// ------------------------------------------------------------------ reporting
int g_bad = 0;
bool g_full = false;

const standin::Upload *upload_of(const void *dst) {
    for (const standin::Upload &u : standin::uploads)
        if (u.dst == dst) return &u;
    return nullptr;
}
void digest(const char *pre, const char *name, const void *dev) {
    if (!dev) {
        printf("%sint %s -\n", pre, name);
        return;
    }
    const standin::Upload *u = upload_of(dev);
    if (!u) {   // an empty table: one element allocated, nothing copied
        printf("%sint %s %zu empty\n", pre, name, standin::size_of(dev));
        return;
    }
    printf("%sint %s %zu %016llx\n", pre, name, u->bytes, (unsigned long long)u->hash);
}
template <class T>
void floats(const char *pre, const char *name, const T *dev) {
    if (!dev) {
        printf("%sflt %s -\n", pre, name);
        return;
    }
    const size_t bytes = standin::size_of(dev), copied = upload_of(dev) ? upload_of(dev)->bytes : 0;
    bool finite = true;
    for (size_t i = 0; i < copied / sizeof(T); i++) finite = finite && std::isfinite((double)dev[i]);
    printf("%sflt %s %zu finite=%d\n", pre, name, bytes, finite ? 1 : 0);
    if (!finite) g_bad++;
}

int64_t pydub_len(int64_t n, int fs) {
    const double ms = std::nearbyint(1000.0 * ((double)n / (double)fs));
    return (int64_t)(ms * (fs / 1000.0));
}

#define REQ(c)                                                      \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("%sinv FAIL line %d: %s\n", pre, __LINE__, #c);  \
            g_bad++;                                                \
            return;                                                 \
        }                                                           \
    } while (0)

// blocks of at most AMX_SCAN_S segments tile each stream's run of segments, in order
template <class Run>
bool blocks_tile(const ScanBlk *blks, int n_blk, int n_streams, Run run) {
    int b = 0;
    for (int t = 0; t < n_streams; t++) {
        int32_t j0 = 0, n = 0;
        run(t, &j0, &n);
        const int first = b;
        for (int32_t q = j0; q < j0 + n;) {
            if (b >= n_blk) return false;
            const ScanBlk &B = blks[b++];
            if (B.seg0 != q || B.nseg < 1 || B.nseg > AMX_SCAN_S || B.first != first || B.stream != t) return false;
            q += B.nseg;
            if (B.last != (q == j0 + n ? 1 : 0) || q > j0 + n) return false;
        }
    }
    return b == n_blk;
}

void invariants(const char *pre, const amx_plan *p) {
    const int fs = p->cd.fs, L = p->L, nc = p->n_chunks;
    const ChunkDev *ch = p->d_chunks;
    const SegDev *segs = p->d_segs;
    const SpanDev *spans = p->d_spans;
    const KwSegDev *ks = p->d_ksegs;
    REQ(L > 0 && L % AMX_TF_FRAMES == 0);
    // chunks: scratch rows, output rows, segments
    int64_t loc = 0, outo = 0;
    int32_t seg = 0;
    for (int c = 0; c < nc; c++) {
        const ChunkDev &k = ch[c];
        REQ(k.loc_off == loc && k.loc_off % 16 == 0 && k.out_off == outo);
        const int64_t n1 = (p->mb && k.n > 0) ? pydub_len(k.n, fs) : k.n;
        REQ(p->d_n1[c] == n1);
        REQ(k.out_n == ((p->mb && k.n > 0) ? pydub_len(n1, fs) : k.n));
        REQ(k.seg0 == seg && k.nseg == (k.n + L - 1) / L);
        int64_t pos = 0;
        for (int32_t q = 0; q < k.nseg; q++) {
            const SegDev &s = segs[seg + q];
            REQ(s.pos == pos && s.chunk == c && s.len >= 1 && s.len <= L && s.first == k.seg0);
            REQ(s.last == (q == k.nseg - 1 ? 1 : 0));
            pos += s.len;
        }
        REQ(pos == k.n);
        seg += k.nseg;
        loc += (k.n + 15) / 16 * 16;
        outo += k.out_n;
    }
    REQ(seg == p->n_seg && loc == p->nloc && outo == p->out_frames);
    REQ(blocks_tile(p->d_blks, p->n_blk, nc, [&](int c, int32_t *j0, int32_t *n) { *j0 = ch[c].seg0; *n = ch[c].nseg; }));
    // envelope tables
    if (p->mb) {
        int ld = 0;
        for (int t = 1; t <= 3; t++) {
            const auto &tab = p->cd.etab[t];
            REQ(tab.Le == p->Le_t[t] && tab.Le >= 128 && tab.Le % 128 == 0);
            const SegDev *es = p->d_esegs + tab.es_off;
            const int *e0 = p->d_eseg0 + tab.ch_off, *ne = p->d_neseg + tab.ch_off;
            int run = 0;
            for (int c = 0; c < nc; c++) {
                REQ(e0[c] == run && ne[c] == (ch[c].n + tab.Le - 1) / tab.Le);
                int64_t pos = 0;
                for (int q = 0; q < ne[c]; q++) {
                    const SegDev &s = es[run + q];
                    REQ(s.pos == pos && s.chunk == c && s.len >= 1 && s.len <= tab.Le && s.first == e0[c]);
                    REQ(s.last == (q == ne[c] - 1 ? 1 : 0));
                    pos += s.len;
                }
                REQ(pos == ch[c].n);
                run += ne[c];
            }
            REQ(run == tab.n_es);
            ld = std::max(ld, run);
        }
        REQ(p->cd.es_ld == ld && p->n_es == ld);
        REQ(memcmp(&p->cd.etab[0], &p->cd.etab[3], sizeof p->cd.etab[0]) == 0);
        REQ(p->Le == p->Le_t[3]);
    }
    // spans and K segments
    const int Lseg = p->resamp ? p->upLout : p->Lkw, Lsin = p->resamp ? p->upLin : p->Lkw;
    int64_t run_out = 0;
    int32_t kseg = 0;
    for (int t = 0; t < p->n_tracks; t++) {
        const SpanDev &sp = spans[t];
        int64_t sum = 0, first_off = -1;
        for (int c = 0; c < nc; c++)
            if (ch[c].track == t) {
                if (first_off < 0) first_off = ch[c].out_off;
                sum += ch[c].out_n;
            }
        REQ(sp.out_n == sum && sp.out_off == (first_off < 0 ? 0 : first_off));
        if (sp.out_n > 0) REQ(sp.out_off == run_out);
        run_out += sp.out_n;
        REQ(sp.kseg0 == kseg && sp.nkseg == (sp.m_n + Lseg - 1) / Lseg);
        REQ(sp.edge_lo == (sp.tframe0 > 0) && sp.edge_hi == (sp.tframe0 + sp.out_n < sp.ttotal));
        int64_t tf = sp.m_tframe0;
        for (int32_t q = 0; q < sp.nkseg; q++) {
            const KwSegDev &s = ks[kseg + q];
            REQ(s.tframe == tf && s.track == t && s.len >= 1 && s.len <= Lseg && s.first == sp.kseg0);
            REQ(s.last == (q == sp.nkseg - 1 ? 1 : 0) && s.out_pos == sp.out_off + (int64_t)q * Lsin);
            tf += s.len;
        }
        REQ(tf == sp.m_tframe0 + sp.m_n);
        kseg += sp.nkseg;
    }
    REQ(kseg == p->n_kseg && run_out == p->out_frames);
    REQ(blocks_tile(p->d_kblks, p->n_kblk, p->n_tracks,
                    [&](int t, int32_t *j0, int32_t *n) { *j0 = spans[t].kseg0; *n = spans[t].nkseg; }));
    // the slow list: sorted, exactly the segments that fail the fast test
    if (p->resamp && (p->up_static || p->up_poly)) {
        std::vector<int32_t> slow;
        for (int32_t j = 0; j < p->n_kseg; j++) {
            const KwSegDev &sg = ks[j];
            const SpanDev &sp = spans[sg.track];
            const int64_t g0 = sg.out_pos - sp.out_off;
            const int64_t split = (sg.tframe / p->hop + 1) * p->hop - sg.tframe;
            if (!(g0 - 15 >= 0 && g0 + p->upLin + 17 <= sp.out_n && sg.len == p->upLout && split >= p->upLout))
                slow.push_back(j);
        }
        REQ((int64_t)slow.size() == p->n_slow && (slow.empty() ? p->d_slow == nullptr : p->d_slow != nullptr));
        for (size_t i = 0; i < slow.size(); i++) REQ(p->d_slow[i] == slow[i]);
    } else if (p->resamp) {
        REQ(p->n_slow == p->n_kseg && p->d_slow == nullptr);
    }
    if (p->up_poly) {
        int64_t sum = 0;
        for (int n = 0; n < p->upLout; n++) REQ(p->d_obase[n] >= (n ? p->d_obase[n - 1] : 0) && p->d_obase[n] < p->upLin);
        for (int f = 0; f < p->upLin; f++) sum += p->d_fcnt[f];
        REQ(sum == p->upLout);
    }
    // workspace: 256-byte aligned regions that do not overlap, ws_bytes past the last
    std::vector<std::pair<size_t, size_t>> reg;
    const size_t nl = (size_t)p->nloc, ns = (size_t)p->n_seg, nk = (size_t)p->n_kseg, D = p->D ? p->D : 1;
    reg.push_back({p->o_a16, nl * 4});
    reg.push_back({p->o_e, ns * 2 * D * 8});
    reg.push_back({p->o_s, ns * 2 * D * 8});
    if (p->mb) {
        const size_t ne = (size_t)p->n_es, mpad = (size_t)std::max(std::max(p->warm, p->Le), 1024) + 64;
        reg.push_back({p->o_p16, nl * 4});
        reg.push_back({p->o_ex, ns * 2 * AMX_XO_DIM * 8});
        reg.push_back({p->o_sx, ns * 2 * AMX_XO_DIM * 8});
        reg.push_back({p->o_bands, 3 * nl * 4});
        reg.push_back({p->o_gain, (3 * nl / 16 + 64) * 8});
        REQ(p->o_m >= mpad * 2);
        reg.push_back({p->o_m - mpad * 2, (3 * nl + 2 * mpad) * 2});
        reg.push_back({p->o_esv, 3 * ne * 8});
        reg.push_back({p->o_ee0, 3 * ne * 8});
        reg.push_back({p->o_eflags, (AMX_ENV_LIST + 3) * 4});
        for (size_t o : {p->o_eact, p->o_ehead, p->o_elist, p->o_eprev, p->o_elist0}) reg.push_back({o, 3 * ne * 4});
        reg.push_back({p->o_ebx, (size_t)p->n_blk * 2 * AMX_XO_DIM * 8});
    }
    if (p->mono16) reg.push_back({p->o_dup, (size_t)p->in_frames * 4});
    reg.push_back({p->o_eb, (size_t)p->n_blk * 2 * D * 8});
    reg.push_back({p->o_ebk, (size_t)p->n_kblk * 2 * AMX_KW_DIM * 8});
    reg.push_back({p->o_ekw, nk * 2 * AMX_KW_DIM * 8});
    reg.push_back({p->o_pk, nk * 4 * 4});
    reg.push_back({p->o_skw, nk * 2 * AMX_KW_DIM * 8});
    reg.push_back({p->o_parts, nk * 4 * 8});
    if (p->resamp) reg.push_back({p->o_eterms, nk * 2 * 10 * 8});
    reg.push_back({p->o_phop, nk * 8});
    std::sort(reg.begin(), reg.end());
    size_t end = 0;
    for (const auto &r : reg) {
        REQ(r.first % 256 == 0 && r.first >= end);
        end = r.first + r.second;
    }
    REQ(p->ws_bytes % 256 == 0 && p->ws_bytes >= end);
    printf("%sinv ok\n", pre);
}

void report(const char *pre, const amx_plan *p) {
    amx_plan_info in;
    if (amx_plan_get_info(p, &in) != AMX_OK) g_bad++;
    printf("%sinfo ws=%lld out=%lld tracks=%d chunks=%d segs=%lld L=%d lev=%d,%d,%d D=%d hop=%d rate=%d hops=%lld\n", pre,
           (long long)in.workspace_bytes, (long long)in.out_frames, in.n_tracks, in.n_chunks, (long long)in.n_segments,
           in.seg_frames, in.scan_levels_eq, in.scan_levels_xover, in.scan_levels_kw, in.eq_dim, in.hop_frames,
           in.meas_rate, (long long)in.max_hops);
    for (int t = 0; t < in.n_tracks; t++) {
        amx_track_span s;
        if (amx_plan_track_span(p, t, &s) != AMX_OK) g_bad++;
        printf("%sspan %d off=%lld n=%lld f0=%lld total=%lld\n", pre, t, (long long)s.out_offset, (long long)s.out_frames,
               (long long)s.track_frame0, (long long)s.track_frames_total);
    }
    printf("%shost resamp=%d up=%d/%d Lin=%d Lout=%d static=%d ok=%d native=%d pc=%d lin=%d taps=%d/%d poly=%d nslow=%lld "
           "Lkw=%d Le=%d,%d,%d,%d warm=%d rounds=%d wg=%d pin=%d f1=%d n_es=%d fuse=%d aligned=%d kseg=%d blk=%d,%d "
           "maxk=%lld nloc=%lld maxout=%lld maxspan=%lld maxn=%lld anb=%lld anv=%d in=%lld mono=%d sc=%d empty=%d\n",
           pre, p->resamp, p->upL, p->upM, p->upLin, p->upLout, p->up_static, p->up_ok, p->meas_native, p->up_pc, p->up_lin,
           p->up_taps, p->up_alloc, p->up_poly, (long long)p->n_slow, p->Lkw, p->Le, p->Le_t[1], p->Le_t[2], p->Le_t[3],
           p->warm, p->rounds, p->env_wg, p->env_pin, p->f1_mode, p->n_es, p->fuse_kw, p->kw_aligned, p->n_kseg, p->n_blk,
           p->n_kblk, (long long)p->max_nkseg, (long long)p->nloc, (long long)p->max_chunk_out, (long long)p->max_span,
           (long long)p->max_chunk_n, (long long)p->an_blocks, p->an_vec, (long long)p->in_frames, p->mono16, p->sc,
           p->any_empty_span);
    printf("%soff a16=%zu e=%zu s=%zu p16=%zu ex=%zu sx=%zu bands=%zu m=%zu gain=%zu esv=%zu ee0=%zu eflags=%zu "
           "eact=%zu ehead=%zu elist=%zu eprev=%zu elist0=%zu ekw=%zu skw=%zu parts=%zu phop=%zu eterms=%zu eb=%zu "
           "ebx=%zu ebk=%zu pk=%zu dup=%zu\n",
           pre, p->o_a16, p->o_e, p->o_s, p->o_p16, p->o_ex, p->o_sx, p->o_bands, p->o_m, p->o_gain, p->o_esv, p->o_ee0,
           p->o_eflags, p->o_eact, p->o_ehead, p->o_elist, p->o_eprev, p->o_elist0, p->o_ekw, p->o_skw, p->o_parts,
           p->o_phop, p->o_eterms, p->o_eb, p->o_ebx, p->o_ebk, p->o_pk, p->o_dup);
    digest(pre, "chunks", p->d_chunks);
    digest(pre, "segs", p->d_segs);
    digest(pre, "blks", p->d_blks);
    digest(pre, "esegs", p->d_esegs);
    digest(pre, "eseg0", p->d_eseg0);
    digest(pre, "neseg", p->d_neseg);
    digest(pre, "ksegs", p->d_ksegs);
    digest(pre, "kblks", p->d_kblks);
    digest(pre, "spans", p->d_spans);
    digest(pre, "n1", p->d_n1);
    digest(pre, "obase", p->d_obase);
    digest(pre, "oph", p->d_oph);
    digest(pre, "fcnt", p->d_fcnt);
    digest(pre, "slow", p->d_slow);
    digest(pre, "pcnt", p->d_pcnt);
    printf("%ssize cd %zu ppart %zu\n", pre, standin::size_of(p->d_cd), standin::size_of(p->d_ppart));
    floats(pre, "G", p->d_G);
    floats(pre, "M", p->d_M);
    floats(pre, "Mp", p->d_Mp);
    floats(pre, "Gx", p->d_Gx);
    floats(pre, "Mx", p->d_Mx);
    floats(pre, "Mpx", p->d_Mpx);
    floats(pre, "Gkw", p->d_Gkw);
    floats(pre, "Mkw", p->d_Mkw);
    floats(pre, "Mpkw", p->d_Mpkw);
    floats(pre, "qh", p->d_qh);
    floats(pre, "qt", p->d_qt);
    floats(pre, "tabs", p->d_tabs);
    floats(pre, "bounds", p->d_bounds);
    floats(pre, "energies", p->d_energies);
    floats(pre, "tailpow", p->d_tailpow);
    floats(pre, "owt", p->d_owt);
    floats(pre, "bank", p->d_bank);
    floats(pre, "bankn", p->d_bankn);
    floats(pre, "lut", p->d_lut);
    floats(pre, "in_lut", p->d_in_lut);
    floats(pre, "lut_half", p->d_lut_half);
    invariants(pre, p);
}

void set_env(const Case &c) {
    for (const char *k : KNOBS) unsetenv(k);
    for (const auto &e : c.env) setenv(e.first, e.second, 1);
    standin::reset();
    standin::ncu = c.ncu;
}
int create(const Case &c, amx_plan **out) {
    const int n = c.n_chunks == INT_MIN ? (int)c.ch.size() : c.n_chunks;
    return amx_plan_create(c.null_desc ? nullptr : &c.d, c.null_chunks ? nullptr : c.ch.data(), n,
                           c.f0.empty() ? nullptr : c.f0.data(), c.tot.empty() ? nullptr : c.tot.data(), c.seg,
                           c.null_out ? nullptr : out);
}

void print_uploads() {
    std::vector<std::pair<size_t, uint64_t>> u;
    for (const standin::Upload &x : standin::uploads) u.push_back({x.bytes, x.hash});
    std::sort(u.begin(), u.end());
    for (const auto &x : u) printf("up %zu %016llx\n", x.first, (unsigned long long)x.second);
}

void run_case(const Case &c) {
    set_env(c);
    printf("case %s\n", c.name.c_str());
    int rc;
    if (c.mc) {
        amx_mc_plan *m = nullptr;
        rc = amx_mc_plan_create(c.null_desc ? nullptr : &c.d, c.ch.data(), (int)c.ch.size(), c.seg, &m);
        printf("rc=%d err=%s\n", rc, rc ? amx_last_error() : "");
        if (rc == AMX_OK) {
            int64_t ws = 0, of = 0;
            amx_mc_plan_get_info(m, &ws, &of);
            printf("mc ws=%lld out=%lld C=%d M=%lld off=%zu,%zu,%zu,%zu,%zu,%zu\n", (long long)ws, (long long)of, m->C,
                   (long long)m->M, m->o_pack, m->o_outa, m->o_outb, m->o_wa, m->o_wb, m->o_wc);
            if (m->pa) report("pa.", m->pa);
            report("pb.", m->pb);
            if (m->pc) report("pc.", m->pc);
        } else if (m) {
            printf("FAIL: *out set on error\n");
            g_bad++;
        }
        if (g_full) print_uploads();
        amx_mc_plan_free(m);
    } else {
        amx_plan *p = nullptr;
        rc = create(c, &p);
        printf("rc=%d err=%s\n", rc, rc ? amx_last_error() : "");
        if (rc == AMX_OK) report("", p);
        else if (p) {
            printf("FAIL: *out set on error\n");
            g_bad++;
        }
        if (g_full) print_uploads();
        amx_plan_free(p);
    }
    if (standin::live() != 0) {
        printf("FAIL: %zu allocations live after free\n", standin::live());
        g_bad++;
    }
}

// --plan NAME FS N0[,N1...] F0|- TOTAL|- KNOB=VALUE|-: a measure-only plan of tracks laid back to
// back (F0 / TOTAL: the first track's place in its file), reported as a case, and its
// resampler bank: every row (the pc phases and the interpolation partner) has a tap > 0
void run_plan(char **a) {
    Case c;
    c.name = a[0];
    c.d = desc_eq(atoi(a[1]));
    c.d.measure_only = 1;
    int64_t off = 0;
    int32_t t = 0;
    for (const char *s = a[2]; *s; t++) {
        char *end;
        amx_chunk k{};
        k.track = t;
        k.in_offset = off;
        k.frames = strtoll(s, &end, 10);
        off += k.frames;
        c.ch.push_back(k);
        s = *end ? end + 1 : end;
    }
    if (strcmp(a[3], "-")) c.f0.assign(c.ch.size(), 0), c.f0[0] = atoll(a[3]);
    if (strcmp(a[4], "-")) {
        for (const amx_chunk &k : c.ch) c.tot.push_back(k.frames);
        c.tot[0] = atoll(a[4]);
        if (c.f0.empty()) c.f0.assign(c.ch.size(), 0);
    }
    std::string knob = a[5];
    const size_t eq_at = knob.find('=');
    if (eq_at != std::string::npos) {
        knob[eq_at] = 0;
        c.env.push_back({knob.c_str(), knob.c_str() + eq_at + 1});
    }
    set_env(c);
    printf("case %s\n", c.name.c_str());
    amx_plan *p = nullptr;
    const int rc = create(c, &p);
    printf("rc=%d err=%s\n", rc, rc ? amx_last_error() : "");
    if (rc == AMX_OK) {
        report("", p);
        const int n_rows = (int)(standin::size_of(p->d_bank) / sizeof(float) / (size_t)p->up_alloc);
        int rows = 0, bad = 0;
        if (p->resamp && p->up_ok)
            for (; rows < n_rows; rows++) {
                const float *h = p->d_bank + (size_t)rows * p->up_alloc;
                bad += std::none_of(h, h + p->up_alloc, [](float v) { return v > 0.0f; }) ? 1 : 0;
            }
        printf("bank rows=%d without_positive_tap=%d\n", rows, bad);
    }
    amx_plan_free(p);
}

// ------------------------------------------------------------------ ownership
#define OWN(c)                                                  \
    do {                                                        \
        if (!(c)) {                                             \
            printf("own FAIL line %d: %s\n", __LINE__, #c);     \
            g_bad++;                                            \
        }                                                       \
    } while (0)

void ownership() {
    Case c;
    c.name = "own";
    c.d = desc_f32(44100, 1, g_lut);
    c.ch = TWO;
    // every allocation of one multiband 44.1 kHz plan fails in turn, then the event creation
    set_env(c);
    amx_plan *p = nullptr;
    OWN(create(c, &p) == AMX_OK && p && p->up_aux && p->up_fork);
    const int n_alloc = standin::mallocs;
    amx_plan_free(p);
    OWN(standin::live() == 0);
    for (int k = 1; k <= n_alloc; k++) {
        set_env(c);
        standin::fail_malloc_at = k;
        p = reinterpret_cast<amx_plan *>(&c);
        OWN(create(c, &p) == AMX_EHIP && p == nullptr && standin::live() == 0);
    }
    set_env(c);
    standin::fail_event = 1;
    p = reinterpret_cast<amx_plan *>(&c);
    OWN(create(c, &p) == AMX_EHIP && p == nullptr && standin::live() == 0);
    OWN(std::string(amx_last_error()) == "stream / event creation failed");
    printf("own allocation failures: %d allocations, each failed once\n", n_alloc);
    // amx_limiter_prepare twice with different segment sizes, then under an injected failure
    set_env(c);
    OWN(create(c, &p) == AMX_OK);
    amx_final_desc fd{};
    fd.limit = 0.98;
    fd.attack_ms = 5.0;
    fd.release_ms = 50.0;
    fd.level_in = fd.level_out = 1.0;
    fd.auto_level = 1;
    OWN(amx_limiter_prepare(p, &fd, 4096, -1) == AMX_OK);
    const void *s0 = p->lim.seg_state;
    OWN(amx_limiter_prepare(p, &fd, 4096, -1) == AMX_OK && p->lim.seg_state == s0);   // same geometry: kept
    OWN(amx_limiter_prepare(p, &fd, 1024, -1) == AMX_OK && p->lim.seg_frames == 1024);
    OWN(standin::size_of(s0) == 0 || p->lim.seg_state == s0);                          // the old one released
    for (int k = 1; k <= 2; k++) {
        const void *s1 = p->lim.seg_state, *c1 = p->lim.cnt;
        const size_t live = standin::live(), bytes = standin::size_of(s1);
        standin::fail_malloc_at = k;
        OWN(amx_limiter_prepare(p, &fd, 2048, -1) == AMX_EHIP);
        OWN(p->lim.seg_state == s1 && p->lim.cnt == c1 && p->lim.seg_frames == 1024);
        OWN(standin::live() == live && standin::size_of(s1) == bytes && bytes > 0 && standin::size_of(c1) > 0);
    }
    OWN(amx_limiter_prepare(p, &fd, 2048, -1) == AMX_OK && p->lim.seg_frames == 2048);
    // amx_kw_carry_setup twice
    const int64_t after[3] = {1000, 48000, 0};
    OWN(amx_kw_carry_setup(p, 2, after) == AMX_OK && p->n_prev == 2 && standin::size_of(p->d_carryP) == 2 * 16 * 8);
    OWN(amx_kw_carry_setup(p, 3, after) == AMX_OK && p->n_prev == 3 && standin::size_of(p->d_carryP) == 3 * 16 * 8);
    OWN(amx_kw_carry_setup(p, 0, nullptr) == AMX_OK && p->n_prev == 0 && standin::size_of(p->d_carryP) == 16 * 8);
    amx_plan_free(p);
    OWN(standin::live() == 0);
    // a multichannel plan whose second / third sub-plan fails releases the earlier ones
    c.d.channels_in = 5;
    set_env(c);
    amx_mc_plan *m = nullptr;
    OWN(amx_mc_plan_create(&c.d, c.ch.data(), (int)c.ch.size(), 0, &m) == AMX_OK && m);
    const int n_mc = standin::mallocs;
    amx_mc_plan_free(m);
    for (int k = 1; k <= n_mc; k += 7) {
        set_env(c);
        standin::fail_malloc_at = k;
        m = reinterpret_cast<amx_mc_plan *>(&c);
        OWN(amx_mc_plan_create(&c.d, c.ch.data(), (int)c.ch.size(), 0, &m) == AMX_EHIP && m == nullptr &&
            standin::live() == 0);
    }
    printf("own done\n");
}

}  // namespace ph

int main(int argc, char **argv) {
    const char *only = nullptr;
    bool plans = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--full")) ph::g_full = true;
        else if (!strcmp(argv[i], "--plan") && i + 6 < argc) {
            ph::run_plan(argv + i + 1);
            i += 6;
            plans = true;
        } else only = argv[i];
    }
    if (plans) {
        printf("%d failed\n", ph::g_bad);
        return ph::g_bad ? 1 : 0;
    }
    for (const ph::Case &c : ph::cases())
        if (!only || c.name == only) ph::run_case(c);
    if (!only) ph::ownership();
    printf("%d failed\n", ph::g_bad);
    return ph::g_bad ? 1 : 0;
}
