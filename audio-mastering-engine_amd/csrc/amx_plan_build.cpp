// amx_plan_build.cpp -- host-only plan construction (amx_plan_build.hpp): resampler
// geometry and bank, chain / K-weighting coefficients, compressor tables, the chunk,
// segment, block, envelope-segment and K-segment tables, the state-space models and scan
// matrices, the workspace layout.  Pure arithmetic on its arguments: no HIP, no
// environment reads but PlanKnobs::from_env().
#include "amx_plan_build.hpp"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace amx {
namespace {

// ------------------------------------------------------------ dense helpers
// The scan tables (GEMV rows A^n B, A^L, block powers) are computed in long double (x86
// 80-bit, 64-bit mantissa) and rounded to double once: built in double by repeated
// products they carried ~1e-12 of error into the segment start states at 96 kHz
// (DESIGN.md §3.1), 20x the sequential recursion's own rounding; rounded once they
// carry less than it.
using LD = long double;

MatL matmul(const MatL &a, const MatL &b, int D) {
    MatL c((size_t)D * D, 0.0L);
    for (int i = 0; i < D; i++)
        for (int k = 0; k < D; k++) {
            const LD v = a[(size_t)i * D + k];
            if (v == 0.0L) continue;
            for (int j = 0; j < D; j++) c[(size_t)i * D + j] += v * b[(size_t)k * D + j];
        }
    return c;
}
MatL matpow(const MatL &a, int64_t p, int D) {
    MatL r((size_t)D * D, 0.0L), b = a;
    for (int i = 0; i < D; i++) r[(size_t)i * D + i] = 1.0L;
    while (p > 0) {
        if (p & 1) r = matmul(r, b, D);
        b = matmul(b, b, D);
        p >>= 1;
    }
    return r;
}
LD norm_inf(const MatL &a, int D) {
    LD m = 0.0L;
    for (int i = 0; i < D; i++) {
        LD s = 0.0L;
        for (int j = 0; j < D; j++) s += std::fabs(a[(size_t)i * D + j]);
        m = s > m ? s : m;
    }
    return m;
}
Mat to_double(const MatL &a) { return Mat(a.begin(), a.end()); }

// host step functions (same math as the device chains, no rounding claims)
template <class T>
void shelf_step_h(const double *c, T *z, T &x, int neg, double gm1) {
    T y = z[0] + (T)c[0] * x;
    z[0] = (z[1] + x * (T)c[1]) - y * (T)c[4];
    z[1] = x * (T)c[2] - y * (T)c[5];
    x = neg ? y : x + (y - x) * (T)gm1;
}
template <class T>
T sos_step_h(const double *c, T *z, T x) {
    T y = (T)c[0] * x + z[0];
    z[0] = ((T)c[1] * x - (T)c[4] * y) + z[1];
    z[1] = (T)c[2] * x - (T)c[5] * y;
    return y;
}

size_t align_up(size_t &off, size_t bytes) {
    size_t o = (off + 255) & ~(size_t)255;
    off = o + bytes;
    return o;
}

// blocks of AMX_SCAN_S segments over each stream's run [j0, j0 + n) of segments
void add_blocks(std::vector<ScanBlk> &out, int32_t j0, int32_t n, int32_t stream) {
    const int32_t first = (int32_t)out.size();
    for (int32_t q = 0; q < n; q += AMX_SCAN_S) {
        ScanBlk b{};
        b.seg0 = j0 + q;
        b.nseg = (n - q) < AMX_SCAN_S ? (n - q) : AMX_SCAN_S;
        b.first = first;
        b.last = (q + AMX_SCAN_S >= n) ? 1 : 0;
        b.stream = stream;
        out.push_back(b);
    }
}

int64_t overlay_len(int64_t n, int fs) {
    // pydub: int(round(1000*(n/fs)) * (fs/1000.0)), Python round = half-to-even
    double ms = std::nearbyint(1000.0 * ((double)n / (double)fs));
    return (int64_t)(ms * (fs / 1000.0));
}

}  // namespace

// scales Gx by 2^-15 in place and returns true when every entry of G and Gx times 2^-15
// is exact (zero, or still normal); else leaves both as they are (lti_models)
bool scale_gemv_rows(const std::vector<double> &G, std::vector<double> &Gx) {
    for (const std::vector<double> *t : {&G, static_cast<const std::vector<double> *>(&Gx)})
        for (double g : *t)
            if (!(g == 0.0 || std::fabs(g) >= 0x1p-1007)) return false;
    for (double &g : Gx) g *= 0x1p-15;
    return true;
}

Mat Lti::pow(int64_t p) const { return to_double(matpow(A, p, D)); }
std::vector<double> Lti::gemv_table(int L) const {
    std::vector<double> G((size_t)L * D);
    std::vector<LD> v = B, t(D);
    for (int n = L - 1; n >= 0; n--) {
        for (int d = 0; d < D; d++) G[(size_t)n * D + d] = (double)v[d];
        for (int i = 0; i < D; i++) {
            LD acc = 0.0L;
            for (int k = 0; k < D; k++) acc += A[(size_t)i * D + k] * v[k];
            t[i] = acc;
        }
        v = t;
    }
    return G;
}
int Lti::window_powers(int64_t LS, double tol, int max_k, std::vector<double> &out) const {
    MatL Mb = matpow(A, LS, D);
    MatL cur = Mb;
    out.clear();
    int K = 1;
    while (norm_inf(cur, D) > tol) {
        for (LD v : cur) out.push_back((double)v);
        cur = matmul(cur, Mb, D);
        K++;
        if (K > max_k) return -1;
    }
    return K;
}

// libswresample's resampler geometry and filter bank for the loudness measurement's
// 192 kHz stream (what ffmpeg inserts ahead of af_loudnorm in dynamic mode, :229).
// Restated from resample.c resample_init / build_filter with swresample's defaults:
// filter_size 32, phase_shift 10, exact_rational 1, cutoff 0.97, Kaiser beta 9, FLTP
// (float32 bank, scale 1).  Upsampling only (factor 1); L / M = out / in reduced (output j
// sits at input position j M / L).  The bank has L phases when L <= 1024 (exact_rational)
// and 1024 otherwise (22.05 / 11.025 kHz): the position then falls between two phases and
// libswresample's linear kernel interpolates (amx_swr_dev.hpp swr_dot_lin).
int swr_geometry(int in_rate, int out_rate, int *L, int *M) {
    if (in_rate <= 0 || out_rate <= 0) return -1;
    int64_t a = in_rate, b = out_rate;
    while (b) { int64_t t = a % b; a = b; b = t; }
    *L = (int)(out_rate / a);
    *M = (int)(in_rate / a);
    return 0;
}

// resample_init: factor = min(out_rate * cutoff / in_rate, 1) (cutoff 0.97); filter_length
// = max(ceil(filter_size / factor), 1) rounded up to even; rows of filter_alloc =
// FFALIGN(filter_length, 8) floats.  An input above 192 kHz / 0.97 (352.8 / 384 / 705.6 /
// 768 kHz) is DOWNsampled with the longer, narrower filter.  Equal rates: no resampler
// (ffmpeg only converts the sample format), the 32-tap identity row.
int swr_filter(int in_rate, int out_rate, int *taps, int *alloc, double *factor, int max_alloc) {
    if (in_rate <= 0 || out_rate <= 0) return -1;
    double f = out_rate * 0.97 / in_rate;
    if (f > 1.0 || in_rate == out_rate) f = 1.0;
    int t = (int)std::ceil(32 / f);
    if (t < 1) t = 1;
    if (t > 1) t = (t + 1) & ~1;
    const int al = (t + 7) & ~7;
    if (al > max_alloc) return -1;
    if (taps) *taps = t;
    if (alloc) *alloc = al;
    if (factor) *factor = f;
    return 0;
}

// resample_init: phase_count 1 << phase_shift (1024), replaced by the exact out / gcd
// when that is <= 1024 (exact_rational).  The interpolating (1024-phase) form is restated
// for the 32-tap filter only.
int swr_phases(int in_rate, int out_rate, int max_alloc) {
    int L, M, t;
    if (swr_geometry(in_rate, out_rate, &L, &M) || swr_filter(in_rate, out_rate, &t, nullptr, nullptr, max_alloc))
        return -1;
    if (L > 1024 && t != 32) return -1;
    return L <= 1024 ? L : 1024;
}

// resample_init: av_reduce(&src_incr, &dst_incr, out_rate, in_rate * phase_count), both
// doubled while below 2^20; output j sits at phase position j dst_incr / src_incr
int swr_incr(int in_rate, int out_rate, int64_t *src_incr, int64_t *dst_incr) {
    const int pc = swr_phases(in_rate, out_rate);
    if (pc < 0) return -1;
    int64_t a = out_rate, b = (int64_t)in_rate * pc, x = a, y = b;
    while (y) { int64_t t = x % y; x = y; y = t; }
    a /= x;
    b /= x;
    while (b < (1 << 20) && a < (1 << 20)) { a *= 2; b *= 2; }
    *src_incr = a;
    *dst_incr = b;
    return 0;
}

static double swr_bessel(double x) {
    double lastv = 0, t, v;
    double inv[100];
    for (int k = 0; k < 100; k++) inv[k] = 1.0 / ((double)(k + 1) * (double)(k + 1));
    x = x * x / 4;
    t = x;
    v = 1 + x;
    for (int i = 1; v != lastv && i < 98; i += 2) {
        t *= x * inv[i];
        v += t;
        lastv = v;
        t *= x * inv[i + 1];
        v += t;
    }
    return v;
}

// build_filter (Kaiser beta 9, FLTP, scale 1): pc rows of filter_alloc floats (zeros past
// filter_length); factor 1 forms sin(x) / x from an alternating sine table, factor < 1
// from sin(x) itself
int swr_bank(int in_rate, int out_rate, float *bank, int max_alloc) {
    const int pc = swr_phases(in_rate, out_rate, max_alloc);
    int taps = 0, alloc = 0;
    double factor = 1.0;
    if (pc < 0 || swr_filter(in_rate, out_rate, &taps, &alloc, &factor, max_alloc)) return -1;
    const int center = (taps - 1) / 2;
    const int ph_nb = pc % 2 ? pc : pc / 2 + 1;
    std::vector<double> sin_lut(ph_nb), tab(taps);
    double norm = 0;
    std::fill(bank, bank + (size_t)pc * alloc, 0.0f);
    if (factor == 1.0)
        for (int ph = 0; ph < ph_nb; ph++) sin_lut[ph] = std::sin(M_PI * ph / pc) * (center & 1 ? 1 : -1);
    for (int ph = 0; ph < ph_nb; ph++) {
        double sv = factor == 1.0 ? sin_lut[ph] : 0.0;
        for (int i = 0; i < taps; i++) {
            const double x = M_PI * ((double)(i - center) - (double)ph / pc) * factor;
            double y = x == 0 ? 1.0 : (factor == 1.0 ? sv / x : std::sin(x) / x);
            const double w = 2.0 * x / (factor * taps * M_PI);
            y *= swr_bessel(9.0 * std::sqrt(std::max(1 - w * w, 0.0)));
            tab[i] = y;
            sv = -sv;
            if (!ph) norm += y;
        }
        for (int i = 0; i < taps; i++) bank[ph * alloc + i] = (float)(tab[i] * 1 / norm);
        if (pc % 2) continue;
        if (pc - ph < pc)
            for (int i = 0; i < taps; i++) bank[(pc - ph) * alloc + taps - 1 - i] = bank[ph * alloc + i];
    }
    return 0;
}

PlanKnobs PlanKnobs::from_env() {
    PlanKnobs k;
    if (const char *ev = std::getenv("AMX_UP_POLY")) k.up_poly = std::atoi(ev) != 0;
    // (tests: AMX_F1 = 2 runs the full-table form k_front1s, the path a table that is
    // not odd takes)
    if (const char *ev = std::getenv("AMX_F1")) k.f1 = std::atoi(ev) == AMX_F1_FULL ? AMX_F1_FULL : AMX_F1_SPLIT;
    return k;
}

namespace {

// build_plan_host's phases, in the order they run; p is the plan being filled
struct Builder {
    PlanHost *p;
    const amx_chain_desc *desc;
    const amx_chunk *chunks;
    int n_chunks;
    const int64_t *track_frame0, *track_total_frames;
    const PlanKnobs &knobs;
    int ncu;
    std::string &err;
    int fs = 0;
    int kfs = AMX_MEAS_RATE;   // the loudness measurement's rate: 192 kHz (af_loudnorm dynamic mode, :229)
    int64_t pattern = -1;      // the spans' common 192 kHz phase pattern (k_segments)

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }

    int check_arguments();
    void measurement_stream();
    int chain_coefficients();
    void kw_coefficients();
    int compressor_tables();
    int count_tracks();
    void envelope_sizing();
    int chunk_tables();
    void envelope_tables();
    int k_segments();
    void resampler_phases();
    void slow_list();
    int lti_models();
    void histogram_tables();
    void tanh_half();
    void workspace_layout();
};

int Builder::check_arguments() {
    if (desc->sample_rate <= 0) return fail(AMX_EINVAL, "sample_rate must be > 0");
    if (desc->channels_in != 1 && desc->channels_in != 2)
        return fail(AMX_EINVAL, "channels_in must be 1 or 2");
    if (desc->analog_on && !desc->tanh_lut)
        return fail(AMX_EINVAL, "analog character needs the float32 tanh table (tanh_lut)");
    if (desc->stream_chain && (desc->analog_on || desc->width_on || !desc->input_s16 || desc->channels_in != 2))
        return fail(AMX_EINVAL, "a stream chain takes int16 pairs, without analog character or width");
    return AMX_OK;
}

// measurement-stream geometry and the resampler bank
void Builder::measurement_stream() {
    std::vector<float> &bank = p->bank;
    if (fs != kfs) {
        p->resamp = 1;
        if (amx::swr_geometry(fs, kfs, &p->upL, &p->upM) != 0 || amx::swr_phases(fs, kfs) < 0) {
            // a rate whose resampler is not restated (an interpolating downsampler: L >
            // 1024 with the longer filter): the plan measures at the track's own rate,
            // which gives the limiter its peaks (the only measurement lufs=None needs);
            // amx_loudness_decide refuses loudnorm on it.
            p->up_ok = 0;
            p->resamp = 0;
            p->meas_native = 1;
            p->upL = p->upM = 1;
            kfs = fs;
        } else {
            // ~480 192 kHz outputs per K segment, a divisor of the 100 ms hop (19200)
            // where one exists, so a segment lies inside one hop (no hop split)
            const int hop192 = (kfs + 5) / 10;
            const int target = 480;
            p->up_pc = amx::swr_phases(fs, kfs);
            amx::swr_filter(fs, kfs, &p->up_taps, &p->up_alloc, nullptr);
            amx::swr_incr(fs, kfs, &p->up_src, &p->up_dst);
            p->up_lin = (p->up_dst % p->up_src) != 0;
            int kk = std::max(1, (target + p->upL / 2) / p->upL);
            for (int d = 0; d <= kk; d++) {
                if (kk - d >= 1 && hop192 % (p->upL * (kk - d)) == 0 && (p->upM * (kk - d)) % 8 == 0) { kk -= d; break; }
                if (hop192 % (p->upL * (kk + d)) == 0 && (p->upM * (kk + d)) % 8 == 0) { kk += d; break; }
            }
            p->upLin = p->upM * kk;
            p->upLout = p->upL * kk;
            const int al = p->up_alloc;
            bank.assign((size_t)(p->up_pc + 1) * al, 0.0f);
            amx::swr_bank(fs, kfs, bank.data());
            // resample_init's extra row pc: row 0 one tap later within the row (the
            // interpolation partner of the last phase)
            for (int i = 0; i < al; i++) bank[(size_t)p->up_pc * al + i] = bank[(i + al - 1) % al];
            // M == 1: the unrolled kernels (phase pattern static, phase 0 the identity)
            bool ident0 = p->up_taps == 32 && bank[15] == 1.0f;
            for (int i = 0; i < 32 && ident0; i++) ident0 = ident0 && (i == 15 || bank[i] == 0.0f);
            p->up_static = (p->upM == 1 && (p->upL == 1 || p->upL == 2 || p->upL == 4) && ident0 && !p->up_lin &&
                            p->upLin % 8 == 0) ? p->upL : 0;
        }
    } else {
        // already 192 kHz: ffmpeg inserts no resampler ahead of af_loudnorm, only the s16
        // -> dbl conversion x / 32768; a one-phase bank that is the unit impulse makes
        // k_ln_upsample produce exactly that (every other tap adds 0).  The measurement
        // takes the resampler path with that identity (L = M = 1, k_up<1>): one pass over
        // the samples -- K filter, peaks and the hop pieces' energy terms -- where the
        // native path (still taken by a rate loudnorm is refused on, above) ran the GEMV
        // and then the filter again (k_kw1 + k_kw2).
        bank.assign(32, 0.0f);
        bank[15] = 1.0f;
        p->resamp = 1;
        p->upL = p->upM = 1;
        p->up_pc = 1;
        p->up_taps = p->up_alloc = 32;
        p->up_src = p->up_dst = 1;
        p->up_lin = 0;
        p->upLin = p->upLout = 480;            // 40 K segments per 100 ms hop
        p->up_static = 1;
    }
    p->hop = (kfs + 5) / 10;                   // libebur128 samples_in_100ms at 192 kHz
    {
        const int chain_hop = (fs + 5) / 10;
        p->Lkw = 128 < chain_hop ? 128 : chain_hop / AMX_TF_FRAMES * AMX_TF_FRAMES;
    }
}

// ChainDev but for the K filter, the compressor and the envelope tables
int Builder::chain_coefficients() {
    ChainDev &cd = p->cd;
    memset(&cd, 0, sizeof cd);
    cd.fs = fs;
    // mono int16 is duplicated to stereo on the device first (k_pcm_to_s16), so the
    // chain reads stereo int16 frames
    p->mono16 = (desc->input_s16 && desc->channels_in == 1) ? 1 : 0;
    cd.chin = p->mono16 ? 2 : desc->channels_in;
    cd.in_s16 = desc->input_s16 ? 1 : 0;
    cd.analog_on = desc->analog_on ? 1 : 0;
    cd.has_lut = desc->tanh_lut ? 1 : 0;
    cd.drive = desc->analog_drive;
    for (int k = 0; k < 6; k++) {
        cd.an_lo[k] = desc->analog_lo_ba[k];
        cd.an_hi[k] = desc->analog_hi_ba[k];
    }
    cd.an_glo1 = desc->analog_lo_gain - 1.0;
    cd.an_ghi1 = desc->analog_hi_gain - 1.0;
    // EQ stages and the compact state model
    int mask = 0, D = 0;
    for (int s = 0; s < 4; s++) {
        int kind = desc->eq_kind[s];
        int want = (s == 0 || s == 3) ? 1 : 2;
        if (kind != 0 && kind != want)
            return fail(AMX_EINVAL, "eq stage %d: kind %d not supported at this position", s, kind);
        EqStageDev &st = cd.st[s];
        st.kind = kind;
        if (!kind) continue;
        mask |= 1 << s;
        D += kind == 1 ? 2 : 8;
        st.neg = desc->eq_gain_db[s] < 0 ? 1 : 0;
        st.g = desc->eq_gain[s];
        st.gm1 = desc->eq_gain[s] - 1.0;
        st.gf = (float)desc->eq_gain[s];
        for (int k = 0; k < 24; k++) st.c[k] = desc->eq_coef[s][k];
    }
    {   // compact register-resident coefficients (amx_dev.hpp eq_chain)
        int c = 0;
        for (int s = 0; s < 4; s++) {
            const EqStageDev &st = cd.st[s];
            if (!st.kind) continue;
            const double *k = st.c;
            int nsec = st.kind == 1 ? 1 : 4;
            for (int q = 0; q < nsec; q++) {
                cd.eqc[c++] = k[6 * q + 0];
                cd.eqc[c++] = k[6 * q + 1];
                cd.eqc[c++] = k[6 * q + 2];
                cd.eqc[c++] = k[6 * q + 4];
                cd.eqc[c++] = k[6 * q + 5];
            }
            if (st.kind == 2) cd.eqc[c++] = st.gm1;
            else if (!st.neg) cd.eqc[c++] = st.gm1;
            else {
                const bool first = (mask & ((1 << s) - 1)) == 0;   // stage sees the float32 column
                cd.eqc[c++] = first ? (double)st.gf : st.g;
            }
        }
    }
    cd.eq_mask = mask;
    cd.eq_dim = D;
    p->mask = mask;
    p->D = D;
    cd.width_on = desc->width_on ? 1 : 0;
    cd.width = desc->width;
    cd.mb_on = p->mb = desc->multiband_on ? 1 : 0;
    for (int k = 0; k < 12; k++) {
        cd.xlo[k] = desc->xover_lo_sos[k];
        cd.xhi[k] = desc->xover_hi_sos[k];
    }
    cd.look = (int32_t)(5.0 * (fs / 1000.0));
    // the detector's window must fit k_rms's largest prefix-sum tile (amx_dyn.hip)
    if (p->mb && cd.look > AMX_RMS_MAXLOOK)
        return fail(AMX_ERANGE, "multiband: the %d-frame detector window at %d Hz exceeds %d frames (rates up to %d Hz)",
                    cd.look, fs, AMX_RMS_MAXLOOK, AMX_RMS_MAXLOOK * 200);
    return AMX_OK;
}

// K-weighting coefficients (libebur128 ebur128_init_filter)
void Builder::kw_coefficients() {
    ChainDev &cd = p->cd;
    double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    double K = std::tan(M_PI * f0 / (double)kfs);
    double Vh = std::pow(10.0, G / 20.0);
    double Vb = std::pow(Vh, 0.4996667741545416);
    double pb[3] = {0.0, 0.0, 0.0}, pa[3] = {1.0, 0.0, 0.0};
    double rb[3] = {1.0, -2.0, 1.0}, ra[3] = {1.0, 0.0, 0.0};
    double a0 = 1.0 + K / Q + K * K;
    pb[0] = (Vh + Vb * K / Q + K * K) / a0;
    pb[1] = 2.0 * (K * K - Vh) / a0;
    pb[2] = (Vh - Vb * K / Q + K * K) / a0;
    pa[1] = 2.0 * (K * K - 1.0) / a0;
    pa[2] = (1.0 - K / Q + K * K) / a0;
    f0 = 38.13547087602444;
    Q = 0.5003270373238773;
    K = std::tan(M_PI * f0 / (double)kfs);
    ra[1] = 2.0 * (K * K - 1.0) / (1.0 + K / Q + K * K);
    ra[2] = (1.0 - K / Q + K * K) / (1.0 + K / Q + K * K);
    // libebur128 multiplies the two sections into one 4th-order direct form II;
    // its state (~1/(1-p)^2 ~ 1e5 x signal at 96 kHz) makes the A^L scan
    // ill-conditioned, so the GPU runs the same two sections as DF-II-T biquads.
    for (int k = 0; k < 3; k++) {
        cd.kw1[k] = pb[k];
        cd.kw1[3 + k] = pa[k];
        cd.kw2[k] = rb[k];
        cd.kw2[3 + k] = ra[k];
    }
    // the fused direct form itself, for the one place that runs libebur128's filter
    // sample by sample (loudnorm's r128_out, amx_ln_dyn.hip)
    p->kdf_b[0] = pb[0] * rb[0];
    p->kdf_b[1] = pb[0] * rb[1] + pb[1] * rb[0];
    p->kdf_b[2] = pb[0] * rb[2] + pb[1] * rb[1] + pb[2] * rb[0];
    p->kdf_b[3] = pb[1] * rb[2] + pb[2] * rb[1];
    p->kdf_b[4] = pb[2] * rb[2];
    p->kdf_a[0] = pa[0] * ra[0];
    p->kdf_a[1] = pa[0] * ra[1] + pa[1] * ra[0];
    p->kdf_a[2] = pa[0] * ra[2] + pa[1] * ra[1] + pa[2] * ra[0];
    p->kdf_a[3] = pa[1] * ra[2] + pa[2] * ra[1];
    p->kdf_a[4] = pa[2] * ra[2];
}

// compressor tables (pydub compress_dynamic_range, exact C math == CPython math)
int Builder::compressor_tables() {
    if (!p->mb) return AMX_OK;
    ChainDev &cd = p->cd;
    std::vector<double> &tabs = p->tabs;
    tabs.assign((size_t)3 * 3 * 32769, 0.0);
    const double A = 5.0 * (fs / 1000.0), R = 50.0 * (fs / 1000.0);
    for (int b = 0; b < 3; b++) {
        double thr = 32768.0 * std::pow(10.0, desc->comp_threshold_db[b] / 20.0);
        double ratio = desc->comp_ratio[b];
        if (ratio == 0.0) return fail(AMX_EINVAL, "compressor ratio must be non-zero");
        int rthr = 0;
        while (rthr <= 32768 && !((double)rthr > thr)) rthr++;
        cd.rthr[b] = rthr;
        double k = 1.0 - (1.0 / ratio);
        double ln10 = std::log(10.0);
        double *mt = &tabs[(size_t)b * 3 * 32769];
        for (int r = 0; r <= 32768; r++) {
            double m;
            if (desc->comp_m_table[b]) {
                m = desc->comp_m_table[b][r];
            } else {
                double over = 0.0;
                if (r != 0) {
                    double db = 20 * (std::log((double)r / thr) / ln10);
                    over = (0 > db) ? 0.0 : db;
                }
                m = k * over;
            }
            mt[r] = m;
            mt[32769 + r] = m / A;
            mt[2 * 32769 + r] = m / R;
        }
        int rq = 0;
        while (rq <= 32768 && mt[rq] == 0.0) rq++;
        cd.rq[b] = rq;
    }
    {
        static const double exc[16] = {
            0x1.a934f0979a371p+1, -0x1.34413509f79ffp-2, 0x1.9dc1da994fd21p-59,
            -0x1.f48ad494ea3e9p-53, 0x1.26bb1bbb55516p+1, 0x1.ade156a5dcb37p-26,
            0x1.28af3fca7ab0cp-22, 0x1.71dee623fde64p-19, 0x1.a01997c89e6b0p-16,
            0x1.a01a014761f6ep-13, 0x1.6c16c1852b7b0p-10, 0x1.1111111122322p-7,
            0x1.55555555502a1p-5, 0x1.5555555555511p-3, 0x1.000000000000bp-1, 0.05};
        for (int i = 0; i < 16; i++) cd.exc[i] = exc[i];
    }
    // the device forms m / A as q = m (1/A), q + (m - q A) (1/A) (two FMAs, exact
    // to the IEEE quotient by Markstein's theorem for a correctly rounded 1/A);
    // checked here for every m the tables can produce
    cd.env_A = A;
    cd.env_R = R;
    cd.env_rA = 1.0 / A;
    cd.env_rR = 1.0 / R;
    cd.env_rcp = 1;
    for (size_t i = 0; i < (size_t)3 * 3 * 32769 && cd.env_rcp; i += 1) {
        if (i % (3 * 32769) >= 32769) continue;
        const double m = tabs[i];
        const double qa = m * cd.env_rA, qr = m * cd.env_rR;
        const double ca = std::fma(std::fma(-qa, A, m), cd.env_rA, qa);
        const double cr = std::fma(std::fma(-qr, R, m), cd.env_rR, qr);
        if (ca != m / A || cr != m / R) cd.env_rcp = 0;
    }
    return AMX_OK;
}

int Builder::count_tracks() {
    int n_tracks = 0;
    for (int c = 0; c < n_chunks; c++) {
        if (chunks[c].frames < 0 || chunks[c].in_offset < 0 || chunks[c].track < 0)
            return fail(AMX_EINVAL, "chunk %d: negative field", c);
        if (c > 0 && chunks[c].track < chunks[c - 1].track)
            return fail(AMX_EINVAL, "chunks must be ordered by track");
        n_tracks = chunks[c].track + 1 > n_tracks ? chunks[c].track + 1 : n_tracks;
    }
    p->n_tracks = n_tracks;
    p->n_chunks = n_chunks;
    return AMX_OK;
}

// envelope segment sizing: Le per active-band count, k_env0's placement, the warm-up
void Builder::envelope_sizing() {
    if (!p->mb) return;
    // k_env0 runs one resident wave set: 2 waves per CU (one workgroup per CU), Le the
    // shortest multiple of 128 whose segments fit it, so no CU runs waves in turn and the
    // warm-up share W / Le shrinks as the job grows
    p->env_wg = 2;
    p->env_pin = 1;
    // segments per band: the waves of one band per CU, the CUs shared by the t bands that
    // are active (t = 3: every band, floor 1024 frames; the tables for 1 and 2 active
    // bands have shorter segments, floor 512)
    int64_t total = 0;
    for (int c = 0; c < n_chunks; c++) total += chunks[c].frames;
    for (int t = 3; t >= 1; t--) {
        const int64_t fit = (int64_t)(ncu / t) * 64 * p->env_wg;
        const int64_t lo = t == 3 ? 1024 : 512;
        int64_t Le = std::max<int64_t>(lo, (total / fit + 127) / 128 * 128);
        for (;; Le += 128) {
            int64_t ne = 0;
            for (int c = 0; c < n_chunks; c++) ne += (chunks[c].frames + Le - 1) / Le;
            if (ne <= fit || Le >= (int64_t)1 << 24) break;
        }
        p->Le_t[t] = (int)Le;
    }
    p->Le = p->Le_t[3];
    // the warm-up: since the fix-up re-runs broken segments in parallel (round 5), a
    // shorter warm-up pays where it is most of a lane's frames (C3: Le 1 408 / 896,
    // C4: 8.5 k); a 60-min track's long segments keep 2 304
    if (desc->env_warm_frames < 0 && p->Le_t[3] <= 16384) p->warm = 1536;
}

// chunks, their IIR segments and scan blocks, the spans' output ranges
int Builder::chunk_tables() {
    const int n_tracks = p->n_tracks;
    int64_t loc = 0, outo = 0;
    p->spans.assign(n_tracks, SpanDev{});
    std::vector<int> track_seen(n_tracks, 0);
    for (int c = 0; c < n_chunks; c++) {
        ChunkDev ch{};
        ch.in_off = chunks[c].in_offset;
        ch.loc_off = loc;
        ch.out_off = outo;
        ch.n = chunks[c].frames;
        int64_t n1 = ch.n, n2 = ch.n;
        if (p->mb && ch.n > 0) {
            n1 = overlay_len(ch.n, fs);
            n2 = overlay_len(n1, fs);
        }
        ch.out_n = n2;
        ch.track = chunks[c].track;
        p->in_frames = std::max(p->in_frames, (int64_t)(chunks[c].in_offset + chunks[c].frames));
        ch.seg0 = (int32_t)p->segs.size();
        int64_t ns = (ch.n + p->L - 1) / p->L;
        ch.nseg = (int32_t)ns;
        add_blocks(p->blks, ch.seg0, (int32_t)ns, c);
        for (int64_t k = 0; k < ns; k++) {
            SegDev s{};
            s.pos = k * p->L;
            s.chunk = c;
            s.len = (int32_t)((ch.n - s.pos) < p->L ? (ch.n - s.pos) : p->L);
            s.first = ch.seg0;
            s.last = (k == ns - 1) ? 1 : 0;
            p->segs.push_back(s);
        }
        SpanDev &sp = p->spans[ch.track];
        if (!track_seen[ch.track]) {
            sp.out_off = outo;
            track_seen[ch.track] = 1;
        }
        sp.out_n += n2;
        p->chunks.push_back(ch);
        p->n1tab.push_back(n1);
        p->max_chunk_out = n2 > p->max_chunk_out ? n2 : p->max_chunk_out;
        p->max_chunk_n = ch.n > p->max_chunk_n ? ch.n : p->max_chunk_n;
        p->an_blocks += (ch.n + 4095) / 4096;
        if (ch.n > 0 && ((ch.in_off & 1) != 0 || ch.n < 4)) p->an_vec = 0;
        loc += (ch.n + 15) / 16 * 16;   // chunk rows of per-frame scratch start 16-frame aligned
        outo += n2;
    }
    if (loc >= ((int64_t)1 << 31) || outo >= ((int64_t)1 << 31))
        // the chain kernels' row offsets are 32-bit (amx_chain.hip VRows)
        return fail(AMX_ERANGE, "a plan holds fewer than 2^31 frames (%lld): split the batch",
                    (long long)std::max(loc, outo));
    p->nloc = loc;
    p->out_frames = outo;
    p->n_seg = (int)p->segs.size();
    p->n_blk = (int)p->blks.size();
    return AMX_OK;
}

// envelope segment tables (ChainDev::etab): per table the chunks cut into Le_t-frame
// segments; segment indices (SegDev::first, eseg0) are table-relative
void Builder::envelope_tables() {
    if (!p->mb) return;
    int ld = 0;
    for (int t = 3; t >= 1; t--) {
        if (t < 3 && p->Le_t[t] == p->Le_t[3]) {
            p->cd.etab[t] = p->cd.etab[3];
            continue;
        }
        const int Le = p->Le_t[t];
        const int es_off = (int)p->esegs.size(), ch_off = (int)p->eseg0.size();
        for (int c = 0; c < n_chunks; c++) {
            const int64_t n = p->chunks[c].n;
            const int64_t ne = (n + Le - 1) / Le;
            p->eseg0.push_back((int)p->esegs.size() - es_off);
            p->neseg.push_back((int)ne);
            for (int64_t k = 0; k < ne; k++) {
                SegDev e{};
                e.pos = k * Le;
                e.chunk = c;
                e.len = (int32_t)((n - e.pos) < Le ? (n - e.pos) : Le);
                e.first = p->eseg0.back();
                e.last = (k == ne - 1) ? 1 : 0;
                p->esegs.push_back(e);
            }
        }
        const int n_es = (int)p->esegs.size() - es_off;
        p->cd.etab[t].es_off = es_off;
        p->cd.etab[t].n_es = n_es;
        p->cd.etab[t].ch_off = ch_off;
        p->cd.etab[t].Le = Le;
        ld = std::max(ld, n_es);
    }
    p->cd.etab[0] = p->cd.etab[3];
    p->cd.es_ld = ld;
    p->n_es = ld;
}

// K-weighting segments per track span, on the measurement stream: output j of
// the 192 kHz stream is made from the chain frames around floor(j M / L); a span
// of chain frames [f0, f0 + n) of its track owns outputs [J(f0), J(f0 + n)),
// J(f) = ceil(f L / M); segment q = chain frames f0 + q Lin + [0, Lin) = outputs
// J(f0) + q Lout + [0, Lout)
int Builder::k_segments() {
    const int64_t uL = p->upL, uM = p->upM, uS = p->up_src, uD = p->up_dst, uP = p->up_pc;
    auto J = [&](int64_t f) { return (f * uL + uM - 1) / uM; };
    // (J(f0) dst - f0 pc src): the phase pattern -- output J(f0)'s position past frame f0
    // in units of 1 / (pc src) frame (exact rates: (J(f0) M - f0 L) src) -- equal for all spans
    for (int t = 0; t < p->n_tracks; t++) {
        SpanDev &sp = p->spans[t];
        sp.tframe0 = track_frame0 ? track_frame0[t] : 0;
        sp.ttotal = track_total_frames ? track_total_frames[t] : sp.out_n;
        sp.kseg0 = (int32_t)p->ksegs.size();
        const int Lseg = p->resamp ? p->upLout : p->Lkw;
        const int Lsin = p->resamp ? p->upLin : p->Lkw;
        if (p->resamp && p->up_ok) {
            sp.m_tframe0 = J(sp.tframe0);
            sp.m_n = J(sp.tframe0 + sp.out_n) - sp.m_tframe0;
            sp.m_total = J(sp.ttotal);
            const int64_t pat = sp.m_tframe0 * uD - sp.tframe0 * uP * uS;
            if (sp.out_n > 0) {
                if (pattern >= 0 && pat != pattern)
                    return fail(AMX_EINVAL, "spans with different 192 kHz phase patterns in one plan");
                pattern = pat;
            }
        } else {
            sp.m_tframe0 = sp.tframe0;
            sp.m_n = sp.out_n;
            sp.m_total = sp.ttotal;
        }
        sp.edge_lo = sp.tframe0 > 0 ? 1 : 0;
        sp.edge_hi = sp.tframe0 + sp.out_n < sp.ttotal ? 1 : 0;
        int64_t nk = (p->resamp && !p->up_ok) ? 0 : (sp.m_n + Lseg - 1) / Lseg;
        sp.nkseg = (int32_t)nk;
        add_blocks(p->kblks, sp.kseg0, (int32_t)nk, t);
        for (int64_t k = 0; k < nk; k++) {
            KwSegDev s{};
            s.out_pos = sp.out_off + k * Lsin;
            s.tframe = sp.m_tframe0 + k * Lseg;
            s.track = t;
            s.len = (int32_t)((sp.m_n - k * Lseg) < Lseg ? (sp.m_n - k * Lseg) : Lseg);
            s.first = sp.kseg0;
            s.last = (k == nk - 1) ? 1 : 0;
            p->ksegs.push_back(s);
        }
        p->max_span = sp.out_n > p->max_span ? sp.out_n : p->max_span;
        p->max_nkseg = sp.nkseg > p->max_nkseg ? sp.nkseg : p->max_nkseg;
        p->max_hops = std::max(p->max_hops, sp.m_total / p->hop + 1);
        p->any_empty_span |= sp.nkseg == 0 ? 1 : 0;
    }
    p->n_kseg = (int)p->ksegs.size();
    p->n_kblk = (int)p->kblks.size();
    // hop splits on 16-frame tile boundaries (k_kw2 picks the hop piece per tile)
    p->kw_aligned = (!p->resamp && p->hop % AMX_TF_FRAMES == 0 && p->Lkw % AMX_TF_FRAMES == 0) ? 1 : 0;
    for (int t = 0; t < p->n_tracks; t++)
        if (p->spans[t].tframe0 % AMX_TF_FRAMES) p->kw_aligned = 0;
    // the K-filter segment grid equals the chain's when there is no multiband
    // (output frames == input frames) and every chunk but a span's last is whole
    // segments long: k_front2 then does loudness pass 1 on the output it writes
    p->fuse_kw = (!p->resamp && !p->mb && p->Lkw == p->L && p->n_kseg == p->n_seg && !desc->measure_only &&
                  !p->sc) ? 1 : 0;
    for (int c = 0; c < n_chunks && p->fuse_kw; c++) {
        const bool span_last = (c == n_chunks - 1) || (chunks[c + 1].track != chunks[c].track);
        if (!span_last && (p->chunks[c].n % p->L) != 0) p->fuse_kw = 0;
    }
    return AMX_OK;
}

// resampler phase tables: per output n of a segment the chain frame its window is
// centred on (relative to the segment's first frame) and its phase; k_up_poly's form
void Builder::resampler_phases() {
    if (!(p->resamp && p->up_ok)) return;
    const int64_t uS = p->up_src, uD = p->up_dst, uP = p->up_pc;
    std::vector<int32_t> &obase = p->obase, &oph = p->oph, &fcnt = p->fcnt;
    if (pattern < 0) pattern = 0;
    obase.resize(p->upLout);
    oph.resize(p->upLout);
    p->owt.resize(p->upLout);
    const float inv = 1.0f / (float)uS;          // the float reciprocal resample.asm forms
    for (int64_t n = 0; n < p->upLout; n++) {
        const int64_t pos = pattern + n * uD;     // (J0 + n) dst - f0 pc src
        const int64_t idx = pos / uS;
        obase[n] = (int32_t)(idx / uP);
        oph[n] = (int32_t)(idx % uP);
        p->owt[n] = (float)(pos % uS) * inv;
    }
    if (p->up_static && pattern != 0) p->up_static = 0;
    if (!p->up_static && !p->up_lin && p->up_taps == 32) {
        // k_up_poly: frame f of a segment is the base of the outputs n with obase[n]
        // == f (consecutive n; every frame has one when L >= M); the form is (min,
        // max count, a block of TB frames dividing Lin)
        fcnt.assign((size_t)p->upLin, 0);
        bool ok = p->upL >= p->upM;
        for (int64_t n = 0; n < p->upLout && ok; n++) {
            ok = obase[n] >= 0 && obase[n] < p->upLin && (n == 0 || obase[n] >= obase[n - 1]);
            if (ok) fcnt[obase[n]]++;
        }
        int cmin = 1 << 30, cmax = 0;
        for (int32_t c : fcnt) { cmin = std::min(cmin, c); cmax = std::max(cmax, c); }
        const int tb = p->upLin % 8 == 0 ? 8 : (p->upLin % 7 == 0 ? 7 : 0);
        if (ok && cmin >= 1 && tb) p->up_poly = amx::up_poly_form(cmin, cmax, tb);
        if (!knobs.up_poly) p->up_poly = 0;       // (AMX_UP_POLY=0)
        if (p->up_poly) {
            p->bankn.resize((size_t)p->upLout * 32);
            for (int64_t n = 0; n < p->upLout; n++)
                for (int k = 0; k < 32; k++) p->bankn[(size_t)n * 32 + k] = p->bank[(size_t)oph[n] * 32 + k];
        }
    }
}

// the segments the unrolled 192 kHz kernel leaves to the general one: windows that
// reach past the span's frames, partial segments, segments holding a hop boundary
// (the same test as up_fast_seg in amx_loud192.hip)
void Builder::slow_list() {
    if (!(p->resamp && p->up_ok)) return;
    if (p->up_static || p->up_poly) {
        for (int32_t j = 0; j < p->n_kseg; j++) {
            const KwSegDev &sg = p->ksegs[j];
            const SpanDev &sp = p->spans[sg.track];
            const int64_t g0 = sg.out_pos - sp.out_off;
            const int64_t split = (sg.tframe / p->hop + 1) * p->hop - sg.tframe;
            const bool fast = g0 - 15 >= 0 && g0 + p->upLin + 17 <= sp.out_n &&
                              sg.len == p->upLout && split >= p->upLout;
            if (!fast) p->slow.push_back(j);
        }
        p->n_slow = (int64_t)p->slow.size();
    } else {
        p->n_slow = p->n_kseg;       // every segment, no list
    }
}

// the three LTI models: GEMV rows, A^L and the block scan's window powers
int Builder::lti_models() {
    const ChainDev &cd = p->cd;
    const double tol = 1e-22;
    if (p->D > 0) {
        Lti eq;
        eq.derive(p->D, [&](LD *z, LD x) {
            int o = 0;
            for (int s = 0; s < 4; s++) {
                const EqStageDev &st = cd.st[s];
                if (st.kind == 1) {
                    shelf_step_h(st.c, z + o, x, st.neg, st.gm1);
                    o += 2;
                } else if (st.kind == 2) {
                    LD b = x;
                    for (int k = 0; k < 4; k++) b = sos_step_h(st.c + 6 * k, z + o + 2 * k, b);
                    x = x + b * (LD)st.gm1;
                    o += 8;
                }
            }
        });
        p->G = eq.gemv_table(p->L);
        p->M = eq.pow(p->L);
        p->lev_eq = eq.window_powers((int64_t)p->L * AMX_SCAN_S, tol, 16, p->Mp);
        if (p->lev_eq < 0)
            return fail(AMX_ERANGE, "EQ decays too slowly for %d-frame segments; raise seg_frames", p->L);
    }
    if (p->mb) {
        Lti xo;
        xo.derive(AMX_XO_DIM, [&](LD *z, LD x) {
            LD l = sos_step_h(cd.xlo, z, x);
            sos_step_h(cd.xlo + 6, z + 2, l);
            LD h = sos_step_h(cd.xhi, z + 4, x);
            sos_step_h(cd.xhi + 6, z + 6, h);
        });
        p->Gx = xo.gemv_table(p->L);
        p->Mx = xo.pow(p->L);
        p->lev_x = xo.window_powers((int64_t)p->L * AMX_SCAN_S, tol, 16, p->Mpx);
        if (p->lev_x < 0) return fail(AMX_ERANGE, "crossover decays too slowly for %d-frame segments", p->L);
    }
    // The int16 sample enters the GEMVs as q 2^-15.  With the rows scaled by 2^-15 the
    // kernels feed (double)q: fma(g 2^-15, q, acc) and fma(g, q 2^-15, acc) round the
    // same real number, as long as g 2^-15 is g's exact multiple -- it is unless it
    // falls below the normal range.  k_front2 reads Gx scaled here; k_gemv16 scales the
    // EQ rows (G, which the float32 front kernels read unscaled) as it stages them, so
    // both tables are checked, and one entry that would be subnormal keeps the
    // unscaled rows and the q / 32768 input for both (gin_scaled = 0).
    p->gin_scaled = scale_gemv_rows(p->G, p->Gx) ? 1 : 0;
    Lti &kw = p->kw_model;
    kw.derive(AMX_KW_DIM, [&](LD *z, LD x) {
        LD y = sos_step_h(cd.kw1, z, x);
        sos_step_h(cd.kw2, z + 2, y);
    });
    const int Lseg = p->resamp ? std::max(1, p->upLout) : p->Lkw;
    if (p->resamp) {
        // the measurement kernels keep no GEMV table: their pass over the samples
        // runs the filter from rest and needs the free-response rows C A^n and
        // their Gram sums (amx_loud192.hip k_up / k_up_energy)
        std::vector<double> &Gkw = p->Gkw, &qh = p->qh, &qt = p->qt;
        LD Cr[AMX_KW_DIM];
        for (int k = 0; k < AMX_KW_DIM; k++) {
            LD z[AMX_KW_DIM] = {0.0L, 0.0L, 0.0L, 0.0L};
            z[k] = 1.0L;
            const LD y1 = sos_step_h(cd.kw1, z, 0.0L);
            Cr[k] = sos_step_h(cd.kw2, z + 2, y1);
        }
        Gkw.assign((size_t)Lseg * AMX_KW_DIM, 0.0);
        qh.assign((size_t)(Lseg + 1) * 16, 0.0);
        qt.assign((size_t)(Lseg + 1) * 16, 0.0);
        std::vector<LD> r(Cr, Cr + AMX_KW_DIM), t(AMX_KW_DIM), gl((size_t)Lseg * AMX_KW_DIM);
        std::vector<LD> qa(16, 0.0L);
        for (int n = 0; n < Lseg; n++) {
            for (int d = 0; d < AMX_KW_DIM; d++) {
                gl[(size_t)n * AMX_KW_DIM + d] = r[d];
                Gkw[(size_t)n * AMX_KW_DIM + d] = (double)r[d];
            }
            for (int u = 0; u < 4; u++)
                for (int w = 0; w < 4; w++) {
                    qa[u * 4 + w] += r[u] * r[w];
                    qh[(size_t)(n + 1) * 16 + u * 4 + w] = (double)qa[u * 4 + w];
                }
            for (int d = 0; d < AMX_KW_DIM; d++) {     // r <- r A
                LD acc = 0.0L;
                for (int k = 0; k < AMX_KW_DIM; k++) acc += r[k] * kw.A[(size_t)k * AMX_KW_DIM + d];
                t[d] = acc;
            }
            r = t;
        }
        std::fill(qa.begin(), qa.end(), 0.0L);
        for (int n = Lseg - 1; n >= 0; n--) {
            const LD *g = &gl[(size_t)n * AMX_KW_DIM];
            for (int u = 0; u < 4; u++)
                for (int w = 0; w < 4; w++) {
                    qa[u * 4 + w] += g[u] * g[w];
                    qt[(size_t)n * 16 + u * 4 + w] = (double)qa[u * 4 + w];
                }
        }
    } else {
        p->Gkw = kw.gemv_table(Lseg);
    }
    p->Mkw = kw.pow(Lseg);
    // up to 32 block powers: a track measured at its own 192 kHz rate (loudnorm's
    // output) needs ~20 with 128-frame segments (the 38 Hz pole)
    p->lev_kw = kw.window_powers((int64_t)Lseg * AMX_SCAN_S, tol, 32, p->Mpkw);
    if (p->lev_kw < 0) return fail(AMX_ERANGE, "K-weighting decays too slowly for %d-frame segments", Lseg);
    p->tail_pow.assign((size_t)p->n_tracks * 16, 0.0);
    for (int t = 0; t < p->n_tracks; t++) {
        const SpanDev &sp = p->spans[t];
        if (sp.nkseg == 0) continue;
        int len_last = p->ksegs[sp.kseg0 + sp.nkseg - 1].len;
        Mat P = kw.pow(len_last);
        for (int k = 0; k < 16; k++) p->tail_pow[(size_t)t * 16 + k] = P[k];
    }
    return AMX_OK;
}

// histogram boundaries (libebur128 init_histogram)
void Builder::histogram_tables() {
    std::vector<double> &bounds = p->bounds, &energies = p->energies;
    bounds.resize(1001);
    energies.resize(1000);
    bounds[0] = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    for (int i = 1; i < 1001; ++i) bounds[i] = std::pow(10.0, ((double)i / 10.0 - 70.0 + 0.691) / 10.0);
    for (int i = 0; i < 1000; ++i) energies[i] = std::pow(10.0, ((double)i / 10.0 - 69.95 + 0.691) / 10.0);
}

// pass 1's form for the analog stage, and the odd tanh table's half
void Builder::tanh_half() {
    if (!(desc->tanh_lut && desc->analog_on)) return;
    // numpy's float32 tanh is odd: lut[32768 - k] == -lut[32768 + k] bit for bit (sign
    // of zero included) for every k; then tanh(s) = sign(s) * half[|s|] with half[k] =
    // lut[32768 + k] and half[32768] = -lut[0].  Checked per table: any pair that
    // differs keeps the full table in global memory (k_front1s).
    bool odd = true;
    for (int k = 1; k < 32768 && odd; k++) {
        uint32_t lo, hi;
        memcpy(&lo, &desc->tanh_lut[32768 - k], 4);
        memcpy(&hi, &desc->tanh_lut[32768 + k], 4);
        odd = lo == (hi ^ 0x80000000u);
    }
    p->f1_mode = knobs.f1;
    if (!odd) p->f1_mode = AMX_F1_FULL;
    if (p->f1_mode == AMX_F1_SPLIT) {
        std::vector<float> &half = p->lut_half;
        half.resize(32769);
        for (int k = 0; k < 32768; k++) half[k] = desc->tanh_lut[32768 + k];
        half[32768] = -desc->tanh_lut[0];
    }
}

void Builder::workspace_layout() {
    const int D = p->D;
    size_t off = 0;
    const size_t nseg = (size_t)p->n_seg, nl = (size_t)p->nloc, nk = (size_t)p->n_kseg;
    p->o_a16 = align_up(off, nl * 4);
    p->o_e = align_up(off, nseg * 2 * (D ? D : 1) * 8);
    p->o_s = align_up(off, nseg * 2 * (D ? D : 1) * 8);
    if (p->mb) {
        p->o_p16 = align_up(off, nl * 4);
        p->o_ex = align_up(off, nseg * 2 * AMX_XO_DIM * 8);
        p->o_sx = align_up(off, nseg * 2 * AMX_XO_DIM * 8);
        p->o_bands = align_up(off, 3 * nl * 4);
        const size_t ne = (size_t)p->n_es;
        p->o_gain = align_up(off, (3 * nl / 16 + 64) * 8);   // envelope checkpoints
        // m rows are read whole-tile by k_env0, from W frames before a chunk to the
        // 16-frame tile past its end: pad the buffer on both sides
        // (and k_gain_overlay reads whole 1024-frame wave tiles)
        // (k_env0's last tiles of a chunk-final segment read up to Le frames past it)
        const size_t mpad = (size_t)std::max(std::max(p->warm, p->Le), 1024) + 64;
        p->o_m = align_up(off, (3 * nl + 2 * mpad) * 2) + mpad * 2;   // u16 r
        p->o_esv = align_up(off, 3 * ne * 8);
        p->o_ee0 = align_up(off, 3 * ne * 8);
        p->o_eflags = align_up(off, (AMX_ENV_LIST + 3) * 4);   // + band words, list lengths, flag
        p->o_eact = align_up(off, 3 * ne * 4);
        p->o_ehead = align_up(off, 3 * ne * 4);   // chain-head marks
        p->o_elist = align_up(off, 3 * ne * 4);   // chain-head list
        p->o_eprev = align_up(off, 3 * ne * 4);   // nearest earlier active segment
        p->o_elist0 = align_up(off, 3 * ne * 4);  // the optimistic re-run list
    }
    if (p->mono16) p->o_dup = align_up(off, (size_t)p->in_frames * 4);
    const size_t nb = (size_t)p->n_blk, nkb = (size_t)p->n_kblk;
    p->o_eb = align_up(off, nb * 2 * (D ? D : 1) * 8);
    if (p->mb) {
        p->o_ebx = align_up(off, nb * 2 * AMX_XO_DIM * 8);
    }
    p->o_ebk = align_up(off, nkb * 2 * AMX_KW_DIM * 8);
    p->o_ekw = align_up(off, nk * 2 * AMX_KW_DIM * 8);
    p->o_pk = align_up(off, nk * 4 * 4);
    p->o_skw = align_up(off, nk * 2 * AMX_KW_DIM * 8);
    p->o_parts = align_up(off, nk * 4 * 8);
    if (p->resamp) p->o_eterms = align_up(off, nk * 2 * 10 * 8);
    p->o_phop = align_up(off, nk * 8);
    p->ws_bytes = (off + 255) & ~(size_t)255;
}

}  // namespace

int build_plan_host(const amx_chain_desc *desc, const amx_chunk *chunks, int32_t n_chunks,
                    const int64_t *track_frame0, const int64_t *track_total_frames, int32_t seg_frames,
                    const PlanKnobs &knobs, int ncu, PlanHost &h, std::string &err) {
    Builder b{&h, desc, chunks, n_chunks, track_frame0, track_total_frames, knobs, ncu, err};
    PlanHost *p = &h;
    int rc = b.check_arguments();
    if (rc) return rc;
    p->desc = *desc;
    p->sc = desc->stream_chain ? 1 : 0;
    b.fs = desc->sample_rate;
    if (desc->env_warm_frames >= 0) p->warm = (desc->env_warm_frames + 127) / 128 * 128;   // whole ring of k_env0 tiles
    if (desc->env_rounds >= 0) p->rounds = desc->env_rounds;
    if (p->rounds > AMX_ENV_MAX_ROUNDS)
        return b.fail(AMX_EINVAL, "env_rounds %d > %d", desc->env_rounds, AMX_ENV_MAX_ROUNDS);
    p->L = seg_frames > 0 ? seg_frames : 256;
    p->L = (p->L + AMX_TF_FRAMES - 1) / AMX_TF_FRAMES * AMX_TF_FRAMES;   // whole LDS tiles
    b.measurement_stream();
    if ((rc = b.chain_coefficients()) != AMX_OK) return rc;
    b.kw_coefficients();
    if ((rc = b.compressor_tables()) != AMX_OK) return rc;
    if ((rc = b.count_tracks()) != AMX_OK) return rc;
    b.envelope_sizing();
    if ((rc = b.chunk_tables()) != AMX_OK) return rc;
    b.envelope_tables();
    if ((rc = b.k_segments()) != AMX_OK) return rc;
    b.resampler_phases();
    b.slow_list();
    if ((rc = b.lti_models()) != AMX_OK) return rc;
    b.histogram_tables();
    b.tanh_half();
    b.workspace_layout();
    return AMX_OK;
}

}  // namespace amx
