/* lim_guess_model.c -- af_alimiter's recurrence as oracle/amx_oracle.c states it (alimiter_core),
 * with the state kept in a struct so that two runs can be compared: the general limiter's
 * speculation (csrc/amx_final.hip, limiter_block) on the host.  For every segment boundary of a
 * span it builds the guess the kernel would build (lim_warm_start's start frame, IDLE there, the
 * ring filled from the input, the warm-up run) and compares it with the true state the way the
 * walker does: scalars, then the live list.  It also runs the `d <= delta` variant beside the
 * true run and compares the attenuation traces.  scripts/lim_guess_sweep.py drives it. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
typedef struct { double att, delta; int pos, nextiter, nextlen; double *buffer, *nextdelta; int *nextpos; } St;
typedef struct { int fs, bs; double level_in, limit, release; int le; } P;
static void st_new(St *s, int bs) { s->buffer = calloc(bs + 4, 8); s->nextdelta = calloc(bs + 4, 8); s->nextpos = malloc(4 * (bs + 4)); }
static void st_idle(St *s, int bs) { s->att = 1; s->delta = 0; s->pos = 0; s->nextiter = 0; s->nextlen = 0;
    for (int i = 0; i < bs + 4; i++) { s->buffer[i] = 0; s->nextdelta[i] = 0; s->nextpos[i] = -1; } }
static double smp(const P *p, int16_t v) { return ((double)v * (1.0 / 32768.0)) * p->level_in; }
static double step(St *s, const P *p, const int16_t *src) {
    const int channels = 2, buffer_size = p->bs; int pos = s->pos; double limit = p->limit;
    double peak = 0;
    for (int c = 0; c < 2; c++) { double sample = smp(p, src[c]); s->buffer[pos + c] = sample; peak = fmax(peak, fabs(sample)); }
    if (peak > limit) {
        double patt = fmin(limit / peak, 1.);
        double rdelta = (1.0 - patt) / (p->fs * p->release);
        double d = (limit / peak - s->att) / buffer_size * channels;
        int found = 0, i;
        if (p->le ? d <= s->delta : d < s->delta) {
            s->delta = d; s->nextpos[0] = pos; s->nextpos[1] = -1; s->nextdelta[0] = rdelta; s->nextlen = 1; s->nextiter = 0;
        } else {
            for (i = s->nextiter; i < s->nextiter + s->nextlen; i++) {
                int j = i % buffer_size; double ppeak = 0, pdelta;
                for (int c = 0; c < 2; c++) ppeak = fmax(ppeak, fabs(s->buffer[s->nextpos[j] + c]));
                pdelta = (limit / peak - limit / ppeak) / (((buffer_size - s->nextpos[j] + pos) % buffer_size) / channels);
                if (pdelta < s->nextdelta[j]) { s->nextdelta[j] = pdelta; found = 1; break; }
            }
            if (found) {
                s->nextlen = i - s->nextiter + 1;
                s->nextpos[(s->nextiter + s->nextlen) % buffer_size] = pos;
                s->nextdelta[(s->nextiter + s->nextlen) % buffer_size] = rdelta;
                s->nextpos[(s->nextiter + s->nextlen + 1) % buffer_size] = -1;
                s->nextlen++;
            }
        }
    }
    double *buf = &s->buffer[(pos + channels) % buffer_size];
    peak = 0; for (int c = 0; c < 2; c++) peak = fmax(peak, fabs(buf[c]));
    s->att += s->delta; double used = s->att;
    if ((pos + channels) % buffer_size == s->nextpos[s->nextiter]) {
        s->delta = s->nextdelta[s->nextiter]; s->att = limit / peak; s->nextlen -= 1;
        s->nextpos[s->nextiter] = -1; s->nextiter = (s->nextiter + 1) % buffer_size;
    }
    if (s->att > 1.) { s->att = 1.; s->delta = 0.; s->nextiter = 0; s->nextlen = 0; s->nextpos[0] = -1; }
    if (s->att <= 0.) { s->att = 0.0000000000001; s->delta = (1.0 - s->att) / (p->fs * p->release); }
    if (s->att != 1. && (1. - s->att) < 0.0000000000001) s->att = 1.;
    if (s->delta != 0. && fabs(s->delta) < 0.00000000000001) s->delta = 0.;
    s->pos = (pos + channels) % buffer_size;
    return used;
}
static int over(const P *p, const int16_t *x, int64_t i) { return fmax(fabs(smp(p, x[2*i])), fabs(smp(p, x[2*i+1]))) > p->limit; }
static int64_t warm_start(const P *p, const int16_t *x, int64_t seg0, int64_t R, int64_t cap) {
    int64_t w0 = seg0, floor_ = seg0 - cap, b = w0;
    for (;;) {
        if (w0 <= 0) return 0;
        if (w0 <= floor_) return w0;
        if (b <= w0 - R || b <= 0) return w0;
        int64_t last = -1;
        for (int l = 0; l < 64; l++) { int64_t i = b - 64 + l; if (i >= 0 && i >= w0 - R && over(p, x, i)) last = i; }
        if (last >= 0) { w0 = last; b = w0; } else b -= 64;
    }
}
/* out: [0] boundaries with a speculative guess, [1] scalars differ, [2] scalars equal lists differ, [3] all equal,
   [4] frames where the d<=delta variant's att trace differs, [5] frames with d == delta exactly (entering peaks) */
int sweep(const int16_t *x, int64_t n, int fs, double level_in, double limit, double attack_ms, double release_ms,
          int LS, int W, int64_t *out) {
    P p; p.fs = fs; p.level_in = level_in; p.limit = limit; p.release = release_ms / 1000.0; p.le = 0;
    int bs = (int)(fs * (attack_ms / 1000.0) * 2); bs -= bs % 2; p.bs = bs; int h = bs / 2 - 1;
    St t, g, v; st_new(&t, bs); st_new(&g, bs); st_new(&v, bs); st_idle(&t, bs); st_idle(&v, bs);
    P pv = p; pv.le = 1;
    memset(out, 0, 8 * 6);
    int64_t cap = W > 0 ? (int64_t)fs * 10 : 0;
    for (int64_t f = 0; f < n; f++) {
        if (f > 0 && f % LS == 0) {
            int64_t w0 = warm_start(&p, x, f, W, cap);
            if (w0 > 0) {
                st_idle(&g, bs);
                for (int64_t q = w0 - h < 0 ? 0 : w0 - h; q < w0; q++) { int r = (int)((2 * q) % bs); g.buffer[r] = smp(&p, x[2*q]); g.buffer[r+1] = smp(&p, x[2*q+1]); }
                g.pos = (int)((2 * w0) % bs);
                for (int64_t q = w0; q < f; q++) step(&g, &p, x + 2 * q);
                out[0]++;
                if (!(g.att == t.att && g.delta == t.delta && g.nextiter == t.nextiter && g.nextlen == t.nextlen)) out[1]++;
                else {
                    int ok = 1;
                    for (int i = 0; i <= t.nextlen; i++) { int j = (t.nextiter + i) % bs;
                        if (t.nextpos[j] != g.nextpos[j] || (i < t.nextlen && t.nextdelta[j] != g.nextdelta[j])) ok = 0; }
                    out[ok ? 3 : 2]++;
                }
            }
        }
        /* d == delta on an entering peak, seen in the true run */
        { double pk = fmax(fabs(smp(&p, x[2*f])), fabs(smp(&p, x[2*f+1])));
          if (pk > limit && (limit / pk - t.att) / bs * 2 == t.delta) out[5]++; }
        double a = step(&t, &p, x + 2 * f), b = step(&v, &pv, x + 2 * f);
        if (memcmp(&a, &b, 8)) out[4]++;
    }
    return 0;
}
int trace(const int16_t *x, int64_t n, int fs, double level_in, double limit, double attack_ms, double release_ms, double *att) {
    P p; p.fs = fs; p.level_in = level_in; p.limit = limit; p.release = release_ms / 1000.0; p.le = 0;
    int bs = (int)(fs * (attack_ms / 1000.0) * 2); bs -= bs % 2; p.bs = bs;
    St t; st_new(&t, bs); st_idle(&t, bs);
    for (int64_t f = 0; f < n; f++) att[f] = step(&t, &p, x + 2 * f);
    return 0;
}
