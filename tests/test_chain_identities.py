"""CPU: the bit identities the chain's segment kernels rest on (amx_chain.hip, amx_dev.hpp).

The kernels keep the reference's arithmetic order; what they changed around it is claimed
to give the same bits by construction.  Each claim is checked here in IEEE arithmetic on the
host (g++ -ffp-contract=off, no fast-math), bit for bit:

* width: both lanes of a channel pair run ``width_mix`` on lane-signed operands and clip;
  the test compiles the text of ``width_frame``, ``width_sign``, ``width_mix`` and
  ``width_self`` taken from amx_dev.hpp itself, runs the two lanes as k_front2 does (own sample, the other
  lane's, and their lane-signed copies) and compares the clipped pair with width_frame's
  on edge values (signed zeros, denormals, values that clip, the largest
  finite floats' neighbourhood excluded only where the reference itself overflows) crossed
  with each other, and on random pairs; and that the clip is idempotent (the kernel clips
  once, in the int16 conversion);
* GEMV input: (double)((float)q / 32768.0f) == q 2^-15 for every int16 q, and
  fma(g 2^-15, q, acc) == fma(g, q 2^-15, acc) on 10^6 random (g, q, acc) plus the extreme
  q, for g whose scaled value is normal (what the plan checks before it scales the rows);
* int16 conversion: the clipped value times 32767 converted to int is its own int16
  narrowing (the kernels keep the int);
* the plan's switch for the scaled rows (``scale_gemv_rows``, amx_plan_build.cpp).

Not covered here: the kernel does not call ``width_self`` but ``width_lane``, which feeds the
same ``width_mix`` from two ``pair_add`` sums -- a hand-written ``v_add_f32_dpp`` (inline
asm, with its own wait states) that cannot run on the host.  That ``pair_add(a, x)`` is
``a + (the other lane's x)``, and so ``width_lane`` equals ``width_self``, is pinned only on
the GPU (tests/test_gpu_chain_small_segments.py and the width cases of
tests/test_gpu_eq_masks.py, bit for bit against the oracle).
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = os.path.join(os.path.dirname(HERE), "audio-mastering-engine_amd", "csrc", "amx_dev.hpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")

PRELUDE = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#define __device__
#define __forceinline__ inline
// v_med3_f32 on non-NaN operands: the median
static inline float med3_host(float a, float b, float c) {
    return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c));
}
#define __builtin_amdgcn_fmed3f med3_host
static inline int __float_as_int(float v) { int u; memcpy(&u, &v, 4); return u; }
static inline float __int_as_float(int u) { float v; memcpy(&v, &u, 4); return v; }
"""

MAIN = r"""
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static float fb(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

static long width_case(float w, float l, float r, long &bad) {
    float a = l, b = r;
    width_frame(w, a, b);
    if (!std::isfinite(a) || !std::isfinite(b)) return 0;   // the reference overflowed
    // the two lanes of k_front2 (width_lane): own and other sample and their lane-signed
    // copies (what the DPP sums bring from the other lane)
    const float el = width_sign(l, 0), er = width_sign(r, 1);
    const float nl = med3_host(width_self(w, 0, l, r, el, er), -1.0f, 1.0f);
    const float nr = med3_host(width_self(w, 1, r, l, er, el), -1.0f, 1.0f);
    if (bits(nl) != bits(a) || bits(nr) != bits(b)) {
        if (bad++ < 10) printf("width w=%a l=%a r=%a: %a %a want %a %a\n", w, l, r, nl, nr, a, b);
    }
    if (bits(med3_host(nl, -1.0f, 1.0f)) != bits(nl)) bad++;   // clip idempotent
    return 1;
}

int main() {
    long bad = 0, n = 0;
    // ---- width
    std::vector<float> edge = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -0.5f, 0.99999994f, 1.0000001f, -1.0000001f,
                               2.0f, -3.5f, 1e-38f, -1e-38f, fb(1), fb(0x80000001u), fb(0x007fffffu),
                               fb(0x807fffffu), fb(0x00800000u), fb(0x80800000u), 1.1754944e-38f,
                               3.0517578e-05f, -3.0517578e-05f, 0.33333334f, -0.7f, 1e10f, -1e10f,
                               1.5e38f, -1.5e38f, 3.0e38f};
    const float ws[] = {1.3f, 0.7f, 0.0f, 1.0f, 2.0f, 0.5f, 1e-30f, fb(3), 100.0f};
    for (float w : ws)
        for (float l : edge)
            for (float r : edge) n += width_case(w, l, r, bad);
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<float> u11(-1.0f, 1.0f), uw(0.0f, 2.0f), ubig(-4.0f, 4.0f);
    for (int i = 0; i < 1000000; i++) {
        const bool big = (i & 7) == 0;
        float l = big ? ubig(rng) : u11(rng), r = big ? ubig(rng) : u11(rng);
        if ((i & 63) == 1) r = l;
        if ((i & 63) == 2) r = -l;
        if ((i & 63) == 3) l = fb((uint32_t)rng() & 0x807fffffu);      // a denormal (or zero)
        n += width_case((i & 1) ? 1.3f : uw(rng), l, r, bad);
    }
    printf("width cases %ld\n", n);
    // ---- the int16 sample as a GEMV / filter input
    for (int q = -32768; q <= 32767; q++) {
        const double a = (double)((float)(int16_t)q / 32768.0f), b = (double)q * 0x1p-15;
        if (bits(a) != bits(b)) bad++;
    }
    // ---- the scaled-row FMA
    long nf = 0;
    auto fma_case = [&](double g, int q, double acc) {
        const double gs = g * 0x1p-15;
        if (!(gs == 0.0 || std::fabs(gs) >= 0x1p-1022)) return;      // the plan's condition
        const double a = std::fma(gs, (double)q, acc);
        const double b = std::fma(g, (double)((float)q / 32768.0f), acc);
        if (bits(a) != bits(b)) {
            if (bad++ < 10) printf("fma g=%a q=%d acc=%a: %a want %a\n", g, q, acc, a, b);
        }
        nf++;
    };
    std::uniform_int_distribution<int> uq(-32768, 32767), ue(-1000, 60), ua(-1060, 40);
    std::uniform_real_distribution<double> um(1.0, 2.0);
    const int qx[] = {-32768, -32767, 32767, 32766, -1, 0, 1};
    for (int i = 0; i < 1000000; i++) {
        double g = std::ldexp(um(rng), ue(rng)) * ((rng() & 1) ? 1.0 : -1.0);
        double acc = std::ldexp(um(rng), ua(rng)) * ((rng() & 1) ? 1.0 : -1.0);
        if ((i & 31) == 0) acc = 0.0;
        if ((i & 31) == 1) acc = -0.0;
        if ((i & 31) == 2) g = std::ldexp(um(rng), -1007);            // the smallest the plan scales
        if ((i & 31) == 3) acc = -g * (double)uq(rng) * 0x1p-15;      // near cancellation
        fma_case(g, uq(rng), acc);
    }
    for (int q : qx)
        for (int i = 0; i < 20000; i++)
            fma_case(std::ldexp(um(rng), ue(rng)) * ((rng() & 1) ? 1.0 : -1.0), q,
                     (i & 3) ? std::ldexp(um(rng), ua(rng)) * ((rng() & 1) ? 1.0 : -1.0) : 0.0);
    printf("fma cases %ld\n", nf);
    // ---- the int16 conversion keeps its int: |clip(x) * 32767| <= 32767
    const float fe[] = {1.0f, -1.0f, 0.99999994f, -0.99999994f, 0.0f, -0.0f, 3.0517578e-05f, 0.5f};
    for (float v : fe) {
        const int q = (int)(med3_host(v, -1.0f, 1.0f) * 32767.0f);
        if (q != (int)(int16_t)q) bad++;
        const double dv = (double)v;
        const int qd = (int)(std::fmax(std::fmin(dv, 1.0), -1.0) * 32767.0);
        if (qd != (int)(int16_t)qd) bad++;
    }
    printf("bad %ld\n", bad);
    return bad ? 1 : 0;
}
"""


def _function(text, name):
    """the source text of one `__device__ __forceinline__` function of the header"""
    m = re.search(r"__device__ __forceinline__ \w+ %s\(.*?\n}\n" % name, text, re.S)
    assert m, name
    return m.group(0)


@pytest.fixture(scope="module")
def identities(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_identities")
    with open(DEV) as f:
        dev = f.read()
    src = PRELUDE + "".join(_function(dev, n) for n in ("width_frame", "width_sign", "width_mix", "width_self")) + MAIN
    (d / "ident.cpp").write_text(src)
    exe = str(d / "ident")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", str(d / "ident.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_width_lanes_equal_width_frame(identities):
    out = identities.stdout
    assert "width " not in out.replace("width cases", ""), out
    n = int(re.search(r"width cases (\d+)", out).group(1))
    assert n > 1000000, out          # the edge grid and the random pairs were compared


def test_scaled_rows_and_int_input(identities):
    out = identities.stdout
    assert "fma g=" not in out, out
    assert int(re.search(r"fma cases (\d+)", out).group(1)) > 1000000, out
    assert identities.returncode == 0 and "bad 0" in out, out


def test_plan_scales_rows_only_when_exact(tmp_path):
    """scale_gemv_rows (amx_plan_build.cpp), which sets the plan's gin_scaled: ordinary
    tables are scaled by 2^-15 and reported scaled; one entry of either table whose scaled
    value would be subnormal leaves both untouched and reports the unscaled input path"""
    csrc = os.path.dirname(DEV)
    (tmp_path / "rows.cpp").write_text(r"""
#include "amx_plan_build.hpp"
#include <cstdio>
int main() {
    using V = std::vector<double>;
    int bad = 0;
    V G = {1.0, -0x1p-1007, 0.0, -0.0, 3.5}, Gx = {0.25, -0x1.8p-1007, 0.0, 0x1p+20};
    const V Gx0 = Gx;
    if (!amx::scale_gemv_rows(G, Gx)) bad |= 1;
    for (size_t i = 0; i < Gx.size(); i++) if (Gx[i] != Gx0[i] * 0x1p-15) bad |= 2;
    if (Gx[1] != -0x1.8p-1022) bad |= 4;                       // the smallest scaled: normal, exact
    V Gy = {0.25, 0x1.fffffffffffffp-1008, 1.0};               // just below: would be subnormal
    const V Gy0 = Gy;
    if (amx::scale_gemv_rows(G, Gy) || Gy != Gy0) bad |= 8;
    V Gt = {1.0, 0x1p-1074}, Gz = {0.5, 2.0};                   // a tiny entry of G alone
    const V Gz0 = Gz;
    if (amx::scale_gemv_rows(Gt, Gz) || Gz != Gz0) bad |= 16;
    V Ge, Gn;                                                  // no EQ, no crossover
    if (!amx::scale_gemv_rows(Ge, Gn)) bad |= 32;
    printf("bad %d\n", bad);
    return bad;
}
""")
    exe = str(tmp_path / "rows")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", csrc, "-I", os.path.join(os.path.dirname(HERE), "include"),
                        str(tmp_path / "rows.cpp"), os.path.join(csrc, "amx_plan_build.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", r.stdout + r.stderr
