"""Plan construction on the CPU (no GPU): tables, invariants, ownership.

amx_plan_create is a host-only builder (csrc/amx_plan_build.cpp) and an upload step
(csrc/amx_plan.cpp).  tests/plan/plan_harness.cpp links both against host stand-ins for the
few HIP runtime calls they make (tests/plan/hip_standin.cpp: "device" memory is malloc'd)
and is built as a program of its own with g++ -fsanitize=address,undefined, leak
detection on.  Over its case list (every measurement rate form, multiband sizing on few
and many CUs, every knob, EQ / input / chunk shapes, every error exit, 3..8 channels) it

* prints amx_plan_info, the track spans, the host scalars, the workspace offsets and a
  digest of every integer table as uploaded; tests/golden/plan_build.txt holds that output
  recorded from the single-function amx_plan_create this split replaced (only values that
  do not depend on libm: floating tables are pinned by size and finiteness);
* checks the tables' invariants on the uploaded copies (segments, blocks, envelope tables
  and K segments tile their ranges, the slow list is exactly the segments that fail the
  fast test, the workspace regions are aligned and disjoint, ...);
* fails every allocation of a plan in turn, and the re-allocating entry points
  (amx_limiter_prepare, amx_kw_carry_setup), under LeakSanitizer.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "audio-mastering-engine_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def harness_exe(tmp_path_factory):
    """the harness, built with the library's floating-point flags plus the sanitizers (the
    kernel launchers stay unresolved: nothing launches)"""
    exe = str(tmp_path_factory.mktemp("plan") / "plan_harness")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-D__HIP_PLATFORM_AMD__",
                        "-I" + ROCM_INC, "-I" + CSRC,
                        os.path.join(HERE, "plan", "plan_harness.cpp"), os.path.join(HERE, "plan", "hip_standin.cpp"),
                        os.path.join(CSRC, "amx_plan.cpp"), os.path.join(CSRC, "amx_plan_build.cpp"),
                        "-Wl,--unresolved-symbols=ignore-all", "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime for the host compiler: %s" % r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def harness_output(harness_exe):
    """the harness run once over all cases"""
    r = subprocess.run([harness_exe], capture_output=True, text=True, env=ENV, timeout=600)
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and \
        "runtime error" not in r.stderr, r.stderr[-6000:]
    return r


def _cases(text):
    """{case name: its lines}, and the lines after the last case (the ownership runs)"""
    cases, name = {}, None
    for line in text.splitlines():
        if line.startswith("case "):
            name = line[5:]
            cases[name] = []
        elif line.startswith("own ") or re.fullmatch(r"\d+ failed", line):
            name = None
            cases.setdefault(None, []).append(line)
        else:
            cases[name].append(line)
    return cases


def test_tables_equal_the_recorded_plan(harness_output):
    """return codes, error texts, amx_plan_info, spans, host scalars, workspace offsets,
    integer-table digests, floating-table sizes: line for line what the unsplit
    amx_plan_create gave"""
    with open(os.path.join(HERE, "golden", "plan_build.txt")) as f:
        want = _cases(f.read())
    got = _cases(harness_output.stdout)
    assert sorted(k for k in got if k) == sorted(k for k in want if k)
    assert len([k for k in want if k]) == 87      # a truncated golden would pass the loop below
    for name in want:
        assert got[name] == want[name], name


def test_multiband_refused_above_204800_hz(harness_output):
    """the compressor's detector window (5 ms) must fit k_rms's largest tile (1024 frames):
    352.8 and 384 kHz with multiband fail at plan construction with AMX_ERANGE and a message
    naming the limit -- in the host-only builder, where nothing can have been launched --
    and the same rates without multiband build"""
    got = _cases(harness_output.stdout)
    for fs, look in ((352800, 1764), (384000, 1920)):
        lines = got["mb_%d" % fs]
        assert len(lines) == 1 and lines[0].startswith("rc=-4 err=multiband: the %d-frame" % look), lines
        assert "1024 frames" in lines[0] and "204800 Hz" in lines[0], lines
        assert got["rate_%d" % fs][0] == "rc=0 err=" and got["rate_%d" % fs][-1].endswith("inv ok")
    assert got["mb_192000"][0] == "rc=0 err="


def test_invariants_hold(harness_output):
    got = _cases(harness_output.stdout)
    plans = 0
    for name, lines in got.items():
        assert not any("FAIL" in ln for ln in lines), (name, [ln for ln in lines if "FAIL" in ln])
        if name and "rc=0 err=" in lines:
            n = sum(ln.endswith("inv ok") for ln in lines)
            assert n == (sum(ln.startswith(("pa.info", "pb.info", "pc.info")) for ln in lines) or 1), name
            plans += n
    assert plans == 60


def test_ownership_under_leak_sanitizer(harness_output):
    """every allocation failure returns AMX_EHIP with *out NULL and nothing leaked, a
    failed amx_limiter_prepare keeps the earlier scratch, and the whole run (create / free
    of every case, the re-allocating entry points, 3..8-channel plans) ends without a
    LeakSanitizer or AddressSanitizer report"""
    tail = _cases(harness_output.stdout)[None]
    assert any(ln.startswith("own allocation failures: ") and "each failed once" in ln for ln in tail), tail
    assert "own done" in tail and tail[-1] == "0 failed", tail
    assert harness_output.returncode == 0, harness_output.stderr[-3000:]


def test_builder_compiles_without_hip(tmp_path):
    """amx_plan_build.cpp alone, plain g++, no ROCm include path"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", os.path.join(CSRC, "amx_plan_build.cpp"),
                        "-o", str(tmp_path / "amx_plan_build.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope="module")
def up192_plans(harness_exe):
    """the plan of every measurement case of tests/up192_cases.py (the harness's --plan)"""
    import up192_cases
    args = []
    for name, pl in up192_cases.PLANS.items():
        args += ["--plan", name, str(pl["fs"]), ",".join(str(n) for n in pl["spans"]),
                 str(pl["f0"][0]) if pl["f0"] else "-", str(pl["total"][0]) if pl["total"] else "-",
                 ",".join("%s=%s" % kv for kv in pl["env"].items()) or "-"]
    r = subprocess.run([harness_exe] + args, capture_output=True, text=True, env=ENV, timeout=600)
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and \
        "runtime error" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, r.stdout[-3000:]
    return _cases(r.stdout)


def _host(lines):
    line = [ln for ln in lines if ln.startswith("host ")][0]
    return dict(kv.split("=") for kv in line.split()[1:])


def test_up192_cases_run_the_paths_they_are_there_for(up192_plans):
    """tests/test_gpu_up192_digests.py's cases, rate for rate and length for length: the
    unrolled k_up<L> with chunked left-overs, the five k_up_poly forms with left-overs on the
    side stream, k_up_slow over every segment (with and without interpolation) and the wave
    kernel over every segment of a downsampling rate; each with fast segments and left-overs
    where the path has both"""
    import up192_cases
    assert sorted(k for k in up192_plans if k) == sorted(up192_cases.PLANS)
    for name, pl in up192_cases.PLANS.items():
        lines = up192_plans[name]
        assert lines[0] == "rc=0 err=" and "inv ok" in lines, (name, lines[:1])
        h = _host(lines)
        print(name, {k: h[k] for k in ("up", "Lin", "Lout", "static", "lin", "taps", "poly", "nslow", "kseg")})
        nslow, kseg = int(h["nslow"]), int(h["kseg"])
        assert int(h["resamp"]) == 1 and int(h["ok"]) == 1, name
        assert int(h["static"]) == pl["static_l"] and int(h["poly"]) == pl["poly"] and int(h["lin"]) == pl["lin"], (name, h)
        assert (h["taps"] != "32/32") == pl["wide"], (name, h)
        if pl["all_slow"]:
            assert nslow == kseg and "int slow -" in lines, (name, h)
        else:
            # a span's first (mirrored or neighbour-fed) and last (partial) segments, the
            # hop-split ones where the segment does not divide the hop; the rest fast
            assert 2 * len(pl["spans"]) <= nslow < kseg - 3 and "int slow -" not in lines, (name, h)
        if pl["static_l"]:
            # (launch_up1: the left-overs are k_up's first workgroups while Lin + 32 <= 544)
            assert int(h["Lin"]) + 32 <= 544, (name, h)


def test_every_resampler_bank_row_has_a_positive_tap(up192_plans):
    """the dot products' first term is a product, not fma(w, h, +0) (csrc/amx_swr_dev.hpp): the
    two differ only when a whole row's products are zeros of negative sign, which the
    positive main-lobe tap of every row rules out for inputs without a -0"""
    for name, lines in up192_plans.items():
        if name is None:
            continue
        bank = [ln for ln in lines if ln.startswith("bank ")]
        assert len(bank) == 1 and bank[0].endswith(" without_positive_tap=0"), (name, bank)
        assert int(bank[0].split()[1].split("=")[1]) >= 1, (name, bank)
