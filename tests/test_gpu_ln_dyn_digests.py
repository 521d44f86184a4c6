"""k_ln_dyn<C> bit for bit: every case of tests/ln_dyn_cases.py gives the output (and summary
words 0-1) recorded in tests/golden/ln_dyn_digests.json, which was written by the two
kernels this one replaced (the stereo k_ln_dyn and k_ln_dyn_mc<C>; the file names the
commit).  The oracle comparisons (test_gpu_dynamic.py, test_gpu_mc_dynamic.py) allow 3 LSB;
this one allows nothing."""
import json
import os

import pytest

import ln_dyn_cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_dyn_digests.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(ln_dyn_cases.CASES)


@pytest.mark.parametrize("name", ln_dyn_cases.CASES)
def test_digest(gpu, name):
    y, s = ln_dyn_cases.run_case(name)
    print("%s: %d frames, summary[0..1] %r %r, r128_out cycles %d, segments %d, hand-over frame %d" %
          (name, y.shape[0], s[0], s[1], s[7], s[12], s[14]))
    # the case runs the path it is there for
    if name in ("never_lifts", "partial_441", "first_burst"):
        # frame by frame to the end, above_threshold 0 and r128_out on every frame
        assert s[0] == 0 and s[1] == 0 and s[12] == 0 and s[7] > 0, s
    if name == "partial_441":
        assert y.shape[0] % 19200 != 0
    if name in ("linear_2s", "c3_2s.pass1", "c3_2s.pass2"):
        assert s[0] == 1.0, s
    if name == "handover":
        assert s[14] > 0, s
    if name.startswith("c6_quiet"):
        assert s[7] > 0, s
    assert ln_dyn_cases.digest(y, s) == GOLDEN[name]
