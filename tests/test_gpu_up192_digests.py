"""The 192 kHz measurement pass and the wide / interpolating loudnorm upsamplers bit for bit:
every case of tests/up192_cases.py gives the digests recorded in
tests/golden/up192_digests.json, which was written by the kernels before the resampler
helpers were shared and k_up_edge / k_up_wide merged (the file names the commit).  The
oracle comparisons (test_gpu_parity.py, test_gpu_dynamic.py) allow a histogram count of 2
or 3 LSB; this one allows nothing.  That each case's plan takes the path it is there for
(static_l, poly, the slow list, lin, taps) is asserted for the same rates and lengths on the
CPU, by tests/test_plan_build.py::test_up192_cases_run_the_paths_they_are_there_for."""
import json
import os

import numpy as np
import pytest

import up192_cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "up192_digests.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(up192_cases.CASES)


@pytest.mark.parametrize("name", up192_cases.CASES)
def test_digest(gpu, name):
    out = up192_cases.run_case(name)
    if name in up192_cases.LN:
        y, s = out
        print("%s: %d frames, summary[0..1] %r %r" % (name, y.shape[0], s[0], s[1]))
        assert y.shape[0] == 480000 and np.any(y != 0)      # 2.5 s at 192 kHz
    else:
        hops, peak, tail = out
        pl = up192_cases.PLANS[name]
        print("%s: hop energies > 0: %d, peaks %r" % (name, int((hops > 0).sum()), peak.tolist()))
        # three whole hops and a piece of the fourth, both channels, on every track
        assert hops.shape[0] == len(pl["spans"]) and all(int((h > 0).sum()) == 8 for h in hops), hops.shape
        assert np.all(peak > 0) and np.all(np.isfinite(tail)) and np.any(tail != 0)
    assert up192_cases.digest(name, out) == GOLDEN[name]
