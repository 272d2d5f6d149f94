"""The eight-wave causal scans at 64 < D <= 128 (fastmax_mfma_bf16.hip, fastmax_mfma_d128_2p.hip, fastmax_scan_d128_2p.hip)
held to the bits they gave before csrc/fastmax_scan128.h took over what they share."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _parity():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import scan128_parity
    return scan128_parity


@pytest.mark.parametrize("name", list(_parity().CASES))
def test_scan128_kernels_give_the_recorded_bits(name):
    """tests/golden/scan128_parity.json: digests of the output and of every gradient (tools/scan128_parity.py), no tolerance.
    The kernels have no atomics, and every case reproduced its own digests when it was recorded.  The plan query names the
    kernel each case is there to pin, and the number of sequence segments that makes it reach the seeded-state path."""
    parity = _parity()
    fwd, bwd, nseg = parity.CASES[name][3:]
    assert parity.planned(name) == (fwd, bwd, nseg)
    with open(parity.GOLDEN) as f:
        want = json.load(f)[name]
    assert parity.run_case(name) == want
