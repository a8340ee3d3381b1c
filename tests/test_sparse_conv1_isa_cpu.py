"""Resource audit of the sparse first convolution's kernels (no GPU needed: hipcc cross-compiles for gfx950): the gather-GEMM
keeps 64 accumulator registers and two operand sets per lane; a spill would put private-memory traffic into its MFMA loop."""
import os

import pytest

from test_head_deferred_isa_cpu import HIPCC, kernel_usage


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sparse_conv1_kernels_use_no_scratch():
    k = {n: u for n, u in kernel_usage("sparse_conv1.hip").items() if "sc1_" in n}
    print(k)
    assert len(k) == 4  # ballot, write, and the gather-GEMM in the K order of either dense chunk size
    assert sum("sc1_gather" in n for n in k) == 2
    for n, u in k.items():
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
        if "sc1_gather" in n:
            assert int(u["Occupancy [waves/SIMD]"]) >= 2, (n, u)  # waves work alone: latency is hidden by the wave next door
