"""bnb_mi355x_gemm_int8_route: the host-side answer to "which int8 kernel runs" (no GPU)."""
import os
import re

import pytest

import bitsandbytes_amd as bnb
from bitsandbytes_amd import cextension as ce
from conftest import ROOT

INT8, TALL = 13, 14


def test_route_query_is_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "bnb_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"^int bnb_mi355x_gemm_int8_route\(long M, long N, long K\);", header, flags=re.M)
    assert hasattr(bnb.lib, "bnb_mi355x_gemm_int8_route") and "bnb_mi355x_gemm_int8_route" in ce.EXPORTED_SYMBOLS


@pytest.mark.parametrize("cus", [32, 256])
def test_route_under_knobs_cu_counts_and_refused_k(cus):
    route = bnb.lib.bnb_mi355x_gemm_int8_route
    try:
        bnb.lib.bnb_mi355x_set_cu_count(cus)
        for value, kernel in ((6000, INT8), (6100, TALL), (6200, TALL), (6300, TALL)):
            bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, value)
            assert [route(M, 4096, 4096) for M in (1, 64, 4096)] == [kernel] * 3
            assert route(64, 4096, 24) == 0 and route(64, 4096, 131072) == 0
        bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, 0)
        assert route(1, 4096, 4096) == INT8 and route(2048, 4096, 4096) == TALL
        assert route(64, 4096, 24) == 0 and route(64, 4096, 131072) == 0
    finally:
        bnb.lib.bnb_mi355x_set_tuning(0, 0, 0, 0)
        bnb.lib.bnb_mi355x_set_cu_count(0)
