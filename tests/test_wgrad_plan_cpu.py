"""The weight-gradient host planners against a table recorded from the commit before they were folded into one
route record, one segment search and one launcher (tests/golden/wgrad_plans.json.gz, JSON with one row per shape,
gzipped; no GPU: without a device the planners size their grids for 256 compute units, the MI355X count the table
was recorded with).

Each row holds a shape (N, M, Cc, Do, Ho, Wo, Di, Hi, Wi, stride, pad) and what the library answered for it:
tb_conv3d_wgrad_ws_bytes, tb_conv3d_wgrad_bias_ws_bytes with its sums_bias flag, the return code and five values
of tb_conv3d_wgrad_config, and the return code and eight values of tb_conv3d_wgrad_plan (taken from the earlier
planners through the same dozen lines of query).  The shapes are the five C3 layers of tests/test_conv_tiling.py,
every shape of tests/test_gpu_conv.py and tests/test_gpu_wgrad_zf1.py, and a sweep over N in {1, 2}, D in
{1, 3, 5, 28, 80}, H in {3, 10, 41}, W in {4, 8, 17, 20, 40, 44, 80, 84, 100, 128, 130, 160, 240, 256, 260} at
stride 1, stride 2 with an input of exactly twice the output and stride 2 with one odd input extent, each
geometry with three (M, Cc) pairs drawn from {1, 3, 5, 6, 8, 16, 24, 32, 40, 64}.

4107 rows by plan kind: 1794 general kernel (kind 0), 224 zm (1), 162 zm2 (2), 226 zf1 (3), 254 zf2 (4) and
1447 without a plan (rows too wide for any tiling: the query returns an error code)."""
import ctypes
import gzip
import json
import os
from collections import Counter

import pytest

from texbias._lib import lib

COUNTS = {0: 1794, 1: 224, 2: 162, 3: 226, 4: 254, "none": 1447}


@pytest.fixture(scope="module")
def table():
    with gzip.open(os.path.join(os.path.dirname(__file__), "golden", "wgrad_plans.json.gz"), "rt") as f:
        t = json.load(f)
    assert t["columns"][:11] == ["N", "M", "Cc", "Do", "Ho", "Wo", "Di", "Hi", "Wi", "stride", "pad"]
    assert t["columns"][11:] == ["ws_bytes", "bias_ws_bytes", "sums_bias", "config_rc", "SEG", "TX", "YB", "chunks",
                                 "lds_bytes", "plan_rc", "kind", "plan_YB", "zlen", "ZS", "grid_x", "grid_y",
                                 "plan_lds_bytes", "plan_ws_bytes"]
    return t["rows"]


def test_table_covers_every_route(table):
    kinds = Counter("none" if r[20] else r[21] for r in table)
    assert dict(kinds) == COUNTS


def _answers(shape):
    L = lib()
    sums = ctypes.c_int(-1)
    ws = int(L.tb_conv3d_wgrad_ws_bytes(*shape))
    bws = int(L.tb_conv3d_wgrad_bias_ws_bytes(*shape, ctypes.byref(sums)))
    cfg = (ctypes.c_int64 * 5)()
    rc = int(L.tb_conv3d_wgrad_config(*shape, cfg))
    plan = (ctypes.c_int64 * 8)()
    prc = int(L.tb_conv3d_wgrad_plan(*shape, plan))
    return [ws, bws, sums.value, rc] + list(cfg) + [prc] + list(plan)


def test_every_row_is_reproduced(table):
    bad = [(r[:11], r[11:], got) for r in table for got in [_answers(r[:11])] if got != r[11:]]
    assert not bad, f"{len(bad)} of {len(table)} rows differ; first (shape, recorded, now): {bad[0]}"


def test_plan_wrapper_matches_the_row(table):
    """conv.wgrad_plan returns the same eight values by name."""
    from texbias import conv as C
    for r in table[:64]:
        if r[20] == 0:
            p = C.wgrad_plan((r[0], r[1]) + tuple(r[3:6]), (r[0], r[2]) + tuple(r[6:9]), r[9], r[10])
            assert list(p.values()) == r[21:] and list(p)[:4] == ["kind", "YB", "zlen", "ZS"]
