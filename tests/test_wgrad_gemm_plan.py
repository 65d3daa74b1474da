"""Host-only plan of the implicit-GEMM weight gradient (tb_conv3d_wgrad_gemm_config / _ws_bytes, no GPU): tiles by
channel count, slices that never straddle a sample and cover it, a workspace that holds every slice's partial
tile, and the shapes the entry declines."""
import ctypes

import pytest

from texbias import conv as C
from texbias._lib import lib

# G shape, X shape, stride, ksize: the six deep layers of the C3 step, then partial tiles and a short reduction
LAYERS = [((2, 256, 15, 15, 10), (2, 64, 30, 30, 20), 2, 3), ((2, 128, 15, 15, 10), (2, 128, 15, 15, 10), 1, 3),
          ((2, 256, 15, 15, 10), (2, 128, 15, 15, 10), 1, 3), ((2, 256, 15, 15, 10), (2, 256, 15, 15, 10), 1, 3),
          ((2, 256, 15, 15, 10), (2, 128, 15, 15, 10), 1, 1), ((2, 384, 15, 15, 10), (2, 64, 30, 30, 20), 2, 3),
          ((2, 40, 5, 7, 6), (2, 24, 5, 7, 6), 1, 3), ((1, 256, 3, 3, 2), (1, 256, 3, 3, 2), 1, 3),
          ((3, 70, 9, 9, 9), (3, 130, 9, 9, 9), 1, 3)]


@pytest.mark.parametrize("g,x,s,k", LAYERS)
def test_plan_covers_the_reduction(g, x, s, k):
    for sps in (0, 1, 5, 1000):
        cfg = C.wgrad_gemm_config(g, x, s, k, sps)
        n, m, c = g[0], g[1], x[1]
        q = g[2] * g[3] * g[4]
        assert cfg["BM"] == (64 if m <= 64 else 128) and cfg["BP"] == (64 if c <= 64 else 128)
        assert cfg["nsplit"] % n == 0 and cfg["kper"] % 32 == 0
        per_sample = cfg["nsplit"] // n
        assert per_sample * cfg["kper"] >= q                      # the slices cover a sample
        assert (per_sample - 1) * cfg["kper"] < q                 # and none is empty
        tiles = -(-m // cfg["BM"]) * -(-c // cfg["BP"]) * k ** 3
        assert cfg["blocks"] == tiles * cfg["nsplit"]
        ws = C._wgg_ws_bytes(n, m, c, *g[2:], *x[2:], s, k, sps)
        assert ws >= 4 * cfg["nsplit"] * m * c * k ** 3
        if sps == 1:
            assert cfg["nsplit"] == n


def test_unplanned_split_matches_the_plain_entry():
    cfg, cfg0 = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    a = (2, 256, 256, 15, 15, 10, 15, 15, 10, 1, 3)
    assert lib().tb_conv3d_wgrad_gemm_config(*a, cfg) == 0 and lib().tb_conv3d_wgrad_gemm_config_ex(*a, 0, cfg0) == 0
    assert list(cfg) == list(cfg0)
    assert lib().tb_conv3d_wgrad_gemm_ws_bytes(*a) == lib().tb_conv3d_wgrad_gemm_ws_bytes_ex(*a, 0) > 0


@pytest.mark.parametrize("g,x,s,k", [((1, 8, 4, 4, 4), (1, 8, 4, 4, 4), 2, 1), ((1, 8, 4, 4, 4), (1, 8, 8, 8, 8), 3, 3),
                                     ((1, 8, 4, 4, 4), (1, 8, 4, 4, 4), 1, 5), ((1, 8, 128, 128, 128), (1, 8, 128, 128, 128), 1, 3),
                                     ((64, 512, 30, 30, 20), (64, 512, 30, 30, 20), 1, 3), ((0, 8, 4, 4, 4), (0, 8, 4, 4, 4), 1, 3)])
def test_declined_shapes_have_no_plan_and_no_workspace(g, x, s, k):
    assert C.wgrad_gemm_config(g, x, s, k) is None
    assert C._wgg_ws_bytes(g[0], g[1], x[1], *g[2:], *x[2:], s, k, 0) == 0
    # the entry refuses before it touches a pointer or launches
    rc = lib().tb_conv3d_wgrad_gemm_f32(1, 0, 1, 0, 1, g[0], g[1], x[1], *g[2:], *x[2:], s, k, None, 0, None)
    assert rc in (1, 2)
