"""CPU-only: the host side of the wide GEMM's tile choice and of eg_gemm_nt_batch.  Every check here happens before any launch,
so the (fake, never dereferenced) pointers need no device."""
import ctypes as C

import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd._lib import GemmDesc, rowmap

FAKE = 0x10000


def desc(M=2048, K=256, dtype=L.EG_BF16, **kw):
    d = GemmDesc()
    d.A, d.W, d.C = FAKE, FAKE, FAKE
    d.a, d.c = rowmap(K), rowmap(256)
    d.r, d.p = d.c, d.c
    d.M, d.N, d.K, d.ldw, d.dtype = M, 256, K, K, dtype
    d.gate_scale = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def batch(*ds):
    arr = (GemmDesc * len(ds))()
    for i, d in enumerate(ds):
        arr[i] = d
    return arr


def test_tile_rule_prefers_fewer_rounds_then_fewer_bytes():
    rows = L.lib().eg_gemm_wide_rows
    assert rows(32768, 256) == 128       # 256 workgroups: one whole round (205 on 160 rows, with more bytes each)
    assert rows(33280, 256) == 160       # 208 workgroups, one round; 260 on 128 rows would be two
    assert rows(35840, 256) == 160       # 224 against 280
    assert rows(131072, 256) == 128      # 1024 = four whole rounds; 820 on 160 rows is four as well, with more bytes each
    assert rows(128, 256) == 128 and rows(0, 256) == 0
    assert rows(160 * 304, 304) == 160   # one round on a 304-CU part; 380 workgroups of 128 rows would be two


def test_batch_refuses_null_and_a_count_out_of_range():
    with pytest.raises(L.EgError, match="null descriptors"):
        L.call("eg_gemm_nt_batch", None, 1, 0)
    for n in (0, -1, L.GEMM_BATCH_MAX + 1):
        with pytest.raises(L.EgError, match="outside"):
            L.call("eg_gemm_nt_batch", batch(*[desc()] * 9), n, 0)
        assert L.lib().eg_gemm_nt_batch_route(batch(*[desc()] * 9), n) == -1
    with pytest.raises(L.EgError, match="null operand"):
        L.call("eg_gemm_nt_batch", batch(desc(), GemmDesc()), 2, 0)


def test_batch_refuses_mixed_dtype_and_mixed_epilogue():
    with pytest.raises(L.EgError, match="dtype"):
        L.call("eg_gemm_nt_batch", batch(desc(), desc(dtype=L.EG_F16)), 2, 0)
    for other in (desc(act=L.ACT_RELU), desc(gate=FAKE), desc(residual=FAKE), desc(bias=FAKE), desc(out_pre=FAKE),
                  desc(drop1_p=0.1, state=FAKE)):
        with pytest.raises(L.EgError, match="epilogue"):
            L.call("eg_gemm_nt_batch", batch(desc(), other), 2, 0)
        assert L.lib().eg_gemm_nt_batch_route(batch(desc(), other), 2) == -1


def test_batch_route_is_one_grid_only_when_every_product_fits_the_wide_kernel():
    route = L.lib().eg_gemm_nt_batch_route
    assert route(batch(desc(M=32768, K=1792), desc(M=32768, K=1536, gate_scale=1.25)), 2) == 1
    assert route(batch(desc()), 1) == 1 and route(batch(*[desc()] * 8), 8) == 1
    assert route(batch(desc(), desc(K=64)), 2) == 0              # below the wide kernel's K floor
    assert route(batch(desc(), desc(M=512)), 2) == 0             # below its row floor
    assert route(batch(desc(), desc(A=FAKE + 8)), 2) == -1       # eg_gemm_nt's own alignment check
    f32 = [desc(dtype=L.EG_F32), desc(dtype=L.EG_F32)]
    assert route(batch(*f32), 2) == 0                            # fp32 products: single launches
    try:
        L.call("eg_gemm_wide_config", -1, 1)
        assert route(batch(desc(), desc(M=512)), 2) == 1
        with pytest.raises(L.EgError, match="tile_rows"):
            L.call("eg_gemm_wide_config", 96, -1)
    finally:
        L.call("eg_gemm_wide_config", -1, 1024)
