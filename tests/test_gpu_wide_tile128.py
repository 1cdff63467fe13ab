"""The wide GEMM's 128-row tile and the batched launch (csrc/widegemm.hip).

Every tile runs the same k-ordered MFMA chain per output element and the same epilogue order, so eg_gemm_nt must give the SAME
BYTES on the 128 x 256 tile, the 160 x 256 tile and the 128 x 128 tiled kernel (eg_gemm_wide_config forces the tile, or raises
the wide kernel's row floor out of reach so that the tiled kernel serves the call), and eg_gemm_nt_batch the bytes of its
products launched one by one.  Shapes: M below one tile, ragged over three tiles, several tiles plus a 16-row rest; K of two,
three (the ring wraps once) and seven K steps.  C sits between sentinel rows, and the row-mapped cases leave sentinel gaps
between the rows they write; whole buffers are compared, gaps and guards included."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import GemmDesc, call, ptr, rowmap  # noqa: E402
from tests.test_gpu_ops import dev_state  # noqa: E402

DEV = "cuda"
N = 256
GUARD = 8                       # sentinel rows before and after every output
SENT = 7.0
SHAPES = [(M, K) for M in (128, 300, 1024 + 16) for K in (128, 192, 448)]
TDT = {"bf16": (torch.bfloat16, L.EG_BF16), "fp16": (torch.float16, L.EG_F16)}
# name -> epilogue switches
EPILOGUES = {
    "bias_relu": dict(bias=1, act=1),
    "gate_scale": dict(gate=1, gate_scale=1.25),
    "residual": dict(bias=1, residual=1),
    "out_pre_drop1": dict(bias=1, out_pre=1, residual=1, drop1=(0.1, 11)),
    "drop_both_sites": dict(bias=1, act=1, out_pre=1, residual=1, drop1=(0.1, 11), drop2=(0.2, 12)),
    "sliding_rows_gate": dict(gate=1, gate_scale=1.25, sliding=1),
}
TILED, WIDE160, WIDE128 = (0, 1 << 30), (160, 1), (128, 1)       # (tile_rows, min_rows) of eg_gemm_wide_config


@pytest.fixture(autouse=True)
def restore_wide_config():
    yield
    forced = os.environ.get("EYEGAZE_WIDE_TILE", "0")
    call("eg_gemm_wide_config", int(forced) if forced in ("128", "160") else 0, 1024)


class Product:
    """operands of one product; run() writes fresh sentinel-filled outputs and returns them whole"""

    def __init__(self, M, K, dtype, ep, seed):
        tdt, self.eg = TDT[dtype]
        self.M, self.K, self.ep, self.tdt = M, K, ep, tdt
        g = torch.Generator(device="cpu").manual_seed(seed + 131 * M + K)
        if ep.get("sliding"):
            # rows of 64 elements, 4 output rows per group: row r of a group reads K elements from its r-th row on (overlapping,
            # as the convolutions' rows do); C, gate: every other row of a [groups, 9, 256] buffer (gaps keep their sentinel)
            grp = 3 + K // 64
            self.A = (torch.randn(M // 4 * grp * 64, generator=g) * 0.5).to(tdt).to(DEV)
            self.amap = rowmap(64, grp * 64, 4)
            self.cmap = rowmap(2 * N, 9 * N, 4)
            self.crows = M // 4 * 9
        else:
            self.A = (torch.randn(M, K, generator=g) * 0.5).to(tdt).to(DEV)
            self.amap, self.cmap, self.crows = rowmap(K), rowmap(N), M
        self.W = (torch.randn(N, K, generator=g) * 0.1).to(tdt).to(DEV)
        self.b = torch.randn(N, generator=g).to(DEV)
        self.R = torch.randn(self.crows + 2 * GUARD, N, generator=g).to(tdt).to(DEV)
        self.G = torch.randn(self.crows + 2 * GUARD, N, generator=g).to(tdt).to(DEV)
        self.st = dev_state(seed=4321 + seed)

    def desc(self):
        ep, es = self.ep, 2
        self.out = torch.full((self.crows + 2 * GUARD, N), SENT, device=DEV, dtype=self.tdt)
        self.pre = torch.full((self.crows + 2 * GUARD, N), SENT, device=DEV, dtype=self.tdt)
        off = GUARD * N * es
        d = GemmDesc()
        d.A, d.W, d.C = ptr(self.A), ptr(self.W), ptr(self.out) + off
        d.bias = ptr(self.b) if ep.get("bias") else None
        d.residual = ptr(self.R) + off if ep.get("residual") else None
        d.gate = ptr(self.G) + off if ep.get("gate") else None
        d.out_pre = ptr(self.pre) + off if ep.get("out_pre") else None
        d.state = ptr(self.st)
        d.a, d.c, d.r, d.p = self.amap, self.cmap, self.cmap, self.cmap
        d.M, d.N, d.K, d.ldw, d.act, d.dtype = self.M, N, self.K, self.K, ep.get("act", 0), self.eg
        d.drop1_p, d.drop1_site = ep.get("drop1", (0.0, 0))
        d.drop2_p, d.drop2_site = ep.get("drop2", (0.0, 0))
        d.gate_scale = ep.get("gate_scale", 1.0)
        return d

    def outputs(self):
        torch.cuda.synchronize()
        return self.out.clone(), self.pre.clone()

    def check_sentinels(self, out, pre):
        for t in (out, pre):
            assert bool((t[:GUARD] == SENT).all()) and bool((t[-GUARD:] == SENT).all())
        if not self.ep.get("out_pre"):
            assert bool((pre == SENT).all())
        body = out[GUARD:-GUARD]
        if self.ep.get("sliding"):                     # rows 1, 3, 5, 7 and 8 of every group of 9 are gaps
            gaps = body.view(-1, 9, N)[:, [1, 3, 5, 7, 8]]
            assert bool((gaps == SENT).all())
            body = body.view(-1, 9, N)[:, [0, 2, 4, 6]]
        assert bool((body != SENT).any(dim=-1).all())  # every real row was written


def run_single(prod, cfg):
    call("eg_gemm_wide_config", *cfg)
    d = prod.desc()
    assert L.lib().eg_gemm_nt_route(C.byref(d)) == (0 if cfg == TILED else 1)
    call("eg_gemm_nt", C.byref(d), 0)
    return prod.outputs()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("ep", list(EPILOGUES))
def test_every_tile_gives_the_same_bytes(ep, dtype):
    for i, (M, K) in enumerate(SHAPES):
        prod = Product(M, K, dtype, EPILOGUES[ep], seed=i)
        ref_out, ref_pre = run_single(prod, TILED)
        prod.check_sentinels(ref_out, ref_pre)
        assert float(ref_out[GUARD:-GUARD].float().abs().max()) > 0
        for cfg in (WIDE160, WIDE128):
            out, pre = run_single(prod, cfg)
            assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (M, K, cfg)
            assert torch.equal(pre.view(torch.int16), ref_pre.view(torch.int16)), (M, K, cfg)


# unequal M and K across the products of a batch
BATCH_SHAPES = [(300, 448), (128, 128), (1024 + 16, 192), (520, 320)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("ep", ["sliding_rows_gate", "drop_both_sites"])
@pytest.mark.parametrize("n", [1, 3, 4])
def test_a_batch_gives_the_bytes_of_its_products_launched_one_by_one(n, ep, dtype):
    prods = [Product(M, K, dtype, EPILOGUES[ep], seed=20 + i) for i, (M, K) in enumerate(BATCH_SHAPES[:n])]
    refs = [run_single(p, WIDE160) for p in prods]
    for cfg in (WIDE128, WIDE160, (0, 1)):             # forced tiles, and the tile by rule
        call("eg_gemm_wide_config", *cfg)
        descs = (GemmDesc * n)()
        for i, p in enumerate(prods):
            descs[i] = p.desc()
        assert L.lib().eg_gemm_nt_batch_route(descs, n) == 1
        call("eg_gemm_nt_batch", descs, n, 0)
        for p, (ref_out, ref_pre) in zip(prods, refs):
            out, pre = p.outputs()
            p.check_sentinels(out, pre)
            assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16)), (p.M, p.K, cfg)
            assert torch.equal(pre.view(torch.int16), ref_pre.view(torch.int16)), (p.M, p.K, cfg)


def test_an_ineligible_batch_runs_as_single_launches():
    """one product below the wide kernel's row floor: the batch falls back to n eg_gemm_nt calls, same bytes"""
    prods = [Product(M, K, "bf16", EPILOGUES["gate_scale"], seed=40 + i) for i, (M, K) in enumerate([(1024 + 16, 192), (300, 448)])]
    refs = [run_single(p, TILED) for p in prods]
    call("eg_gemm_wide_config", 0, 1024)
    descs = (GemmDesc * 2)()
    for i, p in enumerate(prods):
        descs[i] = p.desc()
    assert L.lib().eg_gemm_nt_batch_route(descs, 2) == 0
    call("eg_gemm_nt_batch", descs, 2, 0)
    for p, (ref_out, _) in zip(prods, refs):
        out, pre = p.outputs()
        p.check_sentinels(out, pre)
        assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16))
