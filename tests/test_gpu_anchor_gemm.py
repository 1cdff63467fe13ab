"""eg_gemm_nt against its fp64 statement (tests/anchor_ref.py::gemm_nt_ref), on every route eg_gemm_nt takes.

The fused routes (eg_ffn_chain, eg_attn_block_fwd, eg_ln_bwd_proj, the sliced heads ...) are held bit for bit to "the eg_gemm_nt
launches they replace"; this file holds those launches themselves: the whole epilogue in the header's order, the dropout
element index m * N + n of the LOGICAL row with both sites replayed on the CPU, out_pre as the value before the residual, the
separate c / r / p row maps, ldw != K, segmented A rows, GELU and the 256 x 64 narrow tile.  Every output lies between sentinel
rows in a buffer whose rows are further apart than N; the sentinels must survive, the zeros of the gate and of the dropouts
must be exact zeros, and EVERY element must lie within 1.5 u |ref| + the derived product slack."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import GemmDesc, call, ptr, rowmap  # noqa: E402
from eyegaze_multimodal_amd.engine import scramble_seed  # noqa: E402
from tests import anchor_ref as R  # noqa: E402
from tests.test_gpu_ops import dev_state  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def wide_config():
    call("eg_gemm_wide_config", 0, 1024)
    yield
    forced = os.environ.get("EYEGAZE_WIDE_TILE", "0")
    call("eg_gemm_wide_config", int(forced) if forced in ("128", "160") else 0, 1024)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_nt_matches_fp64(name, dtype):
    cs = R.GEMM_CASES[name]
    A, W, kw = R.gemm_case(name, dtype)
    es = A.element_size()
    dev = {k: (kw[k].to(DEV) if kw[k] is not None else None) for k in ("C", "bias", "residual", "gate", "out_pre")}
    Ad, Wd = A.to(DEV), W.to(DEV)
    st = dev_state(seed=scramble_seed(kw["seed"]))           # the words Engine.set_state publishes, which the CPU replays
    off = kw["base"] * es
    d = GemmDesc()
    d.A, d.W, d.C = ptr(Ad), ptr(Wd), ptr(dev["C"]) + off
    d.bias = ptr(dev["bias"]) or None
    for k in ("residual", "gate", "out_pre"):
        setattr(d, k, ptr(dev[k]) + off if dev[k] is not None else None)
    d.state = ptr(st)
    d.a, d.c, d.r, d.p = rowmap(*kw["a"]), rowmap(*kw["c"]), rowmap(*kw["r"]), rowmap(*kw["p"])
    d.M, d.N, d.K, d.ldw, d.act, d.dtype = kw["M"], kw["N"], kw["K"], kw["ldw"], kw["act"], R.EG[dtype]
    d.drop1_p, d.drop1_site = kw["drop1"]
    d.drop2_p, d.drop2_site = kw["drop2"]
    d.gate_scale, d.a_seg_len, d.a_seg_stride = kw["gate_scale"], kw["a_seg_len"], kw["a_seg_stride"]
    if cs.get("tile"):
        call("eg_gemm_wide_config", cs["tile"], 1024)
    route = L.lib().eg_gemm_nt_route(C.byref(d))
    assert route == (R.ROUTE_TILED if dtype == "f32" else cs["route"]), route
    call("eg_gemm_nt", C.byref(d), 0)
    torch.cuda.synchronize()
    ref = R.gemm_nt_ref(A, W, **kw)
    got = {"C": dev["C"].double().cpu()}
    if dev["out_pre"] is not None:
        got["out_pre"] = dev["out_pre"].double().cpu()
    for k, tag in (("C", "C"), ("out_pre", "pre")):
        if k not in got:
            continue
        assert bool((got[k][~ref["written_" + tag]] == R.SENT).all()), "%s: a sentinel was overwritten" % k
        assert bool((got[k][ref["zero_" + tag]] == 0).all()), "%s: the gate's / the dropouts' zeros are not exact" % k
    R.assert_all_within(got, R.gemm_outputs(ref, dtype), "%s %s" % (name, dtype))
