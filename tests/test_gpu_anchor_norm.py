"""eg_layernorm_fwd / eg_layernorm_bwd against their fp64 statements (tests/anchor_ref.py), dx_drop included.

eg_ln_bwd_proj and eg_ffn_bwd_ln_proj are held bit for bit to eg_layernorm_bwd; this file holds eg_layernorm_bwd itself: the
generic kernel (D = 4 ... 1024) and the D = 256 half-wave kernel, one row and a ragged 130, fewer and more blocks than rows,
random gain and bias, and an input whose rows sit at 100 with a spread of 0.01.  dx_drop's zero pattern must be the mask
replayed on the CPU, element for element; its kept values, dx, the gain and bias gradients and the forward's y, mean and rstd
must lie within 1.5 u |ref| + slack, the slack measured on the CPU from the float32 evaluation of the reference formula."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.engine import scramble_seed  # noqa: E402
from tests import anchor_ref as R  # noqa: E402
from tests.test_gpu_ops import dev_state  # noqa: E402

DEV = "cuda"


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("D,M,kind", R.NORM_CASES)
def test_layernorm_fwd_bwd_match_fp64(D, M, kind, dtype):
    x, gamma, beta, dy = R.norm_case(D, M, kind, dtype)
    eg, tdt = R.EG[dtype], R.TDT[dtype]
    xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    y = torch.full((M + 2, D), R.SENT, device=DEV, dtype=tdt)                 # one sentinel row at each end
    stats = torch.full((M + 2, 2), R.SENT, device=DEV)
    call("eg_layernorm_fwd", ptr(xd), ptr(gd), ptr(bd), ptr(y) + D * x.element_size(), ptr(stats) + 8, M, D, eg, 0)
    torch.cuda.synchronize()
    for t in (y, stats):
        assert bool((t[0] == R.SENT).all()) and bool((t[-1] == R.SENT).all())
    got = dict(y=y[1:-1].double().cpu(), mean=stats[1:-1, 0].double().cpu(), rstd=stats[1:-1, 1].double().cpu())
    R.assert_all_within(got, R.norm_fwd_outputs(x, gamma, beta, dtype), "D%d M%d %s %s fwd" % (D, M, kind, dtype))
    # backward from the STORED statistics, on both sides
    st_dev = stats[1:-1].contiguous()
    mean, rstd = st_dev[:, 0].cpu(), st_dev[:, 1].cpu()
    st = dev_state(seed=scramble_seed(R.NORM_SEED))
    for nblk, (d1, d2) in itertools.product(R.NORM_NBLK, R.NORM_DROPS):
        dx = torch.full((M + 2, D), R.SENT, device=DEV, dtype=tdt)
        dd = torch.full((M + 2, D), R.SENT, device=DEV, dtype=tdt)
        part = torch.full((nblk + 1, 2, D), R.SENT, device=DEV)
        rowb = D * x.element_size()
        call("eg_layernorm_bwd", ptr(dyd), ptr(xd), ptr(st_dev), ptr(gd), ptr(dx) + rowb, ptr(dd) + rowb, ptr(part), nblk, nblk, M, D,
             eg, d1[0], d1[1], d2[0], d2[1], ptr(st), 0)
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        torch.cuda.synchronize()
        assert bool((part[nblk] == R.SENT).all()), "a block wrote past its own row of the partials"
        call("eg_reduce_partials", ptr(part), ptr(dg), D, nblk, 2 * D, 0, 0)
        call("eg_reduce_partials", ptr(part) + 4 * D, ptr(db), D, nblk, 2 * D, 0, 0)
        torch.cuda.synchronize()
        for t in (dx, dd):
            assert bool((t[0] == R.SENT).all()) and bool((t[-1] == R.SENT).all())
        got = dict(dx=dx[1:-1].double().cpu(), dx_drop=dd[1:-1].double().cpu(), dgamma=dg.double().cpu(), dbeta=db.double().cpu())
        what = "D%d M%d %s %s bwd nblk=%d p=(%g, %g)" % (D, M, kind, dtype, nblk, d1[0], d2[0])
        # the zero pattern IS the replayed mask: a dropped element is an exact zero, a kept one is zero only where dx itself is
        keep = R.norm_keep(M, D, d1, d2, R.NORM_SEED)
        assert torch.equal(got["dx_drop"] != 0, keep & (got["dx"] != 0)), what + ": dx_drop's zeros are not the replayed mask"
        assert int((~keep).sum()) > 0 or M * D < 16
        R.assert_all_within(got, R.norm_bwd_outputs(dy, x, mean, rstd, gamma, d1, d2, dtype), what)
