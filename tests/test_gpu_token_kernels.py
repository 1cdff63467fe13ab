"""Direct checks of the token families' small kernels, which the model fixtures reach only at B = 4, C = 8 / 32 (E = C*C a multiple
of 64, 17 frames) and with dropout off.  Each against a float64 statement of the same operation on the same rounded operands:
  * eg_gelu_fwd / eg_gelu_bwd (csrc/signal.hip): erf-GELU + counter-hash dropout of the tokenizer bottleneck and its backward;
  * eg_ibs_inorm: instance norm over the token axis of the selected connectivity features, + affine, + xhat;
  * eg_affine_grad: the split column sums behind the instance norm's gain / bias gradients, empty splits included;
  * eg_spec_conv1_fwd / _bwd (csrc/spec.hip): Conv2d(1, 32, 3, p1) + ReLU + MaxPool2 into the padded channel-last layout, and its
    weight / bias gradient with the pooled gradient routed to the arg-max.
Outputs are pre-filled with a sentinel wherever "written" or "not written" is part of the contract."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.engine import SITE_IBSTOK, scramble_seed  # noqa: E402
from tests.helpers import hip_keep_mask  # noqa: E402
from tests.test_gpu_ops import DEV, DT, dev_state, tol  # noqa: E402

DTYPES = [L.EG_BF16, L.EG_F16, L.EG_F32]
NAN = float("nan")


def sum_tol(ref, length):
    """fp32 sums of `length` terms (the form of tests/test_gpu_spec_kernels.py): 2e-5 * max|ref| + 1e-6 * sqrt(length)"""
    return 2e-5 * float(ref.abs().max()) + 1e-6 * length ** 0.5


# ------------------------------------------------------------------------------------------------------------------------
# eg_gelu_fwd / eg_gelu_bwd
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("n", [1, 255, 257, 10752, 10755])
def test_gelu_dropout_forward_and_backward(n, p, dtype):
    """h = drop(gelu(u)), du = dh * mask / (1 - p) * gelu'(u).  Odd n: the last element's pair hash straddles the end; 257 and 10755:
    one element into the next 256-thread block.  The state carries scramble_seed(seed), as Engine.set_state fills it, so that the
    mask is tests/helpers.py::hip_keep_mask's EXACTLY (dev_state alone stores the seed unscrambled: tests/test_gpu_rsgemm.py)."""
    td, seed, pad = DT[dtype], 0xABC_DEF1_2345 + n, 8
    g = torch.Generator().manual_seed(n)
    u = (torch.randn(n, generator=g) * 1.5).to(td)
    dh = torch.randn(n, generator=g).to(td)
    st = dev_state(seed=scramble_seed(seed))
    ud, dhd = u.to(DEV), dh.to(DEV)
    outs = []
    for _ in range(2):
        h = torch.full((n + pad,), 7.0, dtype=td, device=DEV)
        du = torch.full((n + pad,), 7.0, dtype=td, device=DEV)
        call("eg_gelu_fwd", ptr(ud), ptr(h), n, dtype, p, SITE_IBSTOK, ptr(st), 0)
        call("eg_gelu_bwd", ptr(ud), ptr(dhd), ptr(du), n, dtype, p, SITE_IBSTOK, ptr(st), 0)
        torch.cuda.synchronize()
        outs.append((h.cpu(), du.cpu()))
    (h, du), (h2, du2) = outs
    assert torch.equal(h, h2) and torch.equal(du, du2)                                  # two runs are bit-equal
    assert bool((h[n:] == 7.0).all()) and bool((du[n:] == 7.0).all())                   # nothing past n is written
    h, du = h[:n].double(), du[:n].double()
    x = u.double()
    cdf = 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5))
    gelu, dgelu = x * cdf, cdf + x * torch.exp(-0.5 * x * x) / (2.0 * np.pi) ** 0.5
    if p > 0:
        keep = torch.from_numpy(hip_keep_mask(seed, SITE_IBSTOK, np.arange(n, dtype=np.uint32), p))
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))            # fp32 1 / (1 - p)
    else:
        keep, scale = torch.ones(n, dtype=torch.bool), 1.0
    zero = torch.zeros((), dtype=torch.float64)
    ref_h = torch.where(keep, gelu * scale, zero)
    ref_du = torch.where(keep, dh.double() * scale * dgelu, zero)
    torch.testing.assert_close(h, ref_h, **tol(dtype))
    torch.testing.assert_close(du, ref_du, **tol(dtype))
    # dropped elements are exact zeros, kept ones of any size are not: forward and backward draw the SAME mask, the expected one
    assert bool((h[~keep] == 0).all()) and bool((du[~keep] == 0).all())
    assert bool((h[keep & (ref_h.abs() > 1e-3)] != 0).all())
    assert bool((du[keep & (ref_du.abs() > 1e-3)] != 0).all())
    if p > 0 and n > 1000:
        assert 0.08 < float((~keep).double().mean()) < 0.12


# ------------------------------------------------------------------------------------------------------------------------
# eg_ibs_inorm
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fidx", [list(range(7)), [6, 0, 3], [2]], ids=["all7", "f603", "f2"])
@pytest.mark.parametrize("E", [25, 64, 300, 1024])
def test_ibs_inorm(E, fidx, dtype):
    """[B, 6, 7, E] connectivity -> token rows [B * 6 * nfeat, E]: the features fidx in THAT order, instance norm over the token axis
    (biased variance, eps 1e-5), gamma / beta per column; xhat in fp32.  E below, above and not a multiple of the 256-column block.
    use_norm = 0 (ibs_instance_norm = False): the selected values rounded to the dtype, xhat untouched."""
    td, nb, nf = DT[dtype], 6, len(fidx)
    ntok = nb * nf
    g = torch.Generator().manual_seed(E * 10 + nf)
    for B in (1, 3):
        conn = torch.randn(B, nb, 7, E, generator=g) * 0.5 + 0.3
        gamma, beta = 1.0 + 0.2 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
        sel = conn[:, :, fidx].reshape(B, ntok, E)                  # token = band * nfeat + position in fidx
        cd, fd, gd, bd = conn.to(DEV), torch.tensor(fidx, dtype=torch.int32, device=DEV), gamma.to(DEV), beta.to(DEV)
        for use_norm in (1, 0):
            out = torch.full((B * ntok + 1, E), 7.0, dtype=td, device=DEV)
            xhat = torch.full((B * ntok + 1, E), NAN, device=DEV)
            call("eg_ibs_inorm", ptr(cd), ptr(fd), ptr(gd) if use_norm else 0, ptr(bd) if use_norm else 0, ptr(out), ptr(xhat),
                 B, nb, nf, E, use_norm, dtype, 0)
            torch.cuda.synchronize()
            out, xhat = out.cpu(), xhat.cpu()
            assert bool((out[-1] == 7.0).all()) and bool(torch.isnan(xhat[-1]).all())        # the guard row after the last token
            out, xhat = out[:-1].view(B, ntok, E), xhat[:-1].view(B, ntok, E)
            if not use_norm:
                assert torch.equal(out, sel.to(td))
                assert bool(torch.isnan(xhat).all())                                          # xhat keeps its sentinel
                continue
            x = sel.double()
            xh = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
            torch.testing.assert_close(xhat.double(), xh, **tol(L.EG_F32))
            torch.testing.assert_close(out.double(), xh * gamma.double() + beta.double(), **tol(dtype))


# ------------------------------------------------------------------------------------------------------------------------
# eg_affine_grad
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [25, 64, 300])
def test_affine_grad(E, dtype):
    """partial[sp][0][e] / [sp][1][e] = split sp's share of sum_m dy[m, e] * xhat[m, e] / sum_m dy[m, e]; split sp owns rows
    4 sp .. 4 sp + 3 (mod 4 nsplit), so with 4 nsplit > M some splits own no row and must still write zeros (the caller sums every
    split: eg_reduce_partials)."""
    td = DT[dtype]
    g = torch.Generator().manual_seed(E)
    for M in (1, 3, 168, 170):
        dy = torch.randn(M, E, generator=g).to(td)
        xhat = torch.randn(M, E, generator=g)
        ref_g, ref_b = (dy.double() * xhat.double()).sum(0), dy.double().sum(0)
        dyd, xd = dy.to(DEV), xhat.to(DEV)
        for nsplit in (1, 2, 43, 256):
            partial = torch.full((nsplit + 1, 2, E), NAN, device=DEV)
            call("eg_affine_grad", ptr(dyd), ptr(xd), ptr(partial), nsplit, M, E, dtype, 0)
            torch.cuda.synchronize()
            partial = partial.cpu()
            assert bool(torch.isnan(partial[nsplit]).all()), (M, nsplit)                       # the guard split
            part = partial[:nsplit]
            assert bool(torch.isfinite(part).all()), (M, nsplit)                               # empty splits wrote zeros
            empty = [sp for sp in range(nsplit) if 4 * sp >= M]
            assert float(part[empty].abs().sum()) == 0.0, (M, nsplit)
            got = part.double().sum(0)
            assert float((got[0] - ref_g).abs().max()) <= sum_tol(ref_g, M), (M, nsplit)
            assert float((got[1] - ref_b).abs().max()) <= sum_tol(ref_b, M), (M, nsplit)


# ------------------------------------------------------------------------------------------------------------------------
# eg_spec_conv1_fwd / eg_spec_conv1_bwd
# ------------------------------------------------------------------------------------------------------------------------
# odd frame counts, Hp below 8 and not a multiple of 8, the model's own 64 x 17 image
CONV1_SHAPES = [(3, 8, 8), (3, 8, 9), (5, 24, 16), (1, 40, 8), (2, 64, 17)]
AMBIGUOUS = 1e-4


@functools.lru_cache(maxsize=None)
def conv1_case(shape):
    """inputs and float64 references of one shape, shared by the dtypes (never modified).  The bias is shifted so that a real share
    of the pooled cells is ReLU-dead."""
    nimg, Fq, nfr = shape
    Hp, Wp = Fq // 2, nfr // 2
    g = torch.Generator().manual_seed(nimg * 10000 + Fq * 100 + nfr)
    img = torch.randn(nimg, Fq, nfr, generator=g)
    w = torch.randn(32, 1, 3, 3, generator=g) / 3
    b = torch.randn(32, generator=g) * 0.1 - 1.0
    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    pre = F.conv2d(img.double().unsqueeze(1), w64, b64, padding=1)                    # [nimg, 32, F, nfr]
    y = F.max_pool2d(torch.relu(pre), 2)                                              # [nimg, 32, Hp, Wp]
    # per pooled cell: margin between the best and the second-best pre-activation of its 2 x 2 window, distance of the best from 0
    win = pre.detach()[:, :, : 2 * Hp, : 2 * Wp].reshape(nimg, 32, Hp, 2, Wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(nimg, 32, Hp, Wp, 4)
    top = win.topk(2, dim=-1).values
    ambiguous = ((top[..., 0] - top[..., 1]) < AMBIGUOUS) | (top[..., 0].abs() < AMBIGUOUS)
    gd = torch.randn(nimg, Hp + 2, Wp, 32, generator=g)                               # gradient of p1; rows >= Hp are unused
    return dict(img=img, w=w, b=b, w64=w64, b64=b64, y=y, ambiguous=ambiguous, dp1=gd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=lambda s: "n%d_F%d_fr%d" % s)
def test_spec_conv1_forward(shape, dtype):
    """p1 [nimg, Hp+2, Wp+4, 32]: the interior [1:Hp+1, 1:Wp+1] = max_pool2d(relu(conv2d(img, w, b, padding=1)), 2), channel-last;
    the pad frame (one row above / below, one pixel left, three right) is NOT written: the engine zeroes it once, conv-2 reads it"""
    nimg, Fq, nfr = shape
    Hp, Wp, td = Fq // 2, nfr // 2, DT[dtype]
    c = conv1_case(shape)
    ref = c["y"].detach().permute(0, 2, 3, 1)                                         # [nimg, Hp, Wp, 32]
    share = float((ref > 0).double().mean())
    assert 0.25 < share < 0.75, share                                                 # both sides of the ReLU are populated
    p1 = torch.full((nimg, Hp + 2, Wp + 4, 32), 7.0, dtype=td, device=DEV)
    imgd, wd, bd = c["img"].to(DEV), c["w"].to(DEV), c["b"].to(DEV)
    call("eg_spec_conv1_fwd", ptr(imgd), ptr(wd), ptr(bd), ptr(p1), nimg, Fq, nfr, dtype, 0)
    torch.cuda.synchronize()
    p1 = p1.cpu()
    torch.testing.assert_close(p1[:, 1:Hp + 1, 1:Wp + 1].double(), ref, **tol(dtype))
    frame = torch.ones(nimg, Hp + 2, Wp + 4, 32, dtype=torch.bool)
    frame[:, 1:Hp + 1, 1:Wp + 1] = False
    assert bool((p1[frame] == 7.0).all())                                             # bit for bit the sentinel
    dead = (ref == 0) & ~c["ambiguous"].permute(0, 2, 3, 1)                           # best pre-activation below -1e-4
    assert bool((p1[:, 1:Hp + 1, 1:Wp + 1][dead] == 0).all())                         # ReLU-dead cells are exact zeros


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CONV1_SHAPES, ids=lambda s: "n%d_F%d_fr%d" % s)
def test_spec_conv1_backward(shape, dtype):
    """partial [nimg, 320] = per image (dW[32][9] | db[32]) of Conv2d(1, 32, 3, p1) + ReLU + MaxPool2 from dp1 [nimg, Hp+2, Wp, 32],
    against float64 autograd of that statement.  Arg-max routing is discontinuous: on cells whose best pre-activation is within 1e-4
    of the second best or of 0 (float64), dp1 is zeroed before the kernel and the reference see it; at most 1 % of the cells."""
    nimg, Fq, nfr = shape
    Hp, Wp, td = Fq // 2, nfr // 2, DT[dtype]
    c = conv1_case(shape)
    amb = c["ambiguous"].permute(0, 2, 3, 1)                                          # [nimg, Hp, Wp, 32]
    share = float(amb.double().mean())
    print(f"conv1 bwd {shape}: {int(amb.sum())} of {amb.numel()} cells ambiguous ({share:.2e})")
    assert share <= 0.01, share
    dp1 = c["dp1"].to(td)
    dp1[:, :Hp][amb] = 0
    gy = dp1[:, :Hp].double().permute(0, 3, 1, 2)
    dW, db = torch.autograd.grad(c["y"], (c["w64"], c["b64"]), gy, retain_graph=True)
    partial = torch.full((nimg + 1, 320), NAN, device=DEV)
    imgd, wd, bd, gd = c["img"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), dp1.to(DEV)
    call("eg_spec_conv1_bwd", ptr(imgd), ptr(wd), ptr(bd), ptr(gd), ptr(partial), nimg, Fq, nfr, dtype, 0)
    torch.cuda.synchronize()
    partial = partial.cpu()
    assert bool(torch.isnan(partial[nimg]).all())                                     # the guard row
    assert bool(torch.isfinite(partial[:nimg]).all())
    got = partial[:nimg].double().sum(0)
    cells = nimg * Hp * Wp
    eW = float((got[:288].view(32, 9) - dW.view(32, 9)).abs().max())
    eb = float((got[288:] - db).abs().max())
    assert eW <= sum_tol(dW, cells), (eW, sum_tol(dW, cells))
    assert eb <= sum_tol(db, cells), (eb, sum_tol(db, cells))
