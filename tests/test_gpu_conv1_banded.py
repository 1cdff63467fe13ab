"""The banded conv-1 kernels (csrc/spec.hip: eg_spec_conv1_fwd_banded / _bwd_banded, one workgroup per (image, band of pooled rows))
with the recipe and the gates of tests/test_gpu_token_kernels.py's whole-image checks: the same seeded case, float64 autograd as
the reference, ambiguous arg-max cells zeroed on both sides, sentinel frame, NaN guard row, two runs bit-equal.  Wherever the
whole-image kernel can run too, the interior of p1 must be its output bit for bit.  Small shapes force a band height; the two large
ones take eg_spec_conv1_band_rows', the production rule."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests.test_gpu_ops import DEV, DT, tol  # noqa: E402
from tests.test_gpu_token_kernels import CONV1_SHAPES, NAN, conv1_case, sum_tol  # noqa: E402

ALL = [L.EG_BF16, L.EG_F16, L.EG_F32]
# (nimg, F, nfr, band_rows; None = production): four one-row bands that are all halo; three full bands; a ragged last band 8 + 8 + 4;
# an odd frame count (the model's own spectrogram); ragged 16 + 16 + 4 with wide rows; the reference's image size; the store's limit
SHAPES = [(1, 8, 8, 1), (2, 24, 16, 4), (3, 40, 8, 8), (2, 64, 17, 8), (2, 72, 120, 16), (1, 224, 224, None), (1, 512, 512, None)]
CASES = [pytest.param(s, dt, id="n%d_F%d_fr%d_b%s-%s" % (*s, {L.EG_BF16: "bf16", L.EG_F16: "fp16", L.EG_F32: "f32"}[dt]))
         for s in SHAPES for dt in ALL if not (s[1] == 512 and dt == L.EG_F16)]
LDS_MAX = 65536


def lds_fwd(rows, nfr):
    """bytes of dynamic LDS of a forward launch that stages `rows` rows: the rows, 32 x 9 weights, 32 biases (include/eyegaze_hip.h)"""
    return (rows * (nfr + 2) + 320) * 4


def band_of(shape):
    nimg, Fq, nfr, band = shape
    if band is None:
        band = L.spec_conv1_band_rows(Fq, nfr)
        assert band > 0 and band % 8 == 0, band
    return band


@pytest.mark.parametrize("shape,dtype", CASES)
def test_banded_forward(shape, dtype):
    nimg, Fq, nfr, _ = shape
    band = band_of(shape)
    Hp, Wp, td = Fq // 2, nfr // 2, DT[dtype]
    c = conv1_case(shape[:3])
    ref = c["y"].detach().permute(0, 2, 3, 1)                                         # [nimg, Hp, Wp, 32]
    share = float((ref > 0).double().mean())
    assert 0.25 < share < 0.75, share                                                 # both sides of the ReLU are populated
    imgd, wd, bd = c["img"].to(DEV), c["w"].to(DEV), c["b"].to(DEV)
    p1 = torch.full((nimg, Hp + 2, Wp + 4, 32), 7.0, dtype=td, device=DEV)
    call("eg_spec_conv1_fwd_banded", ptr(imgd), ptr(wd), ptr(bd), ptr(p1), nimg, Fq, nfr, band, dtype, 0)
    torch.cuda.synchronize()
    p1 = p1.cpu()
    inner = p1[:, 1:Hp + 1, 1:Wp + 1]
    torch.testing.assert_close(inner.double(), ref, **tol(dtype))
    frame = torch.ones(nimg, Hp + 2, Wp + 4, 32, dtype=torch.bool)
    frame[:, 1:Hp + 1, 1:Wp + 1] = False
    assert bool((p1[frame] == 7.0).all())                                             # the pad frame keeps the sentinel
    dead = (ref == 0) & ~c["ambiguous"].permute(0, 2, 3, 1)
    assert bool((inner[dead] == 0).all())                                             # ReLU-dead cells are exact zeros
    whole = lds_fwd(Fq + 2, nfr) <= LDS_MAX
    assert whole == (Fq <= 72)                                                        # the five small shapes, not 224 / 512
    if whole:
        q1 = torch.full((nimg, Hp + 2, Wp + 4, 32), 7.0, dtype=td, device=DEV)
        call("eg_spec_conv1_fwd", ptr(imgd), ptr(wd), ptr(bd), ptr(q1), nimg, Fq, nfr, dtype, 0)
        torch.cuda.synchronize()
        assert torch.equal(p1, q1.cpu())                                              # bit for bit, frame included


@pytest.mark.parametrize("shape,dtype", CASES)
def test_banded_backward(shape, dtype):
    nimg, Fq, nfr, _ = shape
    band = band_of(shape)
    Hp, Wp, td = Fq // 2, nfr // 2, DT[dtype]
    nrow = nimg * -(-Hp // band)
    c = conv1_case(shape[:3])
    amb = c["ambiguous"].permute(0, 2, 3, 1)                                          # [nimg, Hp, Wp, 32]
    share = float(amb.double().mean())
    print(f"banded conv1 bwd {shape}: {int(amb.sum())} of {amb.numel()} cells ambiguous ({share:.2e})")
    assert share <= 0.01, share
    dp1 = c["dp1"].to(td)
    dp1[:, :Hp][amb] = 0
    gy = dp1[:, :Hp].double().permute(0, 3, 1, 2)
    dW, db = torch.autograd.grad(c["y"], (c["w64"], c["b64"]), gy, retain_graph=True)
    imgd, wd, bd, gd = c["img"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), dp1.to(DEV)
    runs = []
    for _ in range(2):
        partial = torch.full((nrow + 1, 320), NAN, device=DEV)
        call("eg_spec_conv1_bwd_banded", ptr(imgd), ptr(wd), ptr(bd), ptr(gd), ptr(partial), nimg, Fq, nfr, band, dtype, 0)
        torch.cuda.synchronize()
        runs.append(partial.cpu())
    partial = runs[0]
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))          # two runs give the same bytes
    assert bool(torch.isnan(partial[nrow]).all())                                     # the row behind the last one
    assert bool(torch.isfinite(partial[:nrow]).all())
    got = partial[:nrow].double().sum(0)
    cells = nimg * Hp * Wp
    eW = float((got[:288].view(32, 9) - dW.view(32, 9)).abs().max())
    eb = float((got[288:] - db).abs().max())
    print(f"  dW err {eW:.3e} (gate {sum_tol(dW, cells):.3e})  db err {eb:.3e} (gate {sum_tol(db, cells):.3e})")
    assert eW <= sum_tol(dW, cells), (eW, sum_tol(dW, cells))
    assert eb <= sum_tol(db, cells), (eb, sum_tol(db, cells))


def test_band_rows_rule():
    """0 wherever the whole-image kernels run today; at the image sizes a multiple of 8 whose backward band fits 64 KiB"""
    for _, Fq, nfr in CONV1_SHAPES + [(4, 64, 16)]:
        assert L.spec_conv1_band_rows(Fq, nfr) == 0, (Fq, nfr)
    for Fq, nfr in ((224, 224), (512, 512)):
        b = L.spec_conv1_band_rows(Fq, nfr)
        assert b > 0 and b % 8 == 0 and b <= Fq // 2, (Fq, nfr, b)
        assert lds_fwd(2 * b + 2, nfr) + 8 * 32 * 10 * 4 <= LDS_MAX, (Fq, nfr, b)
        assert lds_fwd(Fq + 2, nfr) > LDS_MAX                                         # the whole image cannot be staged


def test_bad_shapes_and_the_whole_image_entry_at_224():
    t = torch.zeros(1024, device=DEV)
    for Fq, nfr in ((12, 8), (8, 6), (16, 10)):        # F % 8 != 0; fewer than 8 frames; floor(frames / 2) % 4 != 0
        for name, extra in (("eg_spec_conv1_fwd_banded", ()), ("eg_spec_conv1_bwd_banded", (ptr(t),))):
            with pytest.raises(L.EgError, match=r"unsupported \(F % 8 == 0 and floor\(frames/2\) % 4 == 0 required\)"):
                call(name, ptr(t), ptr(t), ptr(t), ptr(t), *extra, 1, Fq, nfr, 1, L.EG_F32, 0)
    with pytest.raises(L.EgError, match="band_rows 5 outside"):
        call("eg_spec_conv1_fwd_banded", ptr(t), ptr(t), ptr(t), ptr(t), 1, 8, 8, 5, L.EG_F32, 0)
    # the whole-image entry points at the reference's size: refused on the host, naming the banded entry, nothing launched
    img = torch.zeros(1, 224, 224, device=DEV)
    p1 = torch.full((1, 114, 116, 32), 7.0, device=DEV)
    part = torch.full((2, 320), NAN, device=DEV)
    dp1 = torch.zeros(1, 114, 112, 32, device=DEV)
    with pytest.raises(L.EgError, match="eg_spec_conv1_fwd_banded"):
        call("eg_spec_conv1_fwd", ptr(img), ptr(t), ptr(t), ptr(p1), 1, 224, 224, L.EG_F32, 0)
    with pytest.raises(L.EgError, match="eg_spec_conv1_bwd_banded"):
        call("eg_spec_conv1_bwd", ptr(img), ptr(t), ptr(t), ptr(dp1), ptr(part), 1, 224, 224, L.EG_F32, 0)
    torch.cuda.synchronize()
    assert bool((p1 == 7.0).all()) and bool(torch.isnan(part).all())
