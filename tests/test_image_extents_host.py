"""CPU-only extent audit of the image engine: every launch of one ImageEngine.forward(train=True) + backward is recorded instead of
issued (profiles/tools/launch_trace.py's Recorder), every pointer argument -- and every pointer inside a descriptor -- must resolve
to a named engine tensor (the caller's glogits is the one temporary), and offset + extent must stay inside that tensor, with the
extent computed from a formula written in this file next to its assertion.  A launch without a formula fails the test by name.

Shapes: the reference's 224 x 224 at its batch of 16 in bf16 and f32, the image store's limit 512 x 512, and the 64 x 16 that the
multimodal fixtures run.  At Wp = 112 and 256 conv-2 leaves the flat-correlation kernels for the segmented-row eg_gemm_nt / eg_gemm_tn
in every dtype; at 64 x 16 in bf16 it is on them.  Nothing at 224 or 512 runs on a GPU before this passes."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

from eyegaze_multimodal_amd import engine as E, image_encoder, tokens
from eyegaze_multimodal_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "profiles" / "tools"))
from launch_trace import Recorder  # noqa: E402

CPU = torch.device("cpu")
DT = {"bf16": L.EG_BF16, "f32": L.EG_F32}
CASES = [(16, 224, 224, "bf16"), (16, 224, 224, "f32"), (2, 512, 512, "bf16"), (4, 64, 16, "bf16")]
LDS_MAX = 65536         # dynamic LDS of a launch that does not raise the kernel's attribute (conv-1, both routes)


def es_of(dtype):
    return 4 if dtype == L.EG_F32 else 2


def last_row(m, M):
    """element offset of the furthest row start among rows 0 .. M-1 of a row map (strides are non-negative here)"""
    assert m.row_stride >= 0 and m.group_stride >= 0
    if m.rows_per_group <= 0:
        return (M - 1) * m.row_stride
    def start(r):
        return (r // m.rows_per_group) * m.group_stride + (r % m.rows_per_group) * m.row_stride
    full = (M - 1) // m.rows_per_group * m.rows_per_group - 1       # the last row of the last complete group before row M-1's
    return max(start(M - 1), start(full) if full >= 0 else 0)


class Audit(Recorder):
    """Recorder that checks each launch as it is recorded (backward allocates lazily: the tensors alive at the call count)"""

    def __init__(self, real):
        super().__init__(real)
        self.active, self.seen, self.temporaries = False, [], {}

    def span(self, launch, what, p, nbytes, optional=False):
        """the bytes [p, p + nbytes) lie inside one named tensor"""
        p = getattr(p, "value", p) or 0
        if not p:
            assert optional, f"{launch}: {what} is null"
            return None
        for lo, hi, name, t in self._known:
            if lo <= p < hi:
                assert nbytes > 0 and p - lo + nbytes <= hi - lo, \
                    f"{launch}: {what} = {name} + {p - lo} needs {nbytes} bytes, the tensor holds {hi - lo}"
                return name
        raise AssertionError(f"{launch}: {what} ({p:#x}) resolves to no engine tensor")

    def __call__(self, name, *args):
        super().__call__(name, *args)
        if not self.active:
            return
        self._known = self.known()
        fn = FORMULAS.get(name)
        assert fn is not None, f"{name}: the audit has no extent formula for this launch"
        fn(self, name, *[getattr(a, "_obj", a) for a in args])
        self.seen.append(name)


# ------------------------------------------------------------------------------------------------------------------------------
# the formulas.  Sizes in bytes; es = element size of the compute dtype; Hp = F // 2, Wp = nfr // 2.
# ------------------------------------------------------------------------------------------------------------------------------
def conv1_common(au, who, img, w, bias, nimg, F, nfr):
    au.span(who, "img", img, nimg * F * nfr * 4)                    # [nimg][F][nfr] f32
    au.span(who, "w", w, 32 * 9 * 4)
    au.span(who, "bias", bias, 32 * 4)


def p1_written(nimg, Hp, Wp, ch):
    """elements up to the last interior cell of a padded channel-last [nimg][Hp+2][Wp+4][ch] image: image nimg-1, row Hp, pixel Wp"""
    return ((nimg - 1) * (Hp + 2) * (Wp + 4) + Hp * (Wp + 4) + Wp) * ch + ch


def conv1_fwd(au, who, img, w, bias, p1, nimg, F, nfr, dtype, stream, band_rows=None):
    conv1_common(au, who, img, w, bias, nimg, F, nfr)
    rows = F + 2 if band_rows is None else 2 * band_rows + 2
    assert (rows * (nfr + 2) + 320) * 4 <= LDS_MAX, f"{who}: LDS"
    assert band_rows is None or 1 <= band_rows <= F // 2
    assert au.span(who, "p1", p1, p1_written(nimg, F // 2, nfr // 2, 32) * es_of(dtype)) == "a.sp_p1"


def conv1_bwd(au, who, img, w, bias, dp1, partial, nimg, F, nfr, dtype, stream, band_rows=None):
    conv1_common(au, who, img, w, bias, nimg, F, nfr)
    Hp, Wp = F // 2, nfr // 2
    rows = F + 2 if band_rows is None else 2 * band_rows + 2
    assert (rows * (nfr + 2) + 320 + 8 * 32 * 10) * 4 <= LDS_MAX, f"{who}: LDS"
    nbands = 1 if band_rows is None else -(-Hp // band_rows)
    # dp1 [nimg][Hp+2][Wp][32]: rows < Hp of every image are read
    au.span(who, "dp1", dp1, ((nimg - 1) * (Hp + 2) * Wp + Hp * Wp) * 32 * es_of(dtype))
    assert au.span(who, "partial", partial, nimg * nbands * 320 * 4) == "g.sp_part"


def gemm_nt(au, who, d, stream):
    es, M, N, K = es_of(d.dtype), d.M, d.N, d.K
    # an A row is K contiguous elements, or K / a_seg_len segments of a_seg_len elements, a_seg_stride apart
    a_row = (K // d.a_seg_len - 1) * d.a_seg_stride + d.a_seg_len if d.a_seg_len else K
    assert not d.a_seg_len or K % d.a_seg_len == 0
    au.span(who, "A", d.A, (last_row(d.a, M) + a_row) * es)
    au.span(who, "W", d.W, ((N - 1) * d.ldw + K) * es)
    au.span(who, "C", d.C, (last_row(d.c, M) + N) * es)
    au.span(who, "bias", d.bias, N * 4, optional=True)
    au.span(who, "residual", d.residual, (last_row(d.r, M) + N) * es, optional=True)
    au.span(who, "gate", d.gate, (last_row(d.c, M) + N) * es, optional=True)          # gate rows are addressed by `c`
    au.span(who, "out_pre", d.out_pre, (last_row(d.p, M) + N) * es, optional=True)
    au.span(who, "state", d.state, C.sizeof(L.StepState), optional=not (d.drop1_p or d.drop2_p))


def gemm_tn(au, who, d, stream):
    es, M, N, K = es_of(d.dtype), d.M, d.N, d.K
    au.span(who, "dY", d.dY, (last_row(d.y, M) + N) * es)
    # an X row is K contiguous elements, or K / 128 tiles of 128 columns, x_tile_stride apart
    if d.x_tile_stride in (0, 128):
        x_row = K
    else:
        assert K % 128 == 0
        x_row = (K // 128 - 1) * d.x_tile_stride + 128
    au.span(who, "X", d.X, (last_row(d.x, M) + x_row) * es)
    slab = N * K + (N if d.has_bias else 0)
    assert d.splits * slab <= au.eng.tn_cap, f"{who}: {d.splits} slabs of {slab} floats exceed tn_cap"
    assert au.span(who, "partial", d.partial, d.splits * slab * 4) == "g.partial"


def avgpool_fwd(au, who, out2, pooled, nimg, Hp, Wp, dtype, stream):
    es = es_of(dtype)
    au.span(who, "out2", out2, ((nimg - 1) * (Hp + 2) * Wp + Hp * Wp) * 64 * es)       # [nimg][Hp+2][Wp][64], rows < Hp read
    au.span(who, "pooled", pooled, nimg * 1024 * es)


def avgpool_bwd(au, who, out2, dpooled, d2, nimg, Hp, Wp, dtype, stream):
    es = es_of(dtype)
    au.span(who, "out2", out2, ((nimg - 1) * (Hp + 2) * Wp + Hp * Wp) * 64 * es)
    au.span(who, "dpooled", dpooled, nimg * 1024 * es)
    au.span(who, "d2", d2, p1_written(nimg, Hp, Wp, 64) * es)                          # interiors of [nimg][Hp+2][Wp+4][64]


def reduce_partials(au, who, partial, out, n, splits, stride, accumulate, stream):
    assert stride >= n
    au.span(who, "partial", partial, ((splits - 1) * stride + n) * 4)
    au.span(who, "out", out, n * 4)


def unpack_conv2d_wgrad(au, who, partial, dW, splits, N, Cin, stream):
    au.span(who, "partial", partial, splits * N * 12 * Cin * 4)                        # [splits][N][12 * Cin]
    au.span(who, "dW", dW, N * Cin * 9 * 4)


def colsum(au, who, Y, y, M, N, partial, nblk, dtype, stream):
    au.span(who, "Y", Y, (last_row(y, M) + N) * es_of(dtype))
    au.span(who, "partial", partial, nblk * N * 4)


def classifier_ce_fwd(au, who, h, W, bias, labels, logits, sloss, loss, B, K, ncls, dtype, stream):
    au.span(who, "h", h, B * K * es_of(dtype))
    au.span(who, "W", W, ncls * K * 4)
    au.span(who, "bias", bias, ncls * 4)
    au.span(who, "labels", labels, B * 8, optional=True)
    au.span(who, "logits", logits, B * ncls * 4)
    au.span(who, "sample_loss", sloss, B * 4)
    au.span(who, "loss", loss, 4)


def classifier_ce_bwd(au, who, h, W, logits, labels, gloss, glogits, dlogits, dh, dW, db, B, K, ncls, use_gate, gate_scale, dtype,
                      stream):
    au.span(who, "h", h, B * K * es_of(dtype))
    au.span(who, "W", W, ncls * K * 4)
    au.span(who, "logits", logits, B * ncls * 4)
    au.span(who, "labels", labels, B * 8, optional=True)
    au.span(who, "gloss", gloss, 4, optional=True)
    assert au.span(who, "glogits", glogits, B * ncls * 4) == "glogits"                 # the one caller-owned temporary
    au.span(who, "dlogits", dlogits, B * ncls * 4)
    au.span(who, "dh", dh, B * K * es_of(dtype))
    au.span(who, "dW", dW, ncls * K * 4)
    au.span(who, "db", db, ncls * 4)


def pack_conv2d_weight(au, who, w, dst, N, Cin, transposed, dtype, stream):
    au.span(who, "w", w, N * Cin * 9 * 4)
    au.span(who, "dst", dst, N * Cin * 12 * es_of(dtype))                              # 3 x 4 taps, the fourth a zero pad


def pack_table(au, who, table, n, total_blocks, dtype, stream):
    assert au.span(who, "table", table, n * C.sizeof(L.PackEntry)) == "plan_dev"
    ents = (L.PackEntry * n).from_buffer_copy(bytes(au.eng._plan_dev.numpy())[: n * C.sizeof(L.PackEntry)])
    blk = 0
    for i, e in enumerate(ents):
        assert e.blk0 == blk and e.nblk > 0, (who, i)
        blk += e.nblk
        assert e.mode in (0, 1, 2), f"{who}: entry {i}: no extent formula for mode {e.mode}"
        au.span(who, f"entry {i} src", e.src, e.rows * e.cols * 4)
        # mode 0 / 2: rows * cols contiguous elements (2: fp32 copy); mode 1: dst[c * ldd + r]
        dst = ((e.cols - 1) * e.ldd + e.rows) * es_of(dtype) if e.mode == 1 else e.rows * e.cols * (4 if e.mode == 2 else es_of(dtype))
        au.span(who, f"entry {i} dst", e.dst, dst)
    assert blk == total_blocks


def conv2d_flat(au, who, inp, W, bias, out, Q, in_rows, rowpx, Wp, cin, nout, act, splits, dtype, stream):
    es = es_of(dtype)
    assert in_rows >= Q + 2 * rowpx + 2 and Q % rowpx == 0                             # the windows of Q pixel slots reach this far
    au.span(who, "in", inp, in_rows * cin * es)
    au.span(who, "W", W, nout * 12 * cin * es)
    au.span(who, "bias", bias, nout * 4, optional=True)
    au.span(who, "out", out, (Q // rowpx) * Wp * nout * es)                            # out[g * Wp + x][nout], g < Q / rowpx


def conv2d_wgrad_flat(au, who, d2, p1, partial, bias_partial, Q, p1_rows, rowpx, splits, dtype, stream):
    es = es_of(dtype)
    assert p1_rows >= Q + 2 * rowpx + 2
    au.span(who, "d2", d2, (Q + rowpx + 1) * 64 * es)                                  # d2[q + rowpx + 1], q < Q
    au.span(who, "p1", p1, p1_rows * 32 * es)
    assert splits * 64 * 384 <= au.eng.tn_cap
    au.span(who, "partial", partial, splits * 64 * 384 * 4)
    au.span(who, "bias_partial", bias_partial, splits * 64 * 4, optional=True)


FORMULAS = {
    "eg_spec_conv1_fwd": conv1_fwd,
    "eg_spec_conv1_bwd": conv1_bwd,
    "eg_spec_conv1_fwd_banded": lambda au, who, img, w, b, p1, nimg, F, nfr, band, dt, st:
        conv1_fwd(au, who, img, w, b, p1, nimg, F, nfr, dt, st, band_rows=band),
    "eg_spec_conv1_bwd_banded": lambda au, who, img, w, b, dp1, part, nimg, F, nfr, band, dt, st:
        conv1_bwd(au, who, img, w, b, dp1, part, nimg, F, nfr, dt, st, band_rows=band),
    "eg_gemm_nt": gemm_nt,
    "eg_gemm_tn": gemm_tn,
    "eg_spec_avgpool_fwd": avgpool_fwd,
    "eg_spec_avgpool_bwd": avgpool_bwd,
    "eg_reduce_partials": reduce_partials,
    "eg_unpack_conv2d_wgrad": unpack_conv2d_wgrad,
    "eg_colsum": colsum,
    "eg_classifier_ce_fwd": classifier_ce_fwd,
    "eg_classifier_ce_bwd": classifier_ce_bwd,
    "eg_pack_conv2d_weight": pack_conv2d_weight,
    "eg_pack_table": pack_table,
    "eg_conv2d_flat": conv2d_flat,
    "eg_conv2d_wgrad_flat": conv2d_wgrad_flat,
}


@pytest.fixture
def audit(monkeypatch):
    au = Audit(L.call)
    for m in (E, tokens, image_encoder):
        monkeypatch.setattr(m, "call", au)
    return au


def run(audit, B, F, W, dtype, d_model=64):
    model = image_encoder.GazeCNNEncoder(num_classes=3, d_model=d_model, compute_dtype=dtype)
    model._flat.ensure(CPU)
    eng = image_encoder.ImageEngine(model, B, F, W, CPU, DT[dtype])
    img, gl = torch.zeros(B, F, W), torch.ones(B, 3)
    audit.eng, audit.engines, audit.extra = eng, [("", eng)], [lambda: dict(glogits=gl)]
    audit.active = True
    eng.forward(img, img, True)
    eng.backward(gl)
    audit.active = False
    return eng


@pytest.mark.parametrize("B,F,W,dtype", CASES, ids=["B%d_%dx%d_%s" % c for c in CASES])
def test_every_launch_of_a_step_stays_inside_its_tensors(audit, B, F, W, dtype):
    eng = run(audit, B, F, W, dtype)
    sp, seen = eng.sp, audit.seen
    banded = F > 64
    assert (sp["band_rows"] > 0) == banded and sp["band_rows"] == L.spec_conv1_band_rows(F, W)
    assert sp["nbands"] == (-(-sp["Hp"] // sp["band_rows"]) if banded else 1)
    assert eng.g["sp_part"].shape == (2 * B * sp["nbands"], 320)
    conv1 = ["eg_spec_conv1_fwd_banded", "eg_spec_conv1_bwd_banded"] if banded else ["eg_spec_conv1_fwd", "eg_spec_conv1_bwd"]
    assert [n for n in seen if n.startswith("eg_spec_conv1")] == conv1
    # conv-2: the flat-correlation kernels only for 16-bit operands and narrow rows; else the segmented-row products
    flat = dtype != "f32" and 2 * (sp["Wp"] + 4) + 2 <= 64
    assert ("eg_conv2d_flat" in seen) == flat == (not banded)
    assert ("eg_gemm_tn" in seen) and ("eg_unpack_conv2d_wgrad" in seen)
    assert seen.count("eg_reduce_partials") >= 2
    # the two conv-1 reduces sum every (image, band) row
    rows = [r for r in audit.rows if r[0] == "eg_reduce_partials" and r[1][0] == "g.sp_part"]
    assert [(r[1][1], r[3], r[4], r[5]) for r in rows] == [(0, 288, 2 * B * sp["nbands"], 320), (288 * 4, 32, 2 * B * sp["nbands"], 320)]


def test_a_launch_without_a_formula_fails_by_name(audit):
    audit.engines, audit.extra, audit.active = [], [], True
    with pytest.raises(AssertionError, match="eg_gelu_fwd: the audit has no extent formula"):
        audit("eg_gelu_fwd", 0, 0, 0, L.EG_BF16, 0.0, 0, 0, 0)


def test_an_overrun_is_reported(audit):
    """the audit's own check: one float short of a conv-1 partial row is an overrun, a foreign pointer resolves to nothing"""
    eng = run(audit, 4, 64, 16, "bf16")
    audit._known = audit.known()
    sp = eng.g["sp_part"]
    audit.span("x", "partial", sp.data_ptr(), sp.numel() * 4)
    with pytest.raises(AssertionError, match="needs"):
        audit.span("x", "partial", sp.data_ptr() + 4, sp.numel() * 4)
    with pytest.raises(AssertionError, match="resolves to no engine tensor"):
        audit.span("x", "partial", torch.zeros(4).data_ptr(), 4)
