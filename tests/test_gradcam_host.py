"""CPU-only: the device Grad-CAM route's semantics, C ABI and launch lists.
  * tests/gradcam_ref.py over the project's oracle against tests/golden/gradcam_class_means.npz, which the reference's own
    compute_gradcam_batch wrote (tests/make_golden_gradcam_means.py);
  * the bilinear restatement behind the kernel's expectation against F.interpolate;
  * every refusal of eg_gradcam_accumulate happens on the host, before any launch; the scratch query; the header and the binding;
  * the launches of Engine.backward(until="spec_conv2") and of a gradcam_statistics batch, recorded, not issued;
  * the argument checks of predict.gradcam_statistics / predict.embedding_features."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gradcam_ref as R
from tests.helpers import GOLDEN, load_golden

REPO = Path(__file__).resolve().parent.parent
BUF = torch.zeros(4096, dtype=torch.float32)      # host memory: its address stands in for every operand of a refused call
P = BUF.data_ptr()


def test_restatement_over_the_oracle_matches_the_reference_fixture():
    """batches of 4, 4 and 2 (the ragged tail), every class present; 1e-6 of each map's maximum.  Both sides run in float64 (the
    fixture's generator says why: fp32 noise of the gradient through six layers is as large as this gate and differs between
    hosts), so what is compared is the algorithm, and the figure is the same on every machine."""
    gz = np.load(GOLDEN / "gradcam_class_means.npz", allow_pickle=False)
    z, kw, cfg, sd = load_golden("cfg5_a2_spec")
    x1, x2, y = R.windows(z)
    assert y.tolist() == R.LABELS == gz["labels"].tolist() and x1.shape == (10, 8, 1024)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref = R.gradcam_ref(R.oracle_runner(sd, cfg), x1.double(), x2.double(), y, 4)
    assert ref["count"] == 10 and list(ref["class_count"].values()) == gz["class_count"].tolist() == [3, 4, 3]
    assert (ref["predictions"] == gz["predictions"]).all()
    for k, name in enumerate(R.NAMES):
        want = gz["class_mean"][k]
        err = np.abs(ref["class_mean"][name] - want).max()
        print(name, "max", want.max(), "difference", err)
        assert want.max() > 1e-5 and err <= 1e-6 * want.max()


def test_the_max_samples_rule_counts_whole_batches():
    z, kw, cfg, sd = load_golden("cfg5_a2_spec")
    x1, x2, y = R.windows(z)
    calls = []

    def run(a, b, yy, target):
        calls.append(len(yy))
        return np.zeros((len(yy), 64, 64), np.float32), np.zeros((len(yy), 3), np.float32), np.zeros(len(yy), np.int64)
    assert R.gradcam_ref(run, x1, x2, y, 4, max_samples=5)["count"] == 8 and calls == [4, 4]
    assert R.gradcam_ref(run, x1, x2, y, 4, max_samples=None)["count"] == 10
    assert R.gradcam_ref(run, x1, x2, y, 4, max_samples=8)["class_count"] == {"Single": 2, "Competition": 3, "Cooperation": 3}


@pytest.mark.parametrize("H,W", [(4, 4), (32, 8), (8, 68)])
def test_bilinear_restatement_equals_interpolate(H, W):
    """up- and downsampling; fp32 interpolation of non-negative data differs from the float64 product of the same fp32 weights by
    at most a few roundings of the value: 8 * 2^-24 of the largest input"""
    g = torch.Generator().manual_seed(H * 100 + W)
    a = torch.rand(3, 1, H, W, generator=g)
    want = F.interpolate(a, size=(64, 64), mode="bilinear", align_corners=False)[:, 0].double().numpy()
    got = R.resize_ref(a[:, 0].double().numpy())
    assert got.shape == (3, 64, 64) and np.abs(got - want).max() <= 8 * R.U * float(a.max())
    for n in (H, W):
        m = R.bilinear_matrix(n)
        assert m.shape == (64, n) and (m >= 0).all() and np.abs(m.sum(1) - 1).max() < 1e-6


def test_kernel_expectation_is_the_reference_algorithm_on_the_engine_s_layouts():
    """kernel_expectation (padded channel-last p1 / d2, images stream-major) against cams_from_taps fed conv-2's pre-ReLU output and
    the same gradient as [B*C, 64, H, W] taps: the layouts, the stream order and the resize agree; fp32 against float64"""
    B, C, Hp, Wp = 3, 2, 8, 12
    g = torch.Generator().manual_seed(5)
    n = 2 * B * C
    p1, d2 = torch.zeros(n, Hp + 2, Wp + 4, 32), torch.zeros(n, Hp + 2, Wp + 4, 64)
    p1[:, 1:Hp + 1, 1:Wp + 1] = torch.randn(n, Hp, Wp, 32, generator=g)
    d2[:, 1:Hp + 1, 1:Wp + 1] = torch.randn(n, Hp, Wp, 64, generator=g) * 1e-4
    w2, b2 = torch.randn(64, 32, 3, 3, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
    labels = [0, 2, 5]
    exp = R.kernel_expectation(p1, d2, w2, b2, labels, B, C, Hp, Wp, 3)
    act = F.conv2d(p1[:, 1:Hp + 1, 1:Wp + 1].permute(0, 3, 1, 2), w2, b2, padding=1)
    grad = d2[:, 1:Hp + 1, 1:Wp + 1].permute(0, 3, 1, 2).contiguous()
    want = R.cams_from_taps(act[:B * C], act[B * C:], grad[:B * C], grad[B * C:], B, C)
    assert np.abs(exp["cams"] - want).max() <= 2e-6 * want.max() and want.max() > 0
    assert (exp["cams_bound"] > 0).all() and exp["cams_bound"].max() < 5e-2 * want.max()
    assert exp["class_count"].tolist() == [1, 0, 1] and not exp["class_sum"][1].any()
    np.testing.assert_array_equal(exp["class_sum"][2], exp["cams"][1])
    scaled = R.kernel_expectation(p1, d2 * 1024, w2, b2, labels, B, C, Hp, Wp, 3, grad_scale=1024.0)
    np.testing.assert_allclose(scaled["cams"], exp["cams"], rtol=1e-12, atol=0)
    # the identity the kernel uses: one filter per image
    filt = torch.einsum("nc,cikl->nikl", d2.double()[:, 1:Hp + 1, 1:Wp + 1].mean(dim=(1, 2)), w2.double())
    x = p1.double()[:, 1:Hp + 1, 1:Wp + 1].permute(0, 3, 1, 2)
    one = torch.stack([F.conv2d(x[i:i + 1], filt[i:i + 1], padding=1)[0, 0] for i in range(n)])
    bias = d2.double()[:, 1:Hp + 1, 1:Wp + 1].mean(dim=(1, 2)) @ b2.double()
    cam = torch.relu(one + bias[:, None, None]).view(2, B, C, Hp, Wp).mean(2)
    np.testing.assert_allclose(R.resize_ref(((cam[0] + cam[1]) / 2).numpy()), exp["cams"], rtol=0, atol=1e-12 * want.max())


# ------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_two_functions():
    from eyegaze_multimodal_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint64_t\s+eg_gradcam_scratch_elems\s*\(int B, int C, int Hp, int Wp\)", text)
    assert re.search(r"\bint\s+eg_gradcam_accumulate\s*\(const void\* p1, const void\* d2, const float\* w2, const float\* b2, "
                     r"const float\* grad_scale,\s*const int64_t\* labels, float\* cams, float\* class_sum, int32_t\* class_count, "
                     r"float\* scratch,\s*int64_t scratch_elems, int B, int C, int Hp, int Wp, int ncls, int dtype, void\* stream\)", text)
    assert "#define EG_ABI_VERSION 5" in text and L.lib().eg_abi_version() == 5 and L.ABI_VERSION == 5
    assert len(L.SIGNATURES["eg_gradcam_accumulate"]) == 18 and len(L.SIGNATURES["eg_gradcam_scratch_elems"]) == 4
    assert all(L.exported_symbols()[n] for n in ("eg_gradcam_accumulate", "eg_gradcam_scratch_elems"))
    from eyegaze_multimodal_amd import build
    assert "gradcam.hip" in build.SOURCES


def _acc(p1=P, d2=P, w2=P, b2=P, grad_scale=0, labels=P, cams=P, class_sum=P, class_count=P, scratch=P, scratch_elems=None,
         B=4, C=8, Hp=32, Wp=8, ncls=3, dtype=None):
    from eyegaze_multimodal_amd import _lib as L
    if scratch_elems is None:
        scratch_elems = max(L.gradcam_scratch_elems(B, C, Hp, Wp), 0)
    L.call("eg_gradcam_accumulate", p1, d2, w2, b2, grad_scale, labels, cams, class_sum, class_count, scratch, scratch_elems,
           B, C, Hp, Wp, ncls, L.EG_BF16 if dtype is None else dtype, 0)


def test_accumulate_refusals_need_no_gpu():
    from eyegaze_multimodal_amd import _lib as L
    who = "eg_gradcam_accumulate"
    with pytest.raises(L.EgError, match=f"{who}: bad dtype 7"):                    # reported first: everything else is wrong too
        _acc(dtype=7, p1=0, B=0, Hp=3, ncls=99, scratch_elems=0)
    for name in ("p1", "d2", "w2", "b2", "labels", "cams", "class_sum", "class_count", "scratch"):
        with pytest.raises(L.EgError, match=f"{who}: null pointer"):
            _acc(**{name: 0})
    for bad in (dict(B=0), dict(C=0), dict(B=-1), dict(C=-3)):
        with pytest.raises(L.EgError, match=f"{who}: bad shape"):
            _acc(scratch_elems=0, **bad)
    for bad in (dict(Hp=0), dict(Wp=0), dict(Hp=6), dict(Wp=10), dict(Hp=-4), dict(Wp=33)):
        with pytest.raises(L.EgError, match=f"{who}: Hp=.* Wp=.* must be positive multiples of 4"):
            _acc(scratch_elems=0, **bad)
    for ncls in (0, 17, -1):
        with pytest.raises(L.EgError, match=rf"{who}: ncls={ncls} outside \[1, 16\]"):
            _acc(ncls=ncls)
    with pytest.raises(L.EgError, match=f"{who}: bad shape .*at most 4096 pixels"):
        _acc(Hp=64, Wp=68, scratch_elems=0)
    need = L.gradcam_scratch_elems(4, 8, 32, 8)
    with pytest.raises(L.EgError, match=f"{who}: scratch holds {need - 1} floats, {need} are needed"):
        _acc(scratch_elems=need - 1)
    with pytest.raises(L.EgError, match=f"{who}: p1 and d2 must be 16-byte aligned"):
        _acc(p1=P + 4)
    # grad_scale may be NULL: with everything else in order the call would launch, so only its refusals are checked here


@pytest.mark.parametrize("B,C,Hp,Wp", [(1, 1, 4, 4), (5, 3, 4, 8), (4, 8, 32, 8), (33, 8, 32, 8), (128, 32, 32, 8), (3, 2, 8, 68)])
def test_scratch_is_a_function_of_the_shapes(B, C, Hp, Wp):
    from eyegaze_multimodal_amd import _lib as L
    need = L.gradcam_scratch_elems(B, C, Hp, Wp)
    assert need == 2 * B * Hp * Wp                      # the channel means of both streams
    assert need <= 2 * B * C * Hp * Wp                  # never more than one fp32 map per image
    for bad in ((0, 8, 32, 8), (4, 0, 32, 8), (4, 8, 0, 8), (4, 8, 32, 0), (4, 8, 30, 8), (4, 8, 32, 6), (4, 8, 64, 68), (-1, 8, 32, 8)):
        assert L.gradcam_scratch_elems(*bad) == -1


# ---- launches recorded on the CPU (profiles/tools/launch_trace.py's Recorder: listed, not issued) ----
class _Rig:
    """a CPU training engine whose launches are recorded; spans of rows issued inside Engine.wgrad for the spectrogram projections
    and inside Engine._wgrad_group_launch are remembered"""

    def __init__(self, kw, dtype, B, T=1024):
        sys.path.insert(0, str(REPO / "profiles" / "tools"))
        from launch_trace import Recorder
        from eyegaze_multimodal_amd import DualEEGTransformer, _lib as L, engine as E, predict, tokens
        self.rec = rec = Recorder(L.call)
        self.saved = [(m, m.call) for m in (E, tokens, predict)]
        for m, _ in self.saved:
            m.call = rec
        self.model = model = DualEEGTransformer(**kw, compute_dtype=dtype)
        cpu = torch.device("cpu")
        self.eng = eng = model.engine(B, T, cpu)
        self.x = torch.zeros(B, model.cfg.in_channels, T)
        self.gl = torch.zeros(B, model.cfg.num_classes)
        self.gl[:, 1] = 1.0
        rec.engines, rec.extra = [("", eng)], [lambda: dict(x=self.x, glogits=self.gl)]
        self.proj, self.group = [], []
        wgrad, launch = eng.wgrad, eng._wgrad_group_launch

        def wg(*a, **k):
            i0 = len(rec.rows)
            wgrad(*a, **k)
            if (k.get("linear") or [""])[0].startswith("spectrogram_generator.proj."):
                self.proj.append((i0, len(rec.rows)))

        def gl_(*a, **k):
            i0 = len(rec.rows)
            launch(*a, **k)
            self.group.append((i0, len(rec.rows)))
        eng.wgrad, eng._wgrad_group_launch = wg, gl_
        # where the front end's backward begins, and inside it the spectrogram branch
        self.front = self.spec = None
        front, self.tokens, self.spec_bwd = eng._front_end_bwd, tokens, tokens.spec_cnn_backward

        def fe(*a, **k):
            self.front = len(rec.rows)
            front(*a, **k)

        def sb(*a, **k):
            self.spec = len(rec.rows)
            self.spec_bwd(*a, **k)
        eng._front_end_bwd, tokens.spec_cnn_backward = fe, sb

    def close(self):
        self.tokens.spec_cnn_backward = self.spec_bwd
        for m, c in self.saved:
            m.call = c

    def run(self, fn):
        self.rec.rows, self.proj, self.group, self.front, self.spec = [], [], [], None, None
        fn()
        return list(self.rec.rows), list(self.proj), list(self.group)


CASES = [("cfg5_a2_spec", "bf16", 4), ("cfg5_a2_spec", "f32", 4), ("a5_full", "bf16", 4), ("a5_full", "f32", 4),
         ("cfg5_a2_spec", "bf16", 32), ("a5_full", "bf16", 32)]       # B = 32: above GROUP_MIN_ROWS, the grouped launch exists


@pytest.mark.parametrize("name,dtype,B", CASES)
def test_analysis_backward_is_a_cut_of_the_full_launch_list(name, dtype, B, monkeypatch):
    from eyegaze_multimodal_amd import _lib as L, predict
    rig = _Rig(load_golden(name)[1], dtype, B)
    try:
        eng, x, gl = rig.eng, rig.x, rig.gl
        fwd = lambda: eng.forward(x, x, None, train=False)
        rig.run(fwd)                                            # (the first forward records the pack table, later ones replay it)
        fwd0, _, _ = rig.run(fwd)
        full, proj, group = rig.run(lambda: eng.backward(glogits=gl))
        front, spec = rig.front, rig.spec
        cut, proj_c, group_c = rig.run(lambda: eng.backward(glogits=gl, until="spec_conv2"))
        full2, _, _ = rig.run(lambda: eng.backward(glogits=gl))
        fwd1, _, _ = rig.run(fwd)
        assert full2 == full and fwd1 == fwd0                   # the cut leaves no switch behind
        assert len(proj) == 2 and not proj_c and not group_c
        grouped = eng._wg_plan is not None
        assert grouped == (len(group) == 1) and (grouped or B == 4)
        entry = eng._wg_plan["entry"] if grouped else None
        names = lambda rows: [r[0] for r in rows]
        end = names(full).index("eg_spec_avgpool_bwd")
        # removed: the two projection weight gradients, the grouped launch where the route has one, and what the front end's
        # backward issues before it reaches the spectrogram branch (the position / cls sums or eg_token_grad_tail, the synchrony
        # tokens' backward): "in _front_end_bwd, everything except the spectrogram branch"
        assert front is not None and front <= spec < end and rig.front is None
        gone = set(i for a, b in proj + group + [(front, spec)] for i in range(a, b))
        assert all(spec <= i < end for a, b in proj for i in (a, b - 1))
        before_spec = names(full[front:spec])
        assert "eg_token_grad_tail" in before_spec or "eg_batch_rowsum" in before_spec
        assert ("eg_gelu_bwd" in before_spec) == (name == "a5_full")
        want = [r for i, r in enumerate(full[:end + 1]) if i not in gone]
        assert cut == want                                      # names AND arguments, order kept
        assert names(cut)[-1] == "eg_spec_avgpool_bwd" and names(cut).count("eg_spec_avgpool_bwd") == 1
        removed = names([full[i] for i in sorted(gone)])
        assert set(removed) <= {"eg_gemm_tn", "eg_reduce_partials", "eg_colsum", "eg_reduce_table", entry, "eg_token_grad_tail",
                                "eg_batch_rowsum", "eg_cast", "eg_rows_gather_gate", "eg_gemm_nt", "eg_gelu_bwd", "eg_affine_grad"}
        if grouped:
            assert entry in ("eg_gemm_tn_grouped", "eg_gemm_tn_grouped256") and entry in names(full)
        for banned in ("eg_gemm_tn_grouped", "eg_gemm_tn_grouped256", "eg_reduce_table", "eg_conv2d_wgrad_flat", "eg_spec_conv1_bwd",
                       "eg_token_grad_tail", "eg_unpack_conv2d_wgrad", "eg_unpack_conv_wgrad", "eg_gemm_nt_batch", "eg_batch_rowsum",
                       "eg_rows_gather_gate", "eg_gelu_bwd", "eg_affine_grad"):
            assert banned not in names(cut), banned
        # conv-1's backward-data and the front end's weight gradients come after eg_spec_conv1_bwd in the full list
        tail = names(full)[end + 1:]
        assert "eg_spec_conv1_bwd" in tail and tail.count("eg_gemm_tn") >= 2 and ("eg_gemm_nt_batch" in tail or "eg_gemm_nt" in tail)
        # a gradcam_statistics batch: the eval forward, the cut, one eg_gradcam_accumulate
        y = torch.zeros(B, dtype=torch.int64)
        cams, cs, cc = torch.zeros(B, 64, 64), torch.zeros(3, 64, 64), torch.zeros(3, dtype=torch.int32)
        scratch = torch.zeros(L.gradcam_scratch_elems(B, eng.C, eng.sp["Hp"], eng.sp["Wp"]))
        count = rig.model._fwd_count
        batch, _, _ = rig.run(lambda: predict._gradcam_batch(rig.model, eng, x, x, y, "label", cams, cs, cc, scratch, 3))
        assert rig.model._fwd_count == count + 1                # the bookkeeping that refuses an older forward's backward
        assert names(batch) == names(fwd0) + names(cut) + ["eg_gradcam_accumulate"]
        assert names(batch).count("eg_gradcam_accumulate") == 1
        row = batch[-1]
        assert row[1] == ["a.sp_p1", 0] and row[2] == ["g.sp_d2", 0] and row[5] == (0 if dtype != "fp16" else row[5])
        assert row[12:18] == [B, eng.C, eng.sp["Hp"], eng.sp["Wp"], 3, eng.dtype]
    finally:
        rig.close()


def test_fp16_hands_the_kernel_the_device_loss_scale():
    from eyegaze_multimodal_amd import _lib as L, predict
    rig = _Rig(load_golden("cfg5_a2_spec")[1], "fp16", 4)
    try:
        eng = rig.eng
        assert eng.scaler_on
        y = torch.zeros(4, dtype=torch.int64)
        scratch = torch.zeros(L.gradcam_scratch_elems(4, eng.C, eng.sp["Hp"], eng.sp["Wp"]))
        batch, _, _ = rig.run(lambda: predict._gradcam_batch(rig.model, eng, rig.x, rig.x, y, "predicted", torch.zeros(4, 64, 64),
                                                            torch.zeros(3, 64, 64), torch.zeros(3, dtype=torch.int32), scratch, 3))
        assert batch[-1][0] == "eg_gradcam_accumulate" and batch[-1][5] == ["state", 32]       # word 8 of eg_step_state
        assert not any(r[0] in ("eg_scaler_update", "eg_clip_coef", "eg_set_step_state", "eg_adamw") for r in batch)
    finally:
        rig.close()


def test_backward_refuses_an_unknown_cut_and_a_model_without_spectrogram():
    from eyegaze_multimodal_amd import _lib as L
    rig = _Rig(load_golden("cfg3_xattn")[1], "bf16", 4)
    try:
        with pytest.raises(L.EgError, match="until='conv1'"):
            rig.eng.backward(glogits=rig.gl, until="conv1")
        with pytest.raises(L.EgError, match="needs a model with spectrogram tokens"):
            rig.eng.backward(glogits=rig.gl, until="spec_conv2")
    finally:
        rig.close()


def test_argument_checks_of_the_two_public_calls():
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.predict import embedding_features, gradcam_statistics
    model = DualEEGTransformer(**load_golden("cfg5_a2_spec")[1])
    x, y = torch.zeros(4, 8, 1024), torch.zeros(4, dtype=torch.long)
    for fn in (gradcam_statistics, embedding_features):
        with pytest.raises(ValueError, match="N >= 1"):
            fn(model, x[:0], x[:0], y[:0])
        with pytest.raises(ValueError, match="batch_size >= 1"):
            fn(model, x, x, y, batch_size=0)
        with pytest.raises(ValueError, match="labelled windows"):
            fn(model, x, x, y[:3])
        with pytest.raises(ValueError):
            fn(model, x, x, None)
    with pytest.raises(ValueError, match="max_samples"):
        gradcam_statistics(model, x, x, y, max_samples=0)
    with pytest.raises(ValueError, match="1 to 16 class names"):
        gradcam_statistics(model, x, x, y, class_names=[str(i) for i in range(17)])
    with pytest.raises(ValueError, match="1 to 16 class names"):
        gradcam_statistics(model, x, x, y, class_names=[])
    for bad in ("true", None, 1):
        with pytest.raises(ValueError, match="target must be one of"):
            gradcam_statistics(model, x, x, y, target=bad)


def test_a_model_without_spectrogram_returns_an_empty_dict():
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.predict import gradcam_statistics
    model = DualEEGTransformer(**load_golden("cfg3_xattn")[1])
    x, y = torch.zeros(4, 8, 1024), torch.zeros(4, dtype=torch.long)
    assert gradcam_statistics(model, x, x, y) == {}
    with pytest.raises(ValueError, match="target"):              # the arguments are still checked
        gradcam_statistics(model, x, x, y, target="other")


def test_the_command_line_has_the_two_flags():
    text = (REPO / "eyegaze_multimodal_amd" / "predict.py").read_text()
    assert '"--gradcam"' in text and '"--gradcam-max-samples", type=int, default=100' in text
    assert "gradcam_class_{k}_mean" in text and "gradcam_class_count" in text
