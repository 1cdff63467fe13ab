"""CPU-only: window augmentation's host surface -- eg_window_augment's refusals (they run before any launch; the pointers are
never dereferenced), WindowAugmentation's validation, the trainer's YAML key, and the numpy restatement's own properties
(tests/augment_ref.py; tests/test_gpu_augment.py holds the kernel to it)."""
import math

import numpy as np
import pytest

from tests import augment_ref as R

FAKE = 0x10000
OK = dict(in1=FAKE, in2=FAKE + 4096, out1=FAKE + 8192, out2=FAKE + 12288, N=2, C=3, T=64, noise_std=0.05, chan_drop_p=0.2,
          n_masks=2, mask_max_len=50, state=FAKE + 16384, stream=0)


def augment(**over):
    from eyegaze_multimodal_amd import _lib as L
    L.call("eg_window_augment", *{**OK, **over}.values())


@pytest.mark.parametrize("over, message", [
    (dict(in1=0), r"eg_window_augment: null pointer \(in1=\(nil\)"),
    (dict(in2=0), r"eg_window_augment: null pointer \(in1=0x10000 in2=\(nil\)"),
    (dict(out1=0), r"eg_window_augment: null pointer .*out1=\(nil\)"),
    (dict(out2=0), r"eg_window_augment: null pointer .*out2=\(nil\)"),
    (dict(state=0), r"eg_window_augment: null state"),
    (dict(N=0), r"eg_window_augment: bad shape N=0 C=3 T=64"),
    (dict(C=-1), r"eg_window_augment: bad shape N=2 C=-1 T=64"),
    (dict(T=0), r"eg_window_augment: bad shape N=2 C=3 T=0"),
    (dict(noise_std=-0.5), r"eg_window_augment: noise_std=-0\.5 must be finite and >= 0"),
    (dict(noise_std=math.inf), r"eg_window_augment: noise_std=inf must be finite and >= 0"),
    (dict(noise_std=math.nan), r"eg_window_augment: noise_std=-?nan must be finite and >= 0"),
    (dict(chan_drop_p=-0.25), r"eg_window_augment: chan_drop_p=-0\.25 outside \[0, 1\)"),
    (dict(chan_drop_p=1.0), r"eg_window_augment: chan_drop_p=1 outside \[0, 1\)"),
    (dict(chan_drop_p=math.nan), r"eg_window_augment: chan_drop_p=-?nan outside \[0, 1\)"),
    (dict(n_masks=-1), r"eg_window_augment: n_masks=-1 outside \[0, 8\]"),
    (dict(n_masks=9), r"eg_window_augment: n_masks=9 outside \[0, 8\]"),
    (dict(mask_max_len=0), r"eg_window_augment: mask_max_len=0 must be >= 1 when n_masks > 0"),
    (dict(N=1 << 16, C=1 << 8, T=1 << 7), r"eg_window_augment: 2\*N\*C\*T = 2\*65536\*256\*128 does not fit 32-bit element indices"),
    (dict(N=1 << 20, C=1 << 20, T=1), r"eg_window_augment: 2\*N\*C\*T = 2\*1048576\*1048576\*1 does not fit"),
])
def test_entry_point_refuses_by_message(over, message):
    from eyegaze_multimodal_amd import _lib as L
    with pytest.raises(L.EgError, match=message):
        augment(**over)


def test_binding_and_header_agree():
    import re
    from pathlib import Path
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import engine as E
    text = (Path(__file__).resolve().parent.parent / "include" / "eyegaze_hip.h").read_text()
    m = re.search(r"\bint\s+eg_window_augment\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == len(L.SIGNATURES["eg_window_augment"]) == 13
    assert L.exported_symbols()["eg_window_augment"]
    sites = {n: int(v) for n, v in re.findall(r"#define EG_SITE_AUG_(\w+)\s+(\d+)", text)}
    assert sites == dict(NOISE_R=E.SITE_AUG_NOISE_R, NOISE_T=E.SITE_AUG_NOISE_T, CHAN=E.SITE_AUG_CHAN, TIME=E.SITE_AUG_TIME)
    assert sites == dict(NOISE_R=R.SITE_AUG_NOISE_R, NOISE_T=R.SITE_AUG_NOISE_T, CHAN=R.SITE_AUG_CHAN, TIME=R.SITE_AUG_TIME)
    taken = {E.SITE_CONV0, E.SITE_CONV1, E.SITE_SPEC, E.SITE_IBSTOK, E.SITE_IBSGEN, E.SITE_CLS, E.SITE_IBSCLS}
    assert not taken & set(sites.values()) and max(sites.values()) < min(E._layer_sites(0).values())
    assert L.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------------------
# WindowAugmentation and the model attribute
# ------------------------------------------------------------------------------------------------------
def test_window_augmentation_defaults_and_enabled():
    from eyegaze_multimodal_amd import WindowAugmentation
    off = WindowAugmentation()
    assert (off.gaussian_noise_std, off.channel_dropout_prob, off.time_mask_max_length, off.time_mask_num) == (0.0, 0.0, 0, 0)
    assert not off.enabled
    assert not WindowAugmentation(time_mask_max_length=50).enabled           # a length without a count masks nothing
    assert WindowAugmentation(gaussian_noise_std=0.05).enabled
    assert WindowAugmentation(channel_dropout_prob=0.2).enabled
    assert WindowAugmentation(time_mask_max_length=50, time_mask_num=2).enabled
    assert WindowAugmentation(0.05, 0.2, 50, 2) == WindowAugmentation(gaussian_noise_std=0.05, channel_dropout_prob=0.2,
                                                                      time_mask_max_length=50, time_mask_num=2)


@pytest.mark.parametrize("kw, message", [
    (dict(gaussian_noise_std=-0.1), "gaussian_noise_std must be finite and >= 0"),
    (dict(gaussian_noise_std=math.inf), "gaussian_noise_std must be finite and >= 0"),
    (dict(gaussian_noise_std=math.nan), "gaussian_noise_std must be finite and >= 0"),
    (dict(gaussian_noise_std="0.05"), "gaussian_noise_std must be a number"),
    (dict(channel_dropout_prob=1.0), r"channel_dropout_prob must lie in \[0, 1\)"),
    (dict(channel_dropout_prob=-0.2), r"channel_dropout_prob must lie in \[0, 1\)"),
    (dict(channel_dropout_prob=math.nan), r"channel_dropout_prob must lie in \[0, 1\)"),
    (dict(time_mask_num=9, time_mask_max_length=5), r"time_mask_num must lie in \[0, 8\]"),
    (dict(time_mask_num=-1), r"time_mask_num must lie in \[0, 8\]"),
    (dict(time_mask_num=2.0, time_mask_max_length=5), "time_mask_num must be an integer"),
    (dict(time_mask_num=2, time_mask_max_length=0), "time_mask_max_length must be >= 1 when time_mask_num > 0"),
    (dict(time_mask_max_length=-3), "time_mask_max_length must be >= 1 when time_mask_num > 0, and never negative"),
    (dict(time_mask_max_length=True), "time_mask_max_length must be an integer"),
])
def test_window_augmentation_refuses(kw, message):
    from eyegaze_multimodal_amd import WindowAugmentation
    with pytest.raises(ValueError, match=message):
        WindowAugmentation(**kw)


def test_model_attribute_is_plain_and_outside_the_state_dict():
    import inspect
    from eyegaze_multimodal_amd import DualEEGTransformer, WindowAugmentation
    kw = dict(in_channels=8, max_len=256, use_spectrogram=False, use_ibs=False, num_layers=1)
    model = DualEEGTransformer(**kw)
    assert model.augmentation is None
    keys = list(model.state_dict())
    model.augmentation = WindowAugmentation(0.05, 0.2, 50, 2)
    assert list(model.state_dict()) == keys
    assert "augmentation" not in dict(model.named_buffers()) and "augmentation" not in dict(model.named_parameters())
    params = inspect.signature(DualEEGTransformer.__init__).parameters
    assert "augmentation" not in params and len(params) == 1 + 21 + 1     # self, the reference's 21 kwargs, compute_dtype


def _recorded_forward(monkeypatch, augmentation, train):
    """the launches of one forward of a CPU engine, recorded instead of issued (as profiles/tools/launch_trace.py does)"""
    import sys
    import torch
    import eyegaze_multimodal_amd as pkg
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd import _lib as L
    from eyegaze_multimodal_amd import tokens  # noqa: F401  (imported lazily by the model: it must be loaded to be patched)
    from eyegaze_multimodal_amd.engine import Engine
    rows, real = [], L.call

    def record(name, *args):
        rows.append((name, args))
        if name == "eg_pack_table_ex_check":
            real(name, *args)
    for name, mod in list(sys.modules.items()):
        if name.startswith(pkg.__name__) and getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", record)
    model = DualEEGTransformer(in_channels=8, max_len=256, use_spectrogram=True, use_ibs=True)
    model._flat.ensure(torch.device("cpu"))
    model.augmentation = augmentation
    eng = Engine(model, 4, 1024, torch.device("cpu"), L.EG_BF16)
    x1, x2, y = torch.zeros(4, 8, 1024), torch.zeros(4, 8, 1024), torch.zeros(4, dtype=torch.long)
    eng.forward(x1, x2, y, train=train)
    return eng, rows, (x1, x2)


def test_engine_issues_one_launch_and_hands_its_buffers_down(monkeypatch):
    from eyegaze_multimodal_amd import WindowAugmentation
    eng, rows, (x1, x2) = _recorded_forward(monkeypatch, WindowAugmentation(0.05, 0.2, 50, 2), train=True)
    names = [n for n, _ in rows]
    assert names.count("eg_window_augment") == 1
    i = names.index("eg_window_augment")
    assert names.index("eg_window_pack") == i + 1                   # the top of the front end: nothing reads the windows before
    buf = eng.a["aug"]
    assert tuple(buf.shape) == (2, 4, 8, 1024) and buf.dtype.is_floating_point and buf.element_size() == 4
    args = rows[i][1]
    assert args[:4] == (x1.data_ptr(), x2.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr())
    assert args[4:7] == (4, 8, 1024) and args[9:11] == (2, 50) and args[11] == eng.st_ptr
    assert args[7] == pytest.approx(0.05) and args[8] == pytest.approx(0.2)
    lo, hi = buf.data_ptr(), buf.data_ptr() + buf.numel() * 4
    readers = {n: a for n, a in rows[i + 1:] if n in ("eg_window_pack", "eg_stft_logmag")}
    assert set(readers) == {"eg_window_pack", "eg_stft_logmag"}
    for n, a in rows[i + 1:]:                                        # below the launch nobody is handed the caller's tensors
        assert x1.data_ptr() not in a and x2.data_ptr() not in a, n
    for n, a in readers.items():
        assert lo <= a[0] < hi, n


@pytest.mark.parametrize("augmentation, train", [(None, True), ("off", True), ("recipe", False)])
def test_engine_issues_nothing_when_off_or_in_eval(monkeypatch, augmentation, train):
    from eyegaze_multimodal_amd import WindowAugmentation
    aug = {None: None, "off": WindowAugmentation(), "recipe": WindowAugmentation(0.05, 0.2, 50, 2)}[augmentation]
    eng, rows, _ = _recorded_forward(monkeypatch, aug, train)
    assert "eg_window_augment" not in [n for n, _ in rows] and "aug" not in eng.a     # no launch, and no buffer either


def test_engine_refuses_a_foreign_augmentation_object(monkeypatch):
    from eyegaze_multimodal_amd import _lib as L
    with pytest.raises(L.EgError, match="model.augmentation must be a WindowAugmentation or None, got dict"):
        _recorded_forward(monkeypatch, dict(gaussian_noise_std=0.05), train=True)


# ------------------------------------------------------------------------------------------------------
# training.augmentation of the YAML
# ------------------------------------------------------------------------------------------------------
RECIPE = dict(gaussian_noise_std=0.05, channel_dropout_prob=0.2, time_mask_max_length=50, time_mask_num=2)


def test_yaml_absent_key_means_none():
    from eyegaze_multimodal_amd.train_art import augmentation_from_config
    assert augmentation_from_config({"training": {"dropout": 0.1}}) is None
    assert augmentation_from_config({"training": {"augmentation": None}}) is None
    assert augmentation_from_config({}) is None


def test_yaml_full_recipe():
    import yaml
    from eyegaze_multimodal_amd import WindowAugmentation
    from eyegaze_multimodal_amd.train_art import augmentation_from_config
    text = ("training:\n  augmentation:\n    gaussian_noise_std: 0.05\n    channel_dropout_prob: 0.2\n"
            "    time_mask_max_length: 50\n    time_mask_num: 2\n")
    aug = augmentation_from_config(yaml.safe_load(text))
    assert aug == WindowAugmentation(**RECIPE) and aug.enabled
    assert augmentation_from_config({"training": {"augmentation": {"gaussian_noise_std": 0.1}}}) == WindowAugmentation(0.1)


def test_yaml_unknown_key_is_named():
    from eyegaze_multimodal_amd.train_art import augmentation_from_config
    with pytest.raises(ValueError, match=r"training\.augmentation: unknown key 'time_shift'"):
        augmentation_from_config({"training": {"augmentation": dict(RECIPE, time_shift=8)}})
    with pytest.raises(ValueError, match="training.augmentation must be a mapping"):
        augmentation_from_config({"training": {"augmentation": [0.05, 0.2]}})
    with pytest.raises(ValueError, match=r"channel_dropout_prob must lie in \[0, 1\)"):
        augmentation_from_config({"training": {"augmentation": dict(RECIPE, channel_dropout_prob=1.5)}})


def test_yaml_all_zero_mapping_means_none():
    from eyegaze_multimodal_amd.train_art import augmentation_from_config
    zero = dict(gaussian_noise_std=0.0, channel_dropout_prob=0.0, time_mask_max_length=0, time_mask_num=0)
    assert augmentation_from_config({"training": {"augmentation": zero}}) is None
    assert augmentation_from_config({"training": {"augmentation": {}}}) is None


# ------------------------------------------------------------------------------------------------------
# the restatement itself.  Draws are deterministic in the seed: these seeds were picked once and checked to pass.
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, L, seed", [(100, 50, 11), (64, 200, 12)])
def test_restated_time_masks_stay_inside_the_window(T, L, seed):
    start, ln = R.time_masks(seed, 10000, T, 2, L)
    assert start.shape == ln.shape == (10000, 2)
    assert ln.min() == 1 and ln.max() == min(L, T)                 # both extremes occur
    assert (ln >= 1).all() and (ln <= min(L, T)).all()
    assert (start >= 0).all() and (start + ln <= T).all()
    assert start.min() == 0 and (start + ln).max() == T            # ... and both ends of the window are reached


def test_restated_noise_is_standard_normal():
    n = 1 << 20
    z = R.standard_normal(13, np.arange(n, dtype=np.uint64))
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5.0 / math.sqrt(n)                      # 5 standard errors
    assert abs(z.std() - 1.0) < 0.01
    # the two branches of a pair are uncorrelated, and the largest radius is sqrt(-2 ln 2^-24) = 5.77
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) < 5.0 / math.sqrt(n / 2)
    assert np.abs(z).max() <= math.sqrt(-2.0 * math.log(2.0 ** -24)) + 1e-12


def test_restated_channel_dropout_matches_hip_keep_mask_and_rate():
    from tests.helpers import hip_keep_mask
    N, C, T = 500, 8, 4
    z = R.zero_mask(14, N, C, T, 0.2, 0, 0)
    keep = hip_keep_mask(14, 10, np.arange(2 * N * C, dtype=np.uint32), 0.2).reshape(2, N, C)
    assert ((~z).all(-1) == keep).all() and (z.all(-1) == ~keep).all()         # whole rows, exactly the dropout mask of site 10
    rate = z[..., 0].mean()
    assert abs(rate - 0.2) < 5.0 * math.sqrt(0.2 * 0.8 / (2 * N * C))
    assert (z[0, ..., 0] != z[1, ..., 0]).any()                                 # the two players draw independently


def test_restated_transform_composes_zeros_over_noise():
    rng = np.random.default_rng(0)
    x1, x2 = rng.standard_normal((2, 3, 5, 101)).astype(np.float32)
    y, z = R.window_augment(x1, x2, 15, noise_std=0.05, chan_drop_p=0.5, n_masks=2, max_len=50)
    x = np.stack([x1, x2]).astype(np.float64)
    assert z.any() and not z.all() and (y[z] == 0.0).all()
    zt = R.zero_mask(15, 3, 5, 101, 0.0, 2, 50)
    assert zt.any() and (zt == zt[:1, :, :1, :]).all()            # time spans: the same for both players and every channel
    assert (z >= zt).all() and (z.all(-1) != zt.all(-1)).any()     # channel dropout adds whole rows on top
    d = (y - x)[~z] / 0.05
    assert 0.5 < d.std() < 1.5 and np.abs(d).max() < 5.8
    y0, z0 = R.window_augment(x1, x2, 15)
    assert not z0.any() and (y0 == x).all()
