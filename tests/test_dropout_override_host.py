"""Host check of tests/helpers.py::hip_dropout_override: it serves EVERY dropout site the oracle names, on every golden
configuration, so that the train-mode parity tests (tests/test_gpu_model.py, tests/test_gpu_train_mode_tokens.py) can feed the
oracle the masks the kernels draw.  No GPU: only the oracle's train forward + backward run, under the override."""
import functools
import re
from pathlib import Path

import pytest
import torch

from oracle import dual_eeg_oracle as O
from tests.helpers import ALL_CONFIGS, ORACLE_SITE_KINDS, hip_dropout_override, load_golden, t

SEED = 0x1234_5678_9ABC


@functools.lru_cache(maxsize=None)
def _run(name):
    z, kw, cfg, sd = load_golden(name)
    x1, x2, lab = t(z["gen_eeg/eeg1"]), t(z["gen_eeg/eeg2"]), t(z["labels"])
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    log = {}
    O.DROPOUT_OVERRIDE = hip_dropout_override(SEED, x1.shape[0], cfg.num_layers, O.CTX, log=log)
    try:
        out = O.forward(x1, x2, params, cfg, lab, train=True)       # a KeyError here = a site the override does not serve
        loss = out["loss_ce"] + (0.5 * out["loss_ibs_cls"] if "loss_ibs_cls" in out else 0.0)
        loss.backward()
    finally:
        O.DROPOUT_OVERRIDE = None
    assert O.CTX["stream"] == 0
    assert torch.isfinite(loss)
    return cfg, log


def _expected_kinds(cfg):
    want = {"conv", "attn", "drop1", "ffn_a", "ffn_b", "drop2", "cls"}
    if cfg.use_cross_attention:
        want.add("xdrop1")
    if cfg.use_spectrogram:
        want.add("spec")
    if cfg.use_ibs:
        want |= {"ibscls", "ibstok" if cfg.use_robust_ibs else "ibsgen"}
    return want


@pytest.mark.parametrize("name", ALL_CONFIGS)
def test_override_serves_every_site_of_the_configuration(name):
    cfg, log = _run(name)
    assert {k[0] for k in log} == _expected_kinds(cfg)
    for key, (keep, pre) in log.items():
        assert keep.shape == pre.shape, key
        p = 0.3 if key[0] == "ibscls" else 0.1
        # binomial: sigma <= 0.5 / sqrt(n); six sigma and the 2^-16 granularity of the threshold
        assert abs(float((~keep).float().mean()) - p) < 3.0 / keep.numel() ** 0.5 + 1e-4, (key, float((~keep).float().mean()))
    # per-stream sites were drawn for both streams, the per-pair sites once
    for key in log:
        if key[0] in ("cls", "ibscls", "ibstok", "ibsgen"):
            assert key[-1] == 0, key
        else:
            assert key[:-1] + (1 - key[-1],) in log, key


@pytest.mark.parametrize("name", [n for n in ALL_CONFIGS if load_golden(n)[2].use_spectrogram])
def test_spec_masks_of_the_two_streams_differ(name):
    cfg, log = _run(name)
    k0, k1 = log[("spec", 0)][0], log[("spec", 1)][0]
    assert k0.shape == k1.shape and k0.shape[0] % cfg.in_channels == 0 and k0.shape[1] == 2 * cfg.d_model
    assert not torch.equal(k0, k1)
    # independent masks at p = 0.1 disagree on 2 * 0.1 * 0.9 = 18 % of the elements
    assert 0.12 < float((k0 != k1).float().mean()) < 0.24


def test_every_site_the_oracle_names_is_served():
    """the oracle's comment block above DROPOUT_OVERRIDE is the list; the configurations together reach all of it"""
    src = Path(O.__file__).read_text()
    block = src[src.index("# Train-mode dropout."): src.index("DROPOUT_OVERRIDE = None")]
    named = set(re.findall(r'\("(\w+)"', block))
    assert named == set(ORACLE_SITE_KINDS)
    served = set()
    for name in ALL_CONFIGS:
        served |= {k[0] for k in _run(name)[1]}
    assert served == named


def test_defects_change_only_their_site():
    """the negative controls' masks (tests/test_gpu_train_mode_tokens.py) differ from the true ones, and only at their site"""
    cfg, good = _run("a5_full")
    z, kw, cfg, sd = load_golden("a5_full")
    x1, x2, lab = t(z["gen_eeg/eeg1"]), t(z["gen_eeg/eeg2"]), t(z["labels"])
    for defect, site in (("spec_stream0", ("spec", 1)), ("ibstok_shift", ("ibstok", 0))):
        log = {}
        O.DROPOUT_OVERRIDE = hip_dropout_override(SEED, x1.shape[0], cfg.num_layers, O.CTX, log=log, defect=defect)
        try:
            with torch.no_grad():
                O.forward(x1, x2, sd, cfg, lab, train=True)
        finally:
            O.DROPOUT_OVERRIDE = None
        assert not torch.equal(log[site][0], good[site][0]), defect
        for key in ("conv", 0, 0), ("conv", 1, 1), ("spec", 0), ("ibscls", 0):
            assert torch.equal(log[key][0], good[key][0]), (defect, key)
