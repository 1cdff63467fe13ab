"""Pins the CPU oracle at attention head width 64 (d_model 128, 2 heads) against fixtures written by the reference
(tests/golden/hd64_*.npz, tests/make_golden_hd64.py), with the check functions of tests/test_oracle_golden.py.  CPU-only."""
import pytest

from tests import test_oracle_golden as TG
from tests.hd64_golden import HD64_CONFIGS, load_hd64


@pytest.fixture(autouse=True)
def hd64_loader(monkeypatch):
    monkeypatch.setattr(TG, "load_golden", load_hd64)


@pytest.mark.parametrize("name", HD64_CONFIGS)
def test_the_fixtures_are_64_wide(name):
    z, kw, cfg, sd = load_hd64(name)
    assert cfg.d_model // cfg.num_heads == 64 and cfg.d_model % cfg.num_heads == 0
    assert any(k.startswith("gen_eeg/") for k in z.files) and any(k.startswith("randn/") for k in z.files)


@pytest.mark.parametrize("name", HD64_CONFIGS)
@pytest.mark.parametrize("kind", ["randn", "gen_eeg"])
def test_forward_matches_reference(name, kind):
    TG.test_forward_matches_reference(name, kind)


@pytest.mark.parametrize("name", HD64_CONFIGS)
def test_gradients_and_step_match_reference(name):
    TG.test_gradients_and_step_match_reference(name)
