"""CPU-only: the attention statistics' semantics and C ABI.
  * tests/attn_stats_ref.py (the float64 restatement every GPU test of the feature compares with) against the reference's own
    extract_attention_weights (5_Metrics/eeg_metrics.py:465-594), loaded by file path and driven by a stub model that replays
    tests/golden/hooks.npz::xattn_probs through cross_attn.cross_attn.dropout; skipped where the reference tree is absent;
  * the header declares eg_attention_stats / eg_attention_stats_scratch_elems, _lib binds them, the ABI version is still 5;
  * every refusal of eg_attention_stats happens on the host, before any launch;
  * the scratch bound: at most max(S^2, 2^21) floats, far below the probabilities it replaces."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.attn_stats_ref import attn_stats_ref
from tests.helpers import GOLDEN

REPO = Path(__file__).resolve().parent.parent
WHO = "eg_attention_stats"


def _reference_metrics():
    from oracle.make_golden import REF
    path = REF / "5_Metrics" / "eeg_metrics.py"
    if not path.exists():
        pytest.skip("the reference tree is not present")
    pytest.importorskip("sklearn.metrics")
    pytest.importorskip("tqdm")
    spec = importlib.util.spec_from_file_location("reference_eeg_metrics", str(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Replay(torch.nn.Module):
    """model(eeg1, eeg2): eeg1 carries sample indices; the recorded probabilities of both directions pass through the hooked module"""

    def __init__(self, probs):
        super().__init__()
        self.cross_attn = torch.nn.Module()
        self.cross_attn.cross_attn = torch.nn.Module()
        self.cross_attn.cross_attn.dropout = torch.nn.Dropout(0.1)
        self.probs = torch.from_numpy(probs)

    def forward(self, eeg1, eeg2):
        idx = eeg1.long()
        self.cross_attn.cross_attn.dropout(self.probs[0][idx])
        self.cross_attn.cross_attn.dropout(self.probs[1][idx])
        return {}


@pytest.mark.parametrize("max_samples,count", [(200, 2), (1, 1)])
def test_restatement_matches_the_reference_function(max_samples, count):
    ref = _reference_metrics()
    probs = np.load(GOLDEN / "hooks.npz", allow_pickle=False)["xattn_probs"]          # [2 directions, 2 samples, H, S, S]
    labels = [2, 0]
    loader = [(torch.tensor([i]), torch.tensor([i]), torch.tensor([labels[i]])) for i in range(2)]
    want = ref.extract_attention_weights(_Replay(probs), loader, torch.device("cpu"), max_samples=max_samples)
    got = attn_stats_ref(probs[0], probs[1], labels, 1, max_samples)
    assert got["count"] == count and sum(v["count"] for v in want["diagonal_stats"].values()) == count
    err = np.abs(got["mean_map"] - want["mean_map"]).max()
    print(f"max_samples={max_samples}: mean_map |restatement - reference| = {err:.3g}")
    np.testing.assert_allclose(got["mean_map"], want["mean_map"], rtol=0, atol=1e-6)
    assert list(got["diagonal_stats"]) == list(want["diagonal_stats"]) == ["Cooperation", "Single"][:count]
    for name, w in want["diagonal_stats"].items():
        g = got["diagonal_stats"][name]
        assert g["count"] == w["count"]
        np.testing.assert_allclose(g["mean_diagonal_vector"], w["mean_diagonal_vector"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(g["mean_diagonal_value"], w["mean_diagonal_value"], rtol=0, atol=1e-6)


def test_header_declares_and_lib_binds_both_functions():
    from eyegaze_multimodal_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint64_t\s+eg_attention_stats_scratch_elems\s*\(\s*int NB, int S, int H\)", text)
    assert re.search(r"\bint\s+eg_attention_stats\s*\(", text)
    assert "#define EG_ABI_VERSION 5" in text and L.lib().eg_abi_version() == 5
    assert len(L.SIGNATURES["eg_attention_stats"]) == 13 and len(L.SIGNATURES["eg_attention_stats_scratch_elems"]) == 3
    assert all(L.exported_symbols()[n] for n in ("eg_attention_stats", "eg_attention_stats_scratch_elems"))


def _stats(NB=8, S=65, H=8, head_dim=32, kv_shift=4, dtype=None, qkv=0x1000, lse=0x1000, map_sum=0x1000, diag=0x1000,
           scratch=0x1000, scratch_elems=None):
    """the pointers are never dereferenced: every call below is refused before a launch"""
    from eyegaze_multimodal_amd import _lib as L
    if scratch_elems is None:
        scratch_elems = max(L.attn_stats_scratch_elems(NB, S, H), 0)
    L.call(WHO, qkv, lse, map_sum, diag, scratch, scratch_elems, NB, S, H, head_dim, kv_shift, L.EG_BF16 if dtype is None else dtype, 0)


def test_refusals_need_no_gpu():
    from eyegaze_multimodal_amd import _lib as L
    with pytest.raises(L.EgError, match=f"{WHO}: bad dtype 7"):                 # reported first: everything else is wrong too
        _stats(NB=7, S=0, head_dim=16, kv_shift=-1, dtype=7, qkv=0, scratch_elems=0)
    with pytest.raises(L.EgError, match=f"{WHO}: NB=7 must be even"):
        _stats(NB=7, kv_shift=3)
    for hd in (16, 128):
        with pytest.raises(L.EgError, match=f"{WHO}: head_dim={hd}"):
            _stats(head_dim=hd)
    with pytest.raises(L.EgError, match=f"{WHO}: bad shape"):
        _stats(S=0)
    with pytest.raises(L.EgError, match=f"{WHO}: S=2049 exceeds"):
        _stats(S=2049)
    for shift in (-1, 8):
        with pytest.raises(L.EgError, match=f"{WHO}: kv_shift={shift} out of range"):
            _stats(kv_shift=shift)
    for name in ("qkv", "lse", "map_sum", "diag", "scratch"):
        with pytest.raises(L.EgError, match=f"{WHO}: null pointer"):
            _stats(**{name: 0})
    need = L.attn_stats_scratch_elems(8, 65, 8)
    assert need > 0
    with pytest.raises(L.EgError, match=f"{WHO}: scratch holds {need - 1} floats, {need} are needed"):
        _stats(scratch_elems=need - 1)


@pytest.mark.parametrize("NB,S,H", [(2, 1, 2), (8, 65, 8), (256, 130, 8), (32, 2048, 8), (256, 2048, 8)])
def test_scratch_bound(NB, S, H):
    from eyegaze_multimodal_amd import _lib as L
    need = L.attn_stats_scratch_elems(NB, S, H)
    assert 0 <= need <= max(S * S, 1 << 21)
    if NB >= 32:
        assert need * 4 < NB * H * S * S * 4 / 8
    for bad in ((3, 65, 8), (0, 65, 8), (8, 0, 8), (8, 2049, 8), (8, 65, 0)):
        assert L.attn_stats_scratch_elems(*bad) == -1
