"""CPU-only: gradient accumulation's host surface -- eg_grad_accumulate's argument refusals (they run before any launch, the
pointers below are never dereferenced), its declaration and binding, and the parsing of training.gradient_accumulation_steps."""
import re
from pathlib import Path

import pytest

from eyegaze_multimodal_amd import _lib as L

REPO = Path(__file__).resolve().parent.parent
FAKE = 0x10000          # 16-B aligned, never dereferenced


def test_null_buffers_are_refused():
    with pytest.raises(L.EgError, match="eg_grad_accumulate: bad arguments"):
        L.call("eg_grad_accumulate", 0, FAKE, 1024, 1, 0, 0, 0)
    with pytest.raises(L.EgError, match="eg_grad_accumulate: bad arguments"):
        L.call("eg_grad_accumulate", FAKE, 0, 1024, 0, 0, 0, 0)


@pytest.mark.parametrize("n", [0, -4, 6, 1023])
def test_length_must_be_a_positive_multiple_of_four(n):
    with pytest.raises(L.EgError, match="eg_grad_accumulate: bad arguments"):
        L.call("eg_grad_accumulate", FAKE, FAKE + 4096, n, 1, 0, 0, 0)


@pytest.mark.parametrize("acc,g", [(FAKE + 4, FAKE + 4096), (FAKE, FAKE + 4096 + 8)])
def test_both_pointers_must_be_16_byte_aligned(acc, g):
    with pytest.raises(L.EgError, match="eg_grad_accumulate: alignment"):
        L.call("eg_grad_accumulate", acc, g, 1024, 0, 0, 0, 0)


@pytest.mark.parametrize("nblk", [0, -1, 1025, 4096])
def test_norm_partials_need_a_block_count_in_range(nblk):
    with pytest.raises(L.EgError, match=r"eg_grad_accumulate: bad arguments \(nblk=-?\d+ outside \[1, 1024\]\)"):
        L.call("eg_grad_accumulate", FAKE, FAKE + 4096, 1024, 0, FAKE + 8192, nblk, 0)


def test_header_declares_and_binding_lists_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+eg_grad_accumulate\s*\(([^)]*)\)", text)
    assert m, "include/eyegaze_hip.h does not declare eg_grad_accumulate"
    assert len(m.group(1).split(",")) == 7
    assert len(L.SIGNATURES["eg_grad_accumulate"]) == 7
    assert L.exported_symbols()["eg_grad_accumulate"]
    assert re.search(r"#define\s+EG_ABI_VERSION\s+5\b", text) and L.ABI_VERSION == 5      # purely additive


def test_accumulation_key_parsing():
    from eyegaze_multimodal_amd.train_art import accumulation_steps
    assert accumulation_steps({"training": {}}) == 1
    assert accumulation_steps({}) == 1
    assert accumulation_steps({"training": {"gradient_accumulation_steps": 1}}) == 1
    assert accumulation_steps({"training": {"gradient_accumulation_steps": 4}}) == 4
    for bad in (0, -2, 1.5, "x"):
        with pytest.raises(ValueError, match="training.gradient_accumulation_steps"):
            accumulation_steps({"training": {"gradient_accumulation_steps": bad}})


def test_accumulator_is_lazy_and_dropped_on_reflatten():
    import torch
    from eyegaze_multimodal_amd import DualEEGTransformer
    model = DualEEGTransformer(in_channels=8, max_len=256, num_layers=1, use_spectrogram=False, use_ibs=False)
    fp = model._flat
    fp.ensure(torch.device("cpu"))
    assert fp.acc is None                                   # never allocated while accumulation is unused
    acc = fp.accumulator()
    assert acc.shape == fp.grad.shape and acc.dtype == torch.float32 and fp.accumulator() is acc
    for p in model.parameters():                            # parameters re-created: the next ensure() re-flattens
        p.data = p.data.clone()
    fp.ensure(torch.device("cpu"))
    assert fp.acc is None
