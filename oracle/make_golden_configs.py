"""
TEST INFRASTRUCTURE — golden data for tests/test_reference_configs.py.  Runs ONLY in the build container (reference mounted
read-only, see oracle/make_golden.py).  It loads the reference's real yaml (4_Experiments/configs/dual_eeg_transformer.yaml),
derives every experiment config the way run_experiments.py does (EXPERIMENTS :47-233, create_experiment_config :242-275),
builds the REFERENCE model from each config exactly as train_art.py:360-385 does, and stores the resolved configs together
with that model's state_dict key order, tensor shapes and parameter count.  Data only; no reference source is copied.

Usage:  python oracle/make_golden_configs.py     -> tests/golden/reference_configs.json
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import yaml

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle.make_golden import REF, _load, load_reference  # noqa: E402

OUT = REPO / "tests" / "golden" / "reference_configs.json"


def reference_model(model_mod, cfg):
    """train_art.py:360-385, key for key"""
    ab, m, d, t = cfg.get("ablation", {}), cfg["model"], cfg["data"], cfg["training"]
    return model_mod.DualEEGTransformer(
        in_channels=m["in_channels"], num_classes=m["num_labels"], d_model=m["d_model"], num_layers=m["num_layers"],
        num_heads=m["num_heads"], d_ff=m["d_ff"], dropout=t["dropout"], max_len=d["window_size"] // 4,
        conv_kernel_size=m["conv_kernel_size"], conv_stride=m["conv_stride"], conv_layers=m["conv_layers"],
        sampling_rate=d["sampling_rate"], use_spectrogram=ab.get("use_spectrogram", True), spec_n_fft=m.get("spec_n_fft", 128),
        spec_hop_length=m.get("spec_hop_length", 64), spec_freq_bins=m.get("spec_freq_bins", 64),
        use_robust_ibs=(ab.get("ibs_mode", "robust") == "robust"), use_ibs=ab.get("use_ibs", True),
        use_cross_attention=ab.get("use_cross_attention", True), ibs_instance_norm=ab.get("ibs_instance_norm", True),
        ibs_feature_type=ab.get("ibs_feature_type", "all"))


def relative_paths(obj):
    """run_experiments.py resolves output_dir against its own location: store such paths relative to the reference root"""
    if isinstance(obj, dict):
        return {k: relative_paths(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [relative_paths(v) for v in obj]
    if isinstance(obj, str) and obj.startswith(str(REF) + "/"):
        return obj[len(str(REF)) + 1:]
    return obj


def main():
    model_mod, _, _ = load_reference()
    runner = _load("ref_run_experiments", REF / "run_experiments.py")
    base = yaml.safe_load((REF / "4_Experiments" / "configs" / "dual_eeg_transformer.yaml").read_text())
    entries = []
    for name, exp in [("base", {})] + list(runner.EXPERIMENTS.items()):
        cfg = runner.create_experiment_config(base, exp, name) if exp else base
        ref = reference_model(model_mod, cfg)
        sd = ref.state_dict()
        entries.append({"name": name, "config": relative_paths(cfg), "state_keys": list(sd),
                        "state_shapes": [list(v.shape) for v in sd.values()],
                        "num_parameters": sum(p.numel() for p in ref.parameters())})
    blob = {"n_experiments": len(runner.EXPERIMENTS), "entries": entries}
    OUT.write_text(json.dumps(blob, indent=1, sort_keys=False) + "\n")
    print(f"{OUT}: {len(entries)} configs")


if __name__ == "__main__":
    main()
