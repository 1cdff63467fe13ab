"""
TEST INFRASTRUCTURE -- the class-mean Grad-CAM maps of the reference (precedent: tests/make_golden_hd64.py).  Runs only where the
reference is mounted.  The reference's own compute_gradcam_batch (5_Metrics/eeg_metrics.py:811-953) runs on the reference model
(cfg5_a2_spec, synthetic weights) over the ten window pairs of tests/gradcam_ref.py::windows in batches of 4, 4 and 2.  The model and
the windows are taken to float64 first: in fp32 the gradient through six layers carries 1e-6 of noise that depends on the host's
thread count and instruction set (measured: 3e-7 .. 1.1e-6 of a map's maximum between machines, 1.5e-6 .. 3.6e-6 from the float64
value), which is the size of the gate the fixture is compared under; in float64 the fixture is the same on every machine.  Data
only: class means [3, 64, 64] (stored f32), counts, predictions and logits.

Usage:  python tests/make_golden_gradcam_means.py     -> tests/golden/gradcam_class_means.npz
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from oracle import make_golden as G  # noqa: E402
from oracle.dual_eeg_oracle import ModelCfg, synthetic_state_dict  # noqa: E402
from tests.gradcam_ref import NAMES, windows  # noqa: E402

BATCH = 4


def main():
    torch.set_num_threads(8)
    model_mod, _, _ = G.load_reference()
    spec = importlib.util.spec_from_file_location("reference_eeg_metrics", str(G.REF / "5_Metrics" / "eeg_metrics.py"))
    metrics = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(metrics)
    kw = G.CONFIGS["cfg5_a2_spec"]
    cfg = ModelCfg(**kw)
    model = model_mod.DualEEGTransformer(**kw)
    model.load_state_dict(synthetic_state_dict(cfg, G.WEIGHT_SEED), strict=True)
    model = model.double()
    z = np.load(REPO / "tests" / "golden" / "cfg5_a2_spec.npz", allow_pickle=False)
    x1, x2, y = windows(z)
    x1, x2 = x1.double(), x2.double()
    loader = [(x1[i:i + BATCH], x2[i:i + BATCH], y[i:i + BATCH]) for i in range(0, len(y), BATCH)]
    res = metrics.compute_gradcam_batch(model, loader, torch.device("cpu"), max_samples=100)
    model.eval()
    with torch.no_grad():
        logits = torch.cat([model(a, b)["logits"] for a, b, _ in loader])
    mean = np.stack([np.asarray(res.get(k, np.zeros((64, 64))), dtype=np.float32) for k in range(len(NAMES))])
    counts = np.array([int((y == k).sum()) for k in range(len(NAMES))], dtype=np.int64)
    out = REPO / "tests" / "golden" / "gradcam_class_means.npz"
    np.savez_compressed(out, class_mean=mean, class_count=counts, predictions=logits.argmax(1).numpy(), logits=logits.float().numpy(),
                        labels=y.numpy(), present=np.array(sorted(int(k) for k in res), dtype=np.int64))
    print("wrote", out, mean.shape, counts, out.stat().st_size)


if __name__ == "__main__":
    main()
