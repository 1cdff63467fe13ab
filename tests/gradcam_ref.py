"""TEST INFRASTRUCTURE -- CPU restatement of the reference's Grad-CAM analysis (5_Metrics/eeg_metrics.py:775-793, 811-953) on tap
tensors, and the float64 expectation of eg_gradcam_accumulate with its error bound.

  cams_from_taps      generate_cam on the two streams' activations / gradients, the channel mean, the stream mean, F.interpolate
  gradcam_ref         compute_gradcam_batch's loop over any per-batch runner: batches, the max_samples rule, class means by TRUE label
  oracle_runner       a per-batch runner over the project's oracle (O.forward with O.SPEC_CONV2_TAPS)
  hook_runner         a per-batch runner over the hook contract of a module (the HIP model's hook route, or the reference model)
  windows             N = 10 window pairs and labels derived from the four gen_eeg windows of a fixture (nothing new is stored)
  bilinear_matrix     F.interpolate(mode="bilinear", align_corners=False)'s weights as a matrix, computed in fp32 as torch does
  kernel_expectation  eg_gradcam_accumulate in float64 from the same input bits, with a bound for ANY order of fp32 accumulation
"""
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

LABELS = [0, 1, 2, 1, 0, 2, 2, 1, 0, 1]
NAMES = ["Single", "Competition", "Cooperation"]
OUT = 64
U = 2.0 ** -24          # unit roundoff of fp32


def windows(z):
    """10 window pairs from the 4 gen_eeg pairs of fixture z: pair i = scale_i * (window i % 4, reversed in time for odd i // 4)
    + 0.05 * CPU-generator noise (seed fixed); labels LABELS.  Returns eeg1, eeg2 [10, C, T] f32 and labels [10] i64."""
    x = [torch.from_numpy(np.ascontiguousarray(z[f"gen_eeg/eeg{s}"])).float() for s in (1, 2)]
    g = torch.Generator().manual_seed(20261020)
    scales = [1.0, 0.8, 1.25, 0.9, 1.1, 0.7, 1.3, 0.95, 1.05, 0.85]
    out = [[], []]
    for i, sc in enumerate(scales):
        for s in (0, 1):
            w = x[s][i % 4]
            if (i // 4) % 2 == 1:
                w = torch.flip(w, dims=[-1])
            out[s].append(sc * w + 0.05 * torch.randn(w.shape, generator=g))
    return torch.stack(out[0]).contiguous(), torch.stack(out[1]).contiguous(), torch.tensor(LABELS, dtype=torch.int64)


def cams_from_taps(act1, act2, grad1, grad2, B, C):
    """[B*C, 64, H, W] activations and gradients of the two streams -> [B, 64, 64] maps, operation for operation as
    compute_gradcam_batch does it (generate_cam :785-793, then :909-931)"""
    def generate_cam(activations, gradients):
        weights = torch.mean(gradients, dim=(2, 3), keepdim=True)
        cam = torch.sum(weights * activations, dim=1)
        return F.relu(cam).cpu().numpy()
    cam1, cam2 = generate_cam(act1, grad1), generate_cam(act2, grad2)
    cam1 = cam1.reshape(B, C, cam1.shape[1], cam1.shape[2])
    cam2 = cam2.reshape(B, C, cam2.shape[1], cam2.shape[2])
    cam_avg = (cam1.mean(axis=1) + cam2.mean(axis=1)) / 2.0
    cam_tensor = torch.from_numpy(cam_avg).unsqueeze(1)
    return F.interpolate(cam_tensor, size=(OUT, OUT), mode="bilinear", align_corners=False).squeeze(1).numpy()


def one_hot_of(logits, labels, target):
    idx = logits.argmax(dim=1) if target == "predicted" else labels.to(logits.device)
    return F.one_hot(idx, num_classes=logits.shape[1]).float()


def oracle_runner(sd, cfg):
    """run(x1, x2, y, target) -> (cams [B, 64, 64], logits, predictions) from the oracle's taps"""
    from oracle import dual_eeg_oracle as O

    def run(x1, x2, y, target):
        x1, x2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        O.SPEC_CONV2_TAPS = []
        try:
            logits = O.forward(x1, x2, sd, cfg)["logits"]
            (logits * one_hot_of(logits.detach(), y, target)).sum().backward()
            taps = O.SPEC_CONV2_TAPS
        finally:
            O.SPEC_CONV2_TAPS = None
        assert len(taps) == 2
        B, C = x1.shape[0], x1.shape[1]
        cams = cams_from_taps(taps[0].detach(), taps[1].detach(), taps[0].grad, taps[1].grad, B, C)
        return cams, logits.detach().numpy(), logits.detach().argmax(1).numpy()
    return run


def hook_runner(model):
    """run(x1, x2, y, target) over the hook contract of `model` (eeg_metrics.py:742-764, 856-907): parameters frozen, inputs
    require grad, a forward hook and a full backward hook on spectrogram_generator.spec_conv[3]; gradients arrive stream 2 first"""
    def run(x1, x2, y, target):
        dev = next(model.parameters()).device
        model.eval()
        flags = [p.requires_grad for p in model.parameters()]
        for p in model.parameters():
            p.requires_grad = False
        x1, x2 = x1.to(dev).clone().requires_grad_(True), x2.to(dev).clone().requires_grad_(True)
        acts, grads = [], []
        layer = model.spectrogram_generator.spec_conv[3]
        h1 = layer.register_forward_hook(lambda m, i, o: acts.append(o.detach()))
        h2 = layer.register_full_backward_hook(lambda m, gi, go: grads.append(go[0].detach()))
        try:
            model.zero_grad()
            logits = model(x1, x2)["logits"]
            (logits * one_hot_of(logits.detach(), y, target)).sum().backward()
        finally:
            h1.remove(), h2.remove()
            for p, f in zip(model.parameters(), flags):
                p.requires_grad = f
        assert len(acts) == 2 and len(grads) == 2
        B, C = x1.shape[0], x1.shape[1]
        cams = cams_from_taps(acts[0].float().cpu(), acts[1].float().cpu(), grads[1].float().cpu(), grads[0].float().cpu(), B, C)
        lg = logits.detach().float().cpu()
        return cams, lg.numpy(), lg.argmax(1).numpy()
    return run


def gradcam_ref(run, eeg1, eeg2, labels, batch_size, max_samples=100, target="predicted", names=NAMES):
    """compute_gradcam_batch's loop (:860-953) over `run`: max_samples is tested BEFORE each batch (None: all), the maps are
    bucketed by the true label and averaged with np.mean; a class that never occurred gets zeros and count 0"""
    by_class, cams, logits, preds, count = defaultdict(list), [], [], [], 0
    for i in range(0, eeg1.shape[0], batch_size):
        if max_samples is not None and count >= max_samples:
            break
        y = labels[i:i + batch_size]
        c, lg, pr = run(eeg1[i:i + batch_size], eeg2[i:i + batch_size], y, target)
        for k, lab in enumerate(y.tolist()):
            by_class[lab].append(c[k])
        cams.append(c), logits.append(lg), preds.append(pr)
        count += len(y)
    mean = {n: (np.mean(by_class[k], axis=0) if by_class.get(k) else np.zeros((OUT, OUT), np.float32)) for k, n in enumerate(names)}
    return {"class_mean": mean, "class_count": {n: len(by_class.get(k, [])) for k, n in enumerate(names)},
            "cams": np.concatenate(cams), "count": count, "logits": np.concatenate(logits), "predictions": np.concatenate(preds)}


# ------------------------------------------------------------------------------------------------
def bilinear_matrix(n_in: int, n_out: int = OUT) -> np.ndarray:
    """[n_out, n_in] float64 matrix of F.interpolate(mode="bilinear", align_corners=False) along one axis; the source index and
    the two weights are computed in fp32, step for step as upsample_bilinear2d does (area_pixel_compute_source_index: the source
    coordinate is clamped at 0)"""
    f = np.float32
    scale = f(n_in) / f(n_out)
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        src = f(f(scale * f(f(o) + f(0.5))) - f(0.5))
        src = f(0) if src < 0 else src
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = f(src - f(i0))
        l0 = f(f(1) - l1)
        m[o, i0] += float(l0)
        m[o, i1] += float(l1)
    return m


def resize_ref(a: np.ndarray) -> np.ndarray:
    """[..., H, W] float64 -> [..., 64, 64]"""
    return bilinear_matrix(a.shape[-2]) @ a @ bilinear_matrix(a.shape[-1]).T


def kernel_expectation(p1, d2, w2, b2, labels, B, C, Hp, Wp, ncls, grad_scale=None):
    """eg_gradcam_accumulate's outputs in float64 from the same input bits (p1 [2BC, Hp+2, Wp+4, 32], d2 [2BC, Hp+2, Wp+4, 64] in any
    dtype; w2 [64, 32, 3, 3], b2 [64] f32) and, beside each, a bound on what fp32 arithmetic may differ by in ANY order of
    accumulation.  A map pixel is, before the ReLU (1-Lipschitz), a sum of the products d2 * w2 * p1 / (Hp Wp) nested three deep:
    Hp Wp gradient pixels into a channel weight, 64 channels into a filter tap, 289 taps and bias into the pixel.  A sum of n terms
    rounds each term at most n - 1 times whatever its order, so a product passes through fewer than
    n = Hp Wp + 64 + 289 + 8 roundings (8: the mean's and the scale's divisions, the bias, the ReLU'd sum) and the error is at most
    n * 2^-24 * sum |products| -- narrower than (number of terms) * 2^-24 * sum |products|, which counts Hp Wp + 64 * 289 roundings.
    The means (C images, two streams), the resize (weights >= 0: the sum of |terms| is the value itself) and the class sums add
    their own terms' count times 2^-24 times their magnitude.
    Returns dict(cams, cams_bound [B, 64, 64], class_sum, class_bound [ncls, 64, 64], class_count [ncls])."""
    n, HW = 2 * B * C, Hp * Wp
    x = p1.double()[:, :, :Wp + 2].permute(0, 3, 1, 2)                  # the padded window the kernel reads: [n, 32, Hp+2, Wp+2]
    d = d2.double()[:, 1:Hp + 1, 1:Wp + 1]
    sc = 1.0 if grad_scale is None else float(grad_scale)
    wgt, wabs = d.mean(dim=(1, 2)) / sc, d.abs().mean(dim=(1, 2)) / sc       # [n, 64]
    w, b = w2.double(), b2.double()
    cam, mag = torch.empty(n, Hp, Wp, dtype=torch.float64), torch.empty(n, Hp, Wp, dtype=torch.float64)
    for i in range(0, n, 64):
        act = F.conv2d(x[i:i + 64], w, b)
        absact = F.conv2d(x[i:i + 64].abs(), w.abs(), b.abs())
        cam[i:i + 64] = torch.relu((wgt[i:i + 64, :, None, None] * act).sum(1))
        mag[i:i + 64] = (wabs[i:i + 64, :, None, None] * absact).sum(1)
    bound = (HW + 64 + 289 + 8) * U * mag
    m = cam.view(2, B, C, Hp, Wp).mean(2)
    mb = bound.view(2, B, C, Hp, Wp).mean(2) + (C + 2) * U * m
    a = ((m[0] + m[1]) / 2).numpy()
    ab = ((mb[0] + mb[1]) / 2).numpy() + 2 * U * a
    cams = resize_ref(a)
    cams_bound = resize_ref(ab) + 8 * U * cams
    lab = np.asarray(labels, dtype=np.int64)
    class_sum, class_bound, class_count = np.zeros((ncls, OUT, OUT)), np.zeros((ncls, OUT, OUT)), np.zeros(ncls, np.int64)
    for c in range(ncls):
        sel = lab == c
        class_count[c] = int(sel.sum())
        class_sum[c] = cams[sel].sum(0)
        class_bound[c] = cams_bound[sel].sum(0) + (class_count[c] + 2) * U * class_sum[c]
    return dict(cams=cams, cams_bound=cams_bound, class_sum=class_sum, class_bound=class_bound, class_count=class_count)
