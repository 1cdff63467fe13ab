"""Exact t-SNE of model embeddings on the device: eeg_metrics.compute_tsne / FeatureExtractor.compute_tsne of the
reference, i.e. sklearn.manifold.TSNE(n_components=2, init="pca", method="exact"), restated in stages that are each a
deterministic function of their inputs:

    joint_probabilities   eg_tsne_sqdist -> eg_tsne_affinities -> eg_tsne_joint       (TSNE._fit: distances, _joint_probabilities)
    pca_init              the top two principal axes, exactly                          (TSNE._fit: PCA, rescaled to std 1e-4)
    tsne                  eg_tsne_gradient + eg_tsne_update per iteration              (TSNE._tsne: two phases of _gradient_descent)

The final coordinates are chaotic in the rounding of every step, so they are no yardstick; what a run is judged by is the KL
divergence it reaches.  The host reads the device once per N_ITER_CHECK iterations (the error and the gradient norm) and never in
between.  There is no CPU path: without the library's kernels every function here raises."""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Tuple

import numpy as np
import torch

from ._lib import TSNE_MAX_D, TSNE_MAX_N, call, ptr, tsne_workspace_bytes

EXPLORATION_ITER = 250          # TSNE._EXPLORATION_MAX_ITER: iterations of the early-exaggeration phase
N_ITER_CHECK = 50               # TSNE._N_ITER_CHECK: the error and the gradient norm are read every 50th iteration
MIN_GAIN = 0.01
CSV_COLUMNS = ["Sample_ID", "True_Label", "Pred_Label", "TSNE_1", "TSNE_2"]          # analyze_eeg.py:607-614


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _device_rows(X, what: str) -> torch.Tensor:
    X = torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X)
    if X.dim() != 2:
        raise ValueError(f"{what} needs an [N, D] array, got {tuple(X.shape)}")
    N, D = X.shape
    if not 2 <= N <= TSNE_MAX_N:
        raise ValueError(f"{what}: N={N} outside [2, {TSNE_MAX_N}]; pass fewer windows (max_samples)")
    if not 1 <= D <= TSNE_MAX_D:
        raise ValueError(f"{what}: D={D} outside [1, {TSNE_MAX_D}]")
    return X.to("cuda", torch.float32).contiguous()


def _workspace(N: int) -> torch.Tensor:
    return torch.empty(tsne_workspace_bytes(N), dtype=torch.uint8, device="cuda")


def joint_probabilities(X, perplexity: float = 30.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """TSNE._fit's P for method="exact": -> (P [N, N] f32, beta [N] f64, steps [N] i32), device tensors.  P is symmetric with a
    zero diagonal and sums to 1; beta_i is the precision the perplexity search ended at on row i, steps_i the number of times it
    moved beta (100: the search ran out).  perplexity must lie in (0, N)."""
    X = _device_rows(X, "joint_probabilities")
    N, D = X.shape
    if not 0 < perplexity < N:
        raise ValueError(f"joint_probabilities: perplexity={perplexity} outside (0, N={N})")
    dist = torch.empty(N, N, device="cuda")
    cond = torch.empty(N, N, device="cuda")
    beta = torch.empty(N, device="cuda", dtype=torch.float64)
    steps = torch.empty(N, device="cuda", dtype=torch.int32)
    ws = _workspace(N)
    call("eg_tsne_sqdist", ptr(X), N, D, ptr(dist), _stream())
    call("eg_tsne_affinities", ptr(dist), N, float(perplexity), ptr(cond), ptr(beta), ptr(steps), _stream())
    call("eg_tsne_joint", ptr(cond), N, ptr(ws), ws.numel(), ptr(dist), _stream())          # P over the distances' storage
    return dist, beta, steps


def pca_init(X, n_components: int = 2) -> torch.Tensor:
    """TSNE(init="pca")'s start with the exact principal axes (sklearn draws them from a randomized solver): X centred and X^T X
    in fp64 on the device, numpy.linalg.eigh of the D x D matrix, each axis signed so that its largest-magnitude entry is positive
    (sklearn's svd_flip), the projection rounded to float32 and rescaled to std(column 0) = 1e-4.  -> [N, n_components] f32 (device)"""
    X = _device_rows(X, "pca_init")
    if not 1 <= n_components <= min(X.shape):
        raise ValueError(f"pca_init: n_components={n_components} outside [1, {min(X.shape)}]")
    Xc = X.double()
    Xc = Xc - Xc.mean(dim=0, keepdim=True)
    _, V = np.linalg.eigh((Xc.T @ Xc).cpu().numpy())                   # ascending eigenvalues
    V = V[:, ::-1][:, :n_components]
    V = V * np.sign(V[np.abs(V).argmax(axis=0), np.arange(n_components)])
    emb = (Xc @ torch.from_numpy(np.ascontiguousarray(V)).to(Xc.device)).float()
    return emb / emb[:, 0].std(unbiased=False) * 1e-4


def descend(step, it: int, max_iter: int, n_iter_without_progress: int, min_grad_norm: float, n_iter_check: int = N_ITER_CHECK):
    """The loop and the two stop rules of sklearn's _gradient_descent.  step(i, check) runs iteration i; with check set -- every
    n_iter_check-th iteration and the last -- it returns (error, gradient norm), the one host sync.  Stops when the error has not
    improved for more than n_iter_without_progress iterations or the gradient norm is at most min_grad_norm.
    -> (the error of the last checked iteration, the index of the last iteration run)"""
    error = best_error = float(np.finfo(float).max)
    best_iter = i = it
    for i in range(it, max_iter):
        converge = (i + 1) % n_iter_check == 0
        check = converge or i == max_iter - 1
        res = step(i, check)
        if check:
            error = res[0]
        if converge:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if res[1] <= min_grad_norm:
                break
    return error, i


class Descent:
    """The state of one descent on the device: Y, update, gains, grad [N, 2] f32, stats [2] f64 and the workspace."""

    def __init__(self, P: torch.Tensor, Y0: torch.Tensor):
        self.P, self.N = P, P.shape[0]
        self.Y = Y0.to("cuda", torch.float32).contiguous().clone()
        self.grad = torch.empty_like(self.Y)
        self.stats = torch.zeros(2, device="cuda", dtype=torch.float64)
        self.ws = _workspace(self.N)
        self.reset()

    def reset(self):
        """update = 0, gains = 1: the start of every phase"""
        self.update, self.gains = torch.zeros_like(self.Y), torch.ones_like(self.Y)

    def step(self, exaggeration: float, momentum: float, learning_rate: float, check: bool):
        """one iteration; with check: -> (KL divergence of the exaggerated P, norm of the gain-scaled gradient), a host sync"""
        st = ptr(self.stats) if check else 0
        call("eg_tsne_gradient", ptr(self.Y), ptr(self.P), float(exaggeration), self.N, ptr(self.ws), self.ws.numel(), ptr(self.grad),
             st, _stream())
        call("eg_tsne_update", ptr(self.Y), ptr(self.update), ptr(self.gains), ptr(self.grad), self.N, float(momentum),
             float(learning_rate), MIN_GAIN, st, _stream())
        if check:
            kl, sq = self.stats.cpu().tolist()
            return kl, float(np.sqrt(sq))
        return None


def tsne(X, perplexity: float = 30.0, max_iter: int = 1000, init="pca", random_state: int = 42, early_exaggeration: float = 12.0,
         n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7, n_components: int = 2, P: torch.Tensor = None):
    """TSNE._fit + TSNE._tsne for method="exact" and learning_rate="auto" -> (Y [N, 2] f32 device tensor, kl_divergence, n_iter).
    perplexity is capped to N - 1 (FeatureExtractor.compute_tsne).  init: "pca" (pca_init), "random"
    (1e-4 * RandomState(random_state).standard_normal, sklearn's draw) or an [N, 2] array.  The first min(250, max_iter)
    iterations run at momentum 0.5 on early_exaggeration * P and give up after 250 iterations without progress, the rest at
    momentum 0.8 on P itself with n_iter_without_progress; update and gains start afresh in each phase.  kl_divergence is the
    divergence read at the last iteration run, n_iter that iteration's index (sklearn's kl_divergence_ and n_iter_).  sklearn
    refuses max_iter < 250; here such a run simply ends inside the first phase.  P: joint probabilities computed before
    (joint_probabilities(X, perplexity)[0]); X then only feeds the init."""
    if n_components != 2:
        raise ValueError(f"tsne maps into two components, not {n_components}")
    if max_iter < 1:
        raise ValueError(f"tsne: max_iter={max_iter} must be >= 1")
    X = _device_rows(X, "tsne")
    N = X.shape[0]
    if P is None:
        P = joint_probabilities(X, min(float(perplexity), N - 1))[0]
    elif tuple(P.shape) != (N, N) or P.dtype != torch.float32 or not P.is_cuda or not P.is_contiguous():
        raise ValueError(f"tsne: P must be a contiguous [N, N] = [{N}, {N}] f32 device tensor")
    if isinstance(init, str):
        if init == "pca":
            Y0 = pca_init(X, 2)
        elif init == "random":
            Y0 = torch.from_numpy(1e-4 * np.random.RandomState(random_state).standard_normal(size=(N, 2)).astype(np.float32))
        else:
            raise ValueError(f"tsne: init must be \"pca\", \"random\" or an [N, 2] array, got {init!r}")
    else:
        Y0 = torch.as_tensor(np.asarray(init) if not torch.is_tensor(init) else init)
        if tuple(Y0.shape) != (N, 2):
            raise ValueError(f"tsne: init must be [N, 2] = [{N}, 2], got {tuple(Y0.shape)}")
    lr = max(N / early_exaggeration / 4.0, 50.0)
    d = Descent(P, Y0)
    explore = min(EXPLORATION_ITER, max_iter)
    kl, it = descend(lambda i, check: d.step(early_exaggeration, 0.5, lr, check), 0, explore, EXPLORATION_ITER, min_grad_norm)
    if it + 1 < max_iter:
        d.reset()
        kl, it = descend(lambda i, check: d.step(1.0, 0.8, lr, check), it + 1, max_iter, n_iter_without_progress, min_grad_norm)
    return d.Y, kl, it


def write_tsne_csv(path, coords, y_true, y_pred, class_names) -> None:
    """tsne_<feature>.csv of run_embedding_analysis (analyze_eeg.py:607-614): Sample_ID, True_Label, Pred_Label, TSNE_1, TSNE_2"""
    coords = np.asarray(coords)
    name = lambda c: class_names[int(c)] if 0 <= int(c) < len(class_names) else str(int(c))
    with open(Path(path), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for i, (t, p) in enumerate(zip(y_true, y_pred)):
            w.writerow([i, name(t), name(p), repr(float(coords[i, 0])), repr(float(coords[i, 1]))])
