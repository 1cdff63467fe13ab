"""CPU-only, world_size 2 over gloo: gradient accumulation under data parallelism (ddp.AccumulatingReducer).
2 ranks x k = 2 micro-batches x 2 samples out of a global batch of 8, the CPU oracle as gradient provider (the HIP engine
cannot run without a GPU, so the accumulation takes the reducer's host branch: a torch add):
  * the accumulated, reduced and scaled gradient equals the oracle's gradient of all 8 samples (the gate of
    tests/test_ddp_gloo.py: mean-loss gradients of equal-sized shards recombine to rounding);
  * the group issues the collectives of ONE plain step, not k times that."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from eyegaze_multimodal_amd import DualEEGTransformer
from eyegaze_multimodal_amd.ddp import AccumulatingReducer, GradAllReducer, bucket_ranges, shard_indices
from oracle import dual_eeg_oracle as O

KW = dict(in_channels=8, max_len=256, num_classes=3, d_model=64, num_layers=2, num_heads=2, d_ff=128,
          use_spectrogram=False, use_ibs=False, use_cross_attention=True)
SEGMENTS = ["heads", "cross", "encoder.norm", "layer1", "layer0", "tokens", "conv1", "frontend"]  # order Engine.backward emits
K = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    torch.manual_seed(0)
    model = DualEEGTransformer(**KW)
    fp = model._flat
    fp.ensure(torch.device("cpu"))
    cfg = O.ModelCfg(**KW)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    Bg = 8
    x1, x2 = torch.randn(Bg, 8, 1024, generator=g), torch.randn(Bg, 8, 1024, generator=g)
    labels = torch.tensor([0, 1, 2, 1, 2, 0, 1, 0])
    mine = list(shard_indices(Bg, rank, world))             # 4 samples per rank, as K micro-batches of 2
    micro = [mine[i * 2:(i + 1) * 2] for i in range(K)]

    def grads(idx):
        P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        out = O.forward(x1[idx], x2[idx], P, cfg, labels[idx])
        out["loss_ce"].backward()
        return P

    def fill(P):                                            # what Engine.backward does: OVERWRITES the flat gradient buffer
        for n, p in zip(fp.names, fp.params):
            o = fp.offsets[n]
            fp.grad[o:o + p.numel()] = P[n].grad.reshape(-1)

    ranges = bucket_ranges(fp.names, fp.offsets, fp.total, KW["num_layers"], True)
    # one plain step (no accumulation) on the first micro-batch: the collective count to compare with
    fill(grads(micro[0]))
    plain = GradAllReducer(fp.grad, ranges)
    for s in SEGMENTS:
        plain.on_segment(s)
    plain.finish()
    # the accumulated group; the accumulator starts out poisoned: `first` must overwrite it
    acc = fp.accumulator()
    acc.fill_(float("nan"))
    red = AccumulatingReducer(fp.grad, acc, ranges)
    for j, idx in enumerate(micro):
        fill(grads(idx))
        if j < K - 1:
            red.accumulate(first=(j == 0))
            assert red.collectives == 0                     # non-final micro-steps issue no collective
        else:
            hook = red.final_hook(first=(j == 0))
            for s in SEGMENTS:
                hook(s)
            red.finish()
    got = acc * red.grad_scale(K)
    if rank == 0:
        Pfull = grads(list(range(Bg)))
        ref = torch.zeros_like(got)
        for n, p in zip(fp.names, fp.params):
            o = fp.offsets[n]
            ref[o:o + p.numel()] = Pfull[n].grad.reshape(-1)
        q.put((float((got - ref).abs().max()), float(ref.abs().max()), red.collectives, plain.collectives,
               red.grad_scale(K)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_times_two_micro_batches_equal_the_global_batch_gradient():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    err, scale, collectives, plain_collectives, gs = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert gs == 0.25
    assert err < 1e-5 * max(1.0, scale), (err, scale)
    assert plain_collectives > 0 and collectives == plain_collectives, (collectives, plain_collectives)


def test_flush_reduces_the_whole_accumulator_in_one_collective():
    """Single process, no process group: world == 1 issues nothing; the host branch still accumulates."""
    g = torch.arange(8, dtype=torch.float32)
    acc = torch.full((8,), float("nan"))
    red = AccumulatingReducer(g, acc, {"a": (0, 4), "b": (4, 8)})
    red.accumulate(first=True)
    g.mul_(2)
    hook = red.final_hook(first=False)
    hook("a")
    assert torch.equal(acc, torch.tensor([0., 3., 6., 9., 4., 5., 6., 7.]))
    hook("b")
    hook("unknown")                                         # segments outside the ranges are ignored, as by GradAllReducer
    red.flush()
    red.finish()
    assert torch.equal(acc, 3 * torch.arange(8, dtype=torch.float32)) and red.collectives == 0
    assert red.grad_scale(3) == 1.0 / 3
