"""Worker for tests/test_gpu_accum.py: one rank of a 2-rank data-parallel run on ONE GPU (gloo carries the collectives) with
gradient accumulation, k = 2 micro-batches per rank.  Real engine, real eg_grad_accumulate in the last micro-step's bucket
hook, the reducer built over the accumulator.  Rank 0 then runs the same four micro-batches as ONE process with k = 4."""
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import torch.distributed as dist

from eyegaze_multimodal_amd import DualEEGTransformer, HipAdamW
from eyegaze_multimodal_amd.data import randn_windows
from eyegaze_multimodal_amd.ddp import AccumulatingReducer, broadcast_params

K, MB = 2, 4


def main():
    out = Path(sys.argv[1])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    kw = dict(in_channels=8, num_classes=3, max_len=256, num_layers=2, use_spectrogram=False, use_ibs=False, use_cross_attention=True)
    torch.manual_seed(100 + rank)                      # different init per rank: broadcast must fix that
    model = DualEEGTransformer(**kw, compute_dtype="f32").to(dev)
    model.eval()                                       # deterministic step (no dropout): comparable with one process
    GB = world * K * MB
    x1, x2, y = randn_windows(GB, 8, 1024, seed=5, num_classes=3)
    micro = lambda r, j: slice((r * K + j) * MB, (r * K + j + 1) * MB)      # noqa: E731
    eng = model.engine(MB, 1024, dev)
    fp = model._flat
    broadcast_params(fp.flat)
    start = fp.flat.clone()
    opt = HipAdamW(model, lr=1e-3, weight_decay=0.01)
    red = AccumulatingReducer(fp.grad, fp.accumulator(), eng.bucket_ranges(), accumulate_fn=eng.accumulate)
    one = torch.ones(1, device=dev)
    before_last = None
    for j in range(K):
        first, last = j == 0, j == K - 1
        sl = micro(rank, j)
        opt.begin_step(eng, seed=j, grad_scale=red.grad_scale(j + 1), advance=first)
        eng.forward(x1[sl].to(dev), x2[sl].to(dev), y[sl].to(dev), train=False)
        if last:
            before_last = red.collectives
            eng.backward(gloss=one, on_segment=red.final_hook(first))
            red.finish()
        else:
            eng.backward(gloss=one)
            red.accumulate(first)
    torch.cuda.synchronize()
    g0 = (fp.acc * red.grad_scale(K)).clone()
    opt.step(eng, accumulated=True)
    torch.cuda.synchronize()
    mineflat = fp.flat.clone()
    other = mineflat.clone()
    dist.broadcast(other, src=0)
    res = {"rank": rank, "same_params_as_rank0": bool(torch.equal(other, mineflat)), "opt_t": opt.t,
           "collectives": red.collectives, "collectives_before_last_micro_step": before_last,
           "moved": float((mineflat - start).abs().max())}
    if rank == 0:
        # single process, k = 4 over the concatenated micro-batches, same starting parameters
        ref = DualEEGTransformer(**kw, compute_dtype="f32").to(dev)
        ref.eval()
        ref._flat.ensure(dev)
        ref._flat.flat.copy_(start)
        e2 = ref.engine(MB, 1024, dev)
        o2 = HipAdamW(ref, lr=1e-3, weight_decay=0.01)
        order = [(r, j) for r in range(world) for j in range(K)]
        for i, (r, j) in enumerate(order):
            sl = micro(r, j)
            o2.begin_step(e2, seed=i, grad_scale=1.0 / (i + 1), advance=(i == 0))
            e2.forward(x1[sl].to(dev), x2[sl].to(dev), y[sl].to(dev), train=False)
            e2.backward(gloss=one)
            e2.accumulate(first=(i == 0), norm=(i == len(order) - 1))
        torch.cuda.synchronize()
        gref = ref._flat.acc * (1.0 / len(order))
        res["grad_rel_err"] = float((g0 - gref).norm() / gref.norm())
        o2.step(e2, accumulated=True, norm_ready=True)
        torch.cuda.synchronize()
        res["param_rel_err_after_1_update"] = float((ref._flat.flat - mineflat).norm() / (mineflat - start).norm())
    (out / f"rank{rank}.json").write_text(json.dumps(res))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
