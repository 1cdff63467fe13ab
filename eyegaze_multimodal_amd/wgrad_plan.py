"""The encoder's grouped weight-gradient launch (eg_gemm_tn_grouped / eg_gemm_tn_grouped256 + eg_reduce_table) as host arithmetic on
explicit inputs: which products ride in it, tile and split counts, the device tables of the whole launch and of its data-parallel
pieces.  No launch is made here; Engine._wgrad_group_plan allocates the operands between layout() and plan() and caches the result."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Callable, Dict, Optional

import torch

from . import _lib as L

GROUP_SPLITS = 5        # row splits of the grouped launch on 128 x 128 tiles (288 tiles x 5 splits)
GROUP_SPLITS_256 = 3    # ... on 256 x 256 tiles (72 tiles x 3 row splits = 216 blocks, one round)


def packed(offsets: Dict[str, int], names, N: int, K: int) -> bool:
    """The product [N, K] feeds N/len(names) rows to each `name.weight` / `name.bias`: True when those (weight, bias) pairs sit
    back to back in the flat buffer (they do: registration order), so ONE reduce can write every weight and bias gradient."""
    P = N // len(names)
    base = offsets[names[0] + ".weight"]
    return all(offsets[n + ".weight"] == base + i * (P * K + P) and offsets[n + ".bias"] == base + i * (P * K + P) + P * K
               for i, n in enumerate(names))


def reduce_blocks(n: int, splits: int) -> int:
    """workgroups eg_reduce_table spends on one entry (include/eyegaze_hip.h: EG_REDUCE_WIDE_SPLITS = 8)"""
    cols = n // 4
    return (cols + 255) // 256 if splits <= 8 else (cols + 7) // 8


def layout(cfg, dtype: int, cus: int, offsets: Dict[str, int]) -> Optional[SimpleNamespace]:
    """The products of the grouped launch, (parameter prefixes, dY buffer, X buffer, N, K, ldy) each, with the tile, the split
    counts and the LayerNorm slots; None when the parameter layout does not allow the fused reduces."""
    d, F, Lr = cfg.d_model, cfg.d_ff, cfg.num_layers
    probs = []
    for l in range(Lr):
        pre = f"encoder.layers.{l}."
        probs += [([pre + "mha.out_proj"], f"dYo{l}", f"ctx{l}", d, d, d),
                  ([pre + "mha.q_proj", pre + "mha.k_proj", pre + "mha.v_proj"], f"dqkv{l}", f"x{l}", 3 * d, d, 3 * d),
                  ([pre + "ffn.linear2"], f"dYf{l}", f"hff{l}", d, F, d),
                  ([pre + "ffn.linear1"], f"dh{l}", f"y1_{l}", F, d, F)]
    ln_names = [f"encoder.layers.{l}.{n}" for l in range(Lr) for n in ("ln1", "ln2")]
    gain_bias = lambda n: offsets[n + ".bias"] == offsets[n + ".weight"] + d        # (gain | bias) back to back
    if not (all(packed(offsets, names, N, K) for names, _, _, N, K, _ in probs) and all(gain_bias(n) for n in ln_names)):
        return None
    # the two weight gradients of the cross-attention block ride in the same launch (their own dY buffers, as the layers have)
    cx = "cross_attn.cross_attn."
    cross = [([cx + "out_proj"], "dYo_x", "ctxx", d, d, d),
             ([cx + "q_proj", cx + "k_proj", cx + "v_proj"], "dqkv_x", "zn", 3 * d, d, 3 * d)]
    wg_cross = bool(cfg.use_cross_attention) and all(packed(offsets, names, N, K) for names, _, _, N, K, _ in cross)
    ncross = len(cross) if wg_cross else 0
    probs += cross[:ncross]
    # 16-bit dtypes: 256 x 256 tiles, one 512-thread workgroup per CU (72 tiles x 3 row splits = 216 blocks, one round);
    # otherwise 128 x 128 tiles, three 256-thread workgroups per CU (288 tiles x 5 splits)
    big = dtype != L.EG_F32 and all(N % 256 == 0 and K % 256 == 0 for _, _, _, N, K, _ in probs)
    splits = GROUP_SPLITS_256 if big else GROUP_SPLITS
    # data-parallel runs cut the launch in two pieces; with 256 x 256 tiles a piece has ~40 tiles, so it takes twice the
    # row splits to fill the chip (240 / 216 blocks) -- with the whole launch's 3 splits each piece ran on 45 % of the CUs
    # and the pair cost 0.42 ms more than the single launch
    piece_tiles = ((Lr - Lr // 2) * 12 + (4 if wg_cross else 0)) if big else 0
    splits_p = max(splits, cus // piece_tiles) if big and piece_tiles else splits
    # encoder.norm and cross_attn.norm get slots behind the layers': without a gradient reducer their gain / bias partials
    # ride in the whole-encoder reduce launch too (backward decides; with a reducer their buckets are released at once)
    tail_names = [n for n in ["encoder.norm"] + (["cross_attn.norm"] if cfg.use_cross_attention else []) if gain_bias(n)]
    return SimpleNamespace(probs=probs, ncross=ncross, wg_cross=wg_cross, big=big, tile=256 if big else 128, splits=splits,
                           splits_p=splits_p, smax=max(splits, splits_p), total=sum(N * K + N for _, _, _, N, K, _ in probs),
                           ln_names=ln_names, tail_names=tail_names,
                           ln_slot={n: i for i, n in enumerate(ln_names + tail_names)})


def plan(lay: SimpleNamespace, cfg, addr: Dict[str, int], wg_partial: int, lnpart_all: int, grad: int, offsets: Dict[str, int],
         ln_cap: int, ln_splits: Callable[[str], int], device) -> dict:
    """The tables of layout `lay`.  addr: device address of every dY / X buffer the products name; wg_partial / lnpart_all / grad:
    addresses of the split partials, the deferred LayerNorm partials ([slot, ln_cap, 2, d] floats) and the flat gradient buffer;
    ln_splits(name): partial rows that the backward of LayerNorm `name` leaves."""
    d, Lr, probs, tile = cfg.d_model, cfg.num_layers, lay.probs, lay.tile
    g_ptr = lambda name: grad + 4 * offsets[name]
    ln_of = {l: [(lay.ln_slot[n], n) for n in lay.ln_names[2 * l:2 * l + 2]] for l in range(Lr)}      # layer -> its (slot, ln1 / ln2)
    ln_tail = [(lay.ln_slot[n], n) for n in lay.tail_names]
    dev = lambda arr: torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    offs, off = [], 0
    for names, dyn, xn, N, K, ldy in probs:
        offs.append(off)
        off += lay.smax * (N * K + N)

    def tables(layers, with_cross=False, nsplit=None, with_tail=False):
        """TN problem table + reduce table (weights, biases and the deferred LayerNorm gain / bias partials) of `layers`
        (+ the cross-attention block's two products); block ranges are relative to the tables' own launches.  Which launch
        a product rides in does not change its result AT EQUAL nsplit (same row split, same ordered sum); the data-parallel
        pieces run with more row splits than the single launch (splits_p vs splits), so their gradients differ from the
        single launch's by fp32 summation order (~2e-6 relative), each arrangement deterministic in itself."""
        nsplit = nsplit or lay.splits
        sel = [4 * l + j for l in layers for j in range(4)]
        if with_cross:
            sel += [4 * Lr + j for j in range(lay.ncross)]
        lns = [e for l in layers for e in ln_of[l]] + (ln_tail if with_tail else [])
        tp = (L.TNProblem * len(sel))()
        rt = (L.ReduceEntry * (len(sel) + len(lns)))()
        blk = 0
        red = []        # (partial, out, n, splits) of the weight-gradient reduce entries
        for e, pi in zip(tp, sel):
            names, dyn, xn, N, K, ldy = probs[pi]
            base = wg_partial + 4 * offs[pi]
            e.dY, e.X, e.partial = addr[dyn], addr[xn], base
            e.ldy, e.ldx, e.N, e.K, e.part_rows, e.has_bias, e.blk0 = ldy, K, N, K, N // len(names), 1, blk
            blk += ((N + tile - 1) // tile) * ((K + tile - 1) // tile) * nsplit
            red.append((base, g_ptr(names[0] + ".weight"), N * K + N, nsplit))
        # deferred LayerNorm gain / bias partials ride in the same reduce launch.  Such an entry is 16 workgroups that walk
        # hundreds of short rows each, pure latency: they go FIRST in the table, so that they run under the streaming
        # weight-gradient entries instead of after them (with them last the 40-entry launch took 32.0 us against 27.7 us)
        lnred = [(lnpart_all + 4 * i * ln_cap * 2 * d, g_ptr(n + ".weight"), 2 * d, ln_splits(n)) for i, n in lns]
        rblk = 0
        for r, (part, out, n, nsp) in zip(rt, lnred + red):
            r.partial, r.out, r.n, r.stride, r.splits, r.blk0 = part, out, n, n, nsp, rblk
            rblk += reduce_blocks(n, nsp)
        return dict(tp=dev(tp), rt=dev(rt), n=len(sel), nr=len(sel) + len(lns), blocks=blk, rblocks=rblk, layers=list(layers),
                    splits=nsplit)

    whole = tables(range(Lr), with_cross=True)
    # data parallel: two pieces, so the gradient buckets of layers L-1 .. L/2 start their all-reduce while layers L/2-1 .. 0
    # are still in backward (one piece would hold every encoder bucket back until backward has finished)
    h = Lr // 2
    pieces = ([tables(range(h, Lr), with_cross=True, nsplit=lay.splits_p), tables(range(0, h), nsplit=lay.splits_p)]
              if Lr >= 2 else [whole])
    return dict(whole, splits=lay.splits, pieces=pieces, split_layer=h,
                whole_norms=tables(range(Lr), with_cross=True, with_tail=True) if ln_tail else None,
                entry="eg_gemm_tn_grouped256" if lay.big else "eg_gemm_tn_grouped")
