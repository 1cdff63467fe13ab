"""In-kernel time stamps for the head launches (csrc/heads.hip): where inside a launch the time goes.

    python tools/diag/stamp_builds.py build            # no GPU needed: writes build/diag/libeyegaze_hip_stamps.so
    python tools/diag/stamp_builds.py run [out.txt]    # on the GPU: a few training steps at B = 256, bf16, then the table

`build` copies heads.hip, puts an EG_STAMP(kernel, slot) statement before / after the source lines named in STAMPS, compiles that
copy and links it with the product's other objects into a DIAGNOSTIC library.  The product library never contains a stamp: nothing in
csrc/ knows about them, and a STAMPS entry whose line is no longer in the source stops the build instead of stamping somewhere else.

A stamp is thread 0 of a workgroup, once its wave's outstanding loads and stores have completed (s_waitcnt 0), storing
wall_clock64() (the 100 MHz constant clock: 10 ns) into a __device__ array at [kernel][slot][blockIdx.x].  `run` reads the array after each step and prints, per kernel and slot, when the workgroups passed it,
in microseconds after the launch's FIRST workgroup passed slot 0: the median workgroup and the last one (the last is what the launch
waits for), medians over the steps.  Add ~5 us (launch to first workgroup, last workgroup to completion) to compare with a trace.
The stamps cost a wait and a store each, so the stamped launches run somewhat slower than the product's."""
from __future__ import annotations

import ctypes as C
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
OUT = REPO / "build" / "diag"
LIB = OUT / "libeyegaze_hip_stamps.so"
NK, NS, NB = 8, 16, 512

PRELUDE = f"""
__device__ unsigned long long eg_diag_stamps[{NK} * {NS} * {NB}];
#define EG_STAMP(kid, slot) do {{ __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0); \\
  if (threadIdx.x == 0) eg_diag_stamps[((kid) * {NS} + (slot)) * {NB} + blockIdx.x] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); }} while (0)
extern "C" int eg_diag_stamps_read(unsigned long long* dst) {{
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(eg_diag_stamps), sizeof(eg_diag_stamps));
}}
extern "C" int eg_diag_stamps_clear() {{
  static unsigned long long zeros[{NK} * {NS} * {NB}];
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(eg_diag_stamps), zeros, sizeof(zeros));
}}
"""

# kernel id -> (name, the line that opens its definition, [(slot expression, label, "before" | "after", source line, occurrence)]);
# lines are compared stripped, searched from the opening line on.
FIRST = "const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;"
STAMPS = {
    0: ("heads_fwd_sf", "__global__ __launch_bounds__(256) void heads_fwd_sf_kernel(HeadsFwd<T> p) {", [
        ("0", "start", "after", FIRST, 1),
        ("1", "fragments arrived, MFMAs done", "after", "for (int e = 0; e < 4; ++e) v[e] = acc[e] + bv[e];", 1),
        ("2", "zf stored (complete)", "after", "if (m < p.B) store4(p.zf + (size_t)m * HK + n, v);", 1)]),
    1: ("heads_fwd_cls", "__global__ __launch_bounds__(256) void heads_fwd_cls_kernel(HeadsFwd<T> p) {", [
        ("0", "start", "after", "const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;", 1),
        ("1", "product done, hcl stored (complete)", "before", "if (!last_arrival(p.counter + 1 + grp, HD / HSL, &last_s)) return;", 1),
        ("2", "group counter passed (last of 4 only from here)", "after", "if (!last_arrival(p.counter + 1 + grp, HD / HSL, &last_s)) return;", 1),
        ("3", "16 rows of hcl in LDS", "after", "__syncthreads();", 1),
        ("4", "class projection + CE of wave 0's rows", "before", "if (!p.labels || !last_arrival(p.counter, ngrp, &last_s)) return;", 1),
        ("5", "launch counter passed (last group only)", "after", "if (!p.labels || !last_arrival(p.counter, ngrp, &last_s)) return;", 1),
        ("6", "mean stored", "after", "block_mean256<true>(p.sloss, p.loss, p.B, red);", 1)]),
    2: ("classifier_ce_bwd_fused", "__device__ __forceinline__ void classifier_ce_bwd_fused_body(const T* __restrict__ h, const float* __restrict__ W,", [
        ("0", "start", "after", "const int lane = threadIdx.x & 63, bl = threadIdx.x >> 6;", 1),
        ("1", "row blocks: dlogits + dh rows stored", "before", "return;", 1),
        ("2", "weight blocks: h slice + dlogits in LDS", "after", "__syncthreads();", 1),
        ("3", "weight blocks: the batch sums", "before", "// the four batch lanes combined, class by class", 1),
        ("4", "weight blocks: combined and stored", "before", "}", -1)]),
    3: ("heads_bwd_dzf slices", "__global__ __launch_bounds__(256) void heads_bwd_dzf_kernel(const T* __restrict__ dhcl, const T* __restrict__ c0T,", [
        ("0", "start", "before", "if ((int)blockIdx.x >= nsl) {", 1),
        ("1", "slice stored (complete)", "after", "if (m < B) store4(dzf + (size_t)m * HK + n0 + 4 * g, v);", 1)]),
    4: ("heads_bwd_dcomb", "__global__ __launch_bounds__(256) void heads_bwd_dcomb_kernel(const T* __restrict__ dzf, const T* __restrict__ sfT,", [
        ("0", "start", "after", FIRST, 1),
        ("1", "slice stored (complete)", "after", "if (m < B) store4(dcomb + (size_t)m * HK + n0 + 4 * g, v);", 1)]),
    5: ("heads_bwd_pool samples", "__global__ __launch_bounds__(256) void heads_bwd_pool_kernel(const T* __restrict__ z, const T* __restrict__ dcomb,", [
        ("0", "start", "before", "if ((int)blockIdx.x >= B) {", 1),
        ("1", "sample's 2 x S rows stored (complete)", "after",
         "pool_fuse_bwd_sample<T>(blockIdx.x, z, dcomb, dzf, gcls1, gcls2, dibs_pool, gibs_pool, dz, B, S, D, off, n_ibs, ibs_first);", 1)]),
    # the weight-gradient tiles of heads_bwd_dzf (blocks 192 ..) and heads_bwd_pool (blocks 256 ..) at B = 256: told apart by block
    6: ("small_tn_tile (in dzf: blocks 192-239, in pool: 256-303)", "__device__ __forceinline__ void small_tn_tile(const T* __restrict__ dY, const int ldy, const T* __restrict__ X, const int ldx,", [
        ("0", "start", "after", "const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;", 1),
        ("1 + 3 * sp", "slab: both operands transposed into LDS", "after", "__syncthreads();", 1),
        ("2 + 3 * sp", "slab: MFMAs issued", "before", "if (db && k0 == 0 && tid < 64) {", 1),
        ("3 + 3 * sp", "slab: bias column sums (k0 == 0 tiles)", "after", "bsplit[sp] = bh[0] + bh[1];", 1, 1),
        ("7", "tile stored (complete)", "after", "if (db && k0 == 0 && tid < 64) db[n0 + tid] = nsplit == 2 ? bsplit[0] + bsplit[1] : bsplit[0];", 1)]),
}


def stamped_source() -> str:
    lines = (REPO / "eyegaze_multimodal_amd" / "csrc" / "heads.hip").read_text().split("\n")
    inserts = []                                   # (line index, before?, text)
    for kid, (name, opening, stamps) in STAMPS.items():
        starts = [i for i, l in enumerate(lines) if l.strip() == opening]
        if len(starts) != 1:
            raise SystemExit(f"stamp_builds: kernel {name}: its opening line occurs {len(starts)} times in heads.hip")
        end = next(i for i in range(starts[0], len(lines)) if lines[i] == "}")          # the definition's closing brace
        for slot, label, where, text, occ, *skip_closing in stamps:
            hits = [i for i in range(starts[0], end + 1) if lines[i].strip() == text]
            if text == "}" and occ == -1:          # the closing brace of the definition itself
                hits, occ = [end], 1
            if len(hits) < occ:
                raise SystemExit(f"stamp_builds: kernel {name}, stamp '{label}': line not found: {text}")
            at = hits[occ - 1]
            if skip_closing:                       # the statement sits in a block that closes on the next line: stamp behind that
                at += skip_closing[0]
            inserts.append((at, where == "before", f"  EG_STAMP({kid}, {slot});   // {label}"))
    for at, before, text in sorted(inserts, key=lambda t: (-t[0], t[1])):
        lines.insert(at if before else at + 1, text)
    src = "\n".join(lines)
    return src.replace('#include "common.h"\n', '#include "common.h"\n' + PRELUDE, 1)


def build():
    from eyegaze_multimodal_amd import build as B
    B.build(verbose=False)                         # the product's objects: everything but heads.o is linked as it is
    OUT.mkdir(parents=True, exist_ok=True)
    src = OUT / "heads_stamped.hip"
    src.write_text(stamped_source())
    obj = OUT / "heads_stamped.o"
    subprocess.run([B.HIPCC, *B.FLAGS, f"-I{B.CSRC}", "-c", str(src), "-o", str(obj)], check=True)
    objs = [str(B.CSRC / (Path(s).stem + ".o")) for s in B.SOURCES if s != "heads.hip"]
    subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB), str(obj), *objs], check=True)
    print(LIB)


def run(out_path=None, steps=12, warm=4):
    import statistics
    import numpy as np
    import torch
    from eyegaze_multimodal_amd import _lib as L
    L.LIB_PATH = LIB                               # before the first call: the package then runs on the diagnostic library
    from eyegaze_multimodal_amd import DualEEGTransformer, HipAdamW
    dev = torch.device("cuda:0")
    Bsz, T = 256, 1024
    model = DualEEGTransformer(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False,
                               use_cross_attention=True, compute_dtype="bf16").to(dev)
    eng, opt = model.engine(Bsz, T, dev), HipAdamW(model)
    g = torch.Generator().manual_seed(0)
    x1, x2 = torch.randn(Bsz, 8, T, generator=g).to(dev), torch.randn(Bsz, 8, T, generator=g).to(dev)
    labels = torch.randint(0, 3, (Bsz,), generator=g).to(dev)
    lib = L.lib()
    lib.eg_diag_stamps_read.argtypes = [C.c_void_p]
    host = np.zeros(NK * NS * NB, dtype=np.uint64)
    per_step = []
    for i in range(warm + steps):
        assert lib.eg_diag_stamps_clear() == 0
        opt.begin_step(eng, seed=i)
        eng.forward(x1, x2, labels, train=True)
        eng.backward(gloss=torch.ones(1, device=dev))
        opt.step(eng)
        torch.cuda.synchronize()
        assert lib.eg_diag_stamps_read(host.ctypes.data) == 0
        if i >= warm:
            per_step.append(host.reshape(NK, NS, NB).astype(np.int64).copy())
    text = [f"in-kernel stamps, B = {Bsz}, bf16, train step; us after the launch's first workgroup passed slot 0 "
            f"(medians over {steps} steps; 100 MHz clock)",
            f"{'kernel / point':78s} {'blocks':>6s} {'median':>7s} {'last':>7s}"]

    def table(kid, name, stamps, blocks=None, title=None):
        text.append(title or name)
        for slot_expr, label, *_ in stamps:
            for sp in (0, 1) if "sp" in slot_expr else (0,):
                slot = eval(slot_expr, {"sp": sp})
                med, last, cnt = [], [], 0
                for st in per_step:
                    sel = np.arange(NB) if blocks is None else np.arange(*blocks)
                    t0s = st[kid, 0, sel]
                    t = st[kid, slot, sel]
                    ok = (t > 0) & (t0s > 0)
                    if not ok.any():
                        continue
                    rel = (t[ok] - t0s[t0s > 0].min()) / 100.0
                    med.append(float(np.median(rel))); last.append(float(rel.max())); cnt = int(ok.sum())
                if med:
                    lab = label + (f" [slab {sp}]" if "sp" in slot_expr else "")
                    text.append(f"  {lab:76s} {cnt:6d} {statistics.median(med):7.2f} {statistics.median(last):7.2f}")
    for kid, (name, _, stamps) in STAMPS.items():
        if kid == 6:
            table(kid, name, stamps, (192, 240), "small_tn_tile inside heads_bwd_dzf (classifier.0 gradients), relative to ITS first tile")
            table(kid, name, stamps, (256, 304), "small_tn_tile inside heads_bwd_pool (symmetric_fusion.proj gradients), relative to ITS first tile")
        else:
            table(kid, name, stamps)
    out = "\n".join(text)
    print(out)
    if out_path:
        Path(out_path).write_text(out + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        build()
    elif len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        raise SystemExit(__doc__)
