"""The lean instantiations' static picture (profiles/infer_isa.txt):

    python profiles/tools/infer_isa.py PARENT_attnblock.s CHANGE_attnblock.s PARENT_ffn.s CHANGE_ffn.s

Listings by `hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only`.  The change adds a trailing template flag KEEP to
attn_block_fwd_kernel and ffn_chain_kernel, so the symbols differ; kernels are matched by demangled name with the trailing flag removed:
  * `<..., true>` on the change side is the parent's `<...>`: instruction text (isa_compare.py's normalisation) and the compiler's
    resource summary must be equal;
  * `<..., false>` is a lean form: its resources are shown beside its keeping twin's; it must not use scratch or more registers,
    and its global stores are counted (the LayerNorm output alone: 2 x 16 B per row a lane owns).
Exit status 1 if any of that fails."""
import re
import subprocess
import sys

from isa_compare import kernels, mix

CXXFILT = "c++filt"
KEYS = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def demangled(ks):
    names = list(ks)
    out = subprocess.run([CXXFILT, *names], capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^void \(anonymous namespace\)::|\(.*$", "", d): ks[n] for n, d in zip(names, out)}


def stores(body):
    return sum(l.split()[0].startswith(("global_store", "buffer_store", "flat_store", "scratch_store")) for l in body if not l.startswith(".LBB"))


def short(res):
    return " ".join(f"{k} {res.get(k, '-')}" for k in KEYS)


def main():
    bad = False
    for pa, ch in zip(sys.argv[1::2], sys.argv[2::2]):
        a, b = demangled(kernels(pa)), demangled(kernels(ch))
        print(f"== {pa.split('/')[-1]}: {len(a)} kernels on the parent, {len(b)} on the change")
        for name in sorted(b):
            body, res = b[name]
            base = re.sub(r", (true|false)>$", ">", name)
            if name.endswith(", true>") and base in a:
                pb, pr = a[base]
                same = pb == body and pr == res
                bad |= not same
                print(f"{base}\n    parent {len(pb):6d} instructions | {short(pr)}\n    change {len(body):6d} instructions | {short(res)}"
                      f"\n    {'SAME instruction stream and resources' if same else 'DIFFERENT'}")
            elif name.endswith(", false>"):
                tb, tr = b[base[:-1] + ", true>"]
                ok = res["ScratchSize"] == 0 and res["NumVgprs"] <= tr["NumVgprs"] and res["Occupancy"] >= tr["Occupancy"]
                bad |= not ok
                print(f"{name}   (LEAN)\n    keeping {len(tb):6d} instructions | {short(tr)} | {mix(tb)} global stores {stores(tb)}"
                      f"\n    lean    {len(body):6d} instructions | {short(res)} | {mix(body)} global stores {stores(body)}"
                      f"\n    {'no scratch, registers <= the keeping twin' if ok else 'FAILS the resource rule'}")
            else:
                print(f"{name}  UNMATCHED")
                bad = True
        for name in sorted(set(a) - {re.sub(r", (true|false)>$", ">", n) for n in b}):
            print(f"{name}  ONLY IN PARENT")
            bad = True
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
