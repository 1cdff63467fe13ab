"""Per-kernel comparison of two `hipcc -S --cuda-device-only` listings (a refactor's bar: no instruction moves):

    python profiles/tools/isa_compare.py PARENT.s CHANGE.s [more pairs ...]

For every kernel symbol the instruction text is compared after dropping comments and directives and normalising the function number
in `.LBB<n>_<m>` labels; the resource summary the compiler prints after each kernel (registers, spills, scratch, LDS, occupancy) is
compared too.  A kernel that differs is shown with its differing lines and its MFMA / ds_ / vector-memory counts on both sides.
Exit status 1 if a kernel present on both sides differs or the change side has a kernel the parent has not."""
import difflib
import re
import sys


def kernels(path):
    """{symbol: (instruction lines, {resource: value})} of the .amdhsa kernels of a listing"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(\S+):", lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        sym, body, res = m.group(1), [], {}
        i += 1
        while not lines[i].startswith(".Lfunc_end"):
            s = lines[i].split(";")[0].strip()
            if s and (not s.startswith(".") or s.startswith(".LBB")):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
            i += 1
        while i < len(lines) and not ((m := re.match(r"^(\S+):", lines[i])) and m.group(1) in names):
            if (m := re.match(r"^; (\w[\w ]*): (\d+)\s*$", lines[i])):
                res[m.group(1)] = int(m.group(2))
            i += 1
        out[sym] = (body, res)
    return out


def mix(body):
    ops = [l.split()[0] for l in body if not l.startswith(".LBB")]
    return {"mfma": sum(o.startswith("v_mfma") for o in ops), "ds": sum(o.startswith("ds_") for o in ops),
            "vmem": sum(o.startswith(("global_", "buffer_", "scratch_", "flat_")) for o in ops)}


def main():
    bad = False
    for pa, ch in zip(sys.argv[1::2], sys.argv[2::2]):
        a, b = kernels(pa), kernels(ch)
        print(f"== {pa}  vs  {ch}: {len(a)} / {len(b)} kernels")
        for sym in sorted(set(a) | set(b)):
            if sym not in b:
                print(f"{sym}  {len(a[sym][0])}  -  only in parent")
            elif sym not in a:
                print(f"{sym}  -  {len(b[sym][0])}  ONLY IN CHANGE")
                bad = True
            else:
                (ia, ra), (ib, rb) = a[sym], b[sym]
                same = ia == ib and ra == rb
                print(f"{sym}  {len(ia)}  {len(ib)}  {'same' if same else 'DIFFERENT'}")
                if not same:
                    bad = True
                    print(f"   parent {mix(ia)} {ra}\n   change {mix(ib)} {rb}")
                    for l in list(difflib.unified_diff(ia, ib, "parent", "change", lineterm="", n=1))[:200]:
                        print("   " + l)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
