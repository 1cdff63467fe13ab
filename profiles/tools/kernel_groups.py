"""Two kernel traces of the bench command side by side, per (kernel, grid) group: launches per step, per-launch mean and the
p10 / p50 / p90 of the last `steps` steps, and for every group present on both sides whether the change's mean lies inside the
parent's own p10-p90 band.  Usage: kernel_groups.py <parent trace dir> <change trace dir> [steps=100]"""
import collections
import csv
import glob
import sys


def groups(d, steps):
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "set_step_state_kernel" in r["Kernel_Name"]]     # the first launch of a step
    rows = rows[marks[-steps - 1]:marks[-1]] if len(marks) > steps else rows
    agg = collections.defaultdict(list)
    for r in rows:
        n = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        agg[(n, int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: sorted(v) for k, v in agg.items()}


def stats(v, steps):
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return len(v) / steps, sum(v) / len(v), q(0.1), q(0.5), q(0.9)


steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
P, Cg = groups(sys.argv[1], steps), groups(sys.argv[2], steps)
print(f"per-launch us over the last {steps} steps; band = the change's mean inside the parent's p10-p90")
print(f"{'kernel':58s} {'grid':>6s} {'n/step':>6s} | {'parent mean':>11s} {'p10':>7s} {'p50':>7s} {'p90':>7s} | {'change mean':>11s} {'p50':>7s} | band")
tot = {"parent": 0.0, "change": 0.0}
for k in sorted(set(P) | set(Cg), key=lambda k: -(sum(P.get(k, [0])) + sum(Cg.get(k, [0])))):
    p = stats(P[k], steps) if k in P else None
    c = stats(Cg[k], steps) if k in Cg else None
    tot["parent"] += sum(P.get(k, [])) / steps
    tot["change"] += sum(Cg.get(k, [])) / steps
    ps = f"{p[1]:11.1f} {p[2]:7.1f} {p[3]:7.1f} {p[4]:7.1f}" if p else f"{'--':>11s} {'':7s} {'':7s} {'':7s}"
    cs = f"{c[1]:11.1f} {c[3]:7.1f}" if c else f"{'--':>11s} {'':7s}"
    band = "" if not (p and c) else ("in" if p[2] <= c[1] <= p[4] else ("BELOW" if c[1] < p[2] else "ABOVE"))
    print(f"{k[0][:58]:58s} {k[1]:6d} {(p or c)[0]:6.1f} | {ps} | {cs} | {band}")
print(f"sum of kernel durations per step: parent {tot['parent']:.1f} us, change {tot['change']:.1f} us")
