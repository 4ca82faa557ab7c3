#!/usr/bin/env python3
"""Per-kernel totals of one counter over a rocprofv3 counter-collection CSV, per proof, and the deltas
between two runs (kernels joined by name, template arguments kept):
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -o run -- python3 profiles/prove_loop.py 20 1 lanes1
usage: valu_by_kernel.py PROOFS BEFORE.csv [AFTER.csv]      (PROOFS: proofs the program ran, the divisor)
SQ_INSTS_VALU counts wave64 VALU instructions; totals are printed in millions per proof."""
import collections
import csv
import sys

COUNTER = "SQ_INSTS_VALU"


def totals(path, proofs):
    tot, n = collections.Counter(), collections.Counter()
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] != COUNTER:
            continue
        name = r["Kernel_Name"].split("(")[0].replace("kgs::", "").replace("void ", "")
        tot[name] += float(r["Counter_Value"]) / proofs / 1e6
        n[name] += 1
    return tot, n


def main():
    proofs = float(sys.argv[1])
    a, na = totals(sys.argv[2], proofs)
    b, nb = totals(sys.argv[3], proofs) if len(sys.argv) > 3 else (None, None)
    base = lambda k: k.split("<")[0]
    if b is None:
        for k, v in sorted(a.items(), key=lambda kv: -kv[1]):
            print(f"{v:12.3f} M  x{na[k] / proofs:7.1f}  {k}")
        print(f"{sum(a.values()):12.3f} M  total")
        return
    # the two builds may differ in template arguments: join by the name before '<'
    ga, gb = collections.Counter(), collections.Counter()
    for k, v in a.items():
        ga[base(k)] += v
    for k, v in b.items():
        gb[base(k)] += v
    print(f"{'before M':>12s} {'after M':>12s} {'delta M':>10s}  kernel")
    for k in sorted(set(ga) | set(gb), key=lambda k: -max(ga[k], gb[k])):
        print(f"{ga[k]:12.3f} {gb[k]:12.3f} {gb[k] - ga[k]:10.3f}  {k}")
    print(f"{sum(ga.values()):12.3f} {sum(gb.values()):12.3f} {sum(gb.values()) - sum(ga.values()):10.3f}  total")


if __name__ == "__main__":
    main()
