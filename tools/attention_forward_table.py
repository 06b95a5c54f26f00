#!/usr/bin/env python3
"""profiles/attention_forward_rows.txt from the MOBI_RECORD_ERRORS rows of tests/test_gpu_attention_forward.py:

    MOBI_RECORD_ERRORS=rows.tsv pytest -m gpu tests/test_gpu_attention_forward.py        (one MI355X)
    python tools/attention_forward_table.py rows.tsv > profiles/attention_forward_rows.txt

Per (kernel body, V layout, storage type): the launches judged, the worst whole-tensor rel-L2 of the kernel (and of the
storage restatement) against float64 with its bound, and the worst head-row measure of the kernel over the restatement's
on the same case (the criterion asks for at most 2)."""
import collections
import sys


def main(path):
    cases = collections.defaultdict(dict)
    for line in open(path):
        parts = line.rstrip("\n").split("\t")
        if len(parts) != 4 or "test_gpu_attention_forward" not in parts[0]:
            continue
        name, value, bound = parts[1], float(parts[2]), float(parts[3])
        for suffix in (".rel.restated", ".row.restated", ".row.kernel", ".rel"):
            if name.endswith(suffix):
                cases[name[:-len(suffix)]][suffix] = (value, bound)
                break
    groups = collections.defaultdict(list)
    for name, c in cases.items():
        if len(c) == 4:
            groups[tuple(name.split(".")[:3])].append((name, c))
    print("# mobi_attention per (image, query, head) row on the MI355X, from the MOBI_RECORD_ERRORS rows of")
    print("# tests/test_gpu_attention_forward.py (tools/attention_forward_table.py).  body: rows<KS,QSH|C> = attention_rows_kernel (shift in")
    print("# Q' | in the C operand), exact<KS> = attention_kernel; rel-L2 against float64, bound TOL (x 1.5 where the kernel rounds Q');")
    print("# row ratio = head-row measure of the kernel / of the storage restatement (tests/attention_ref.py), asserted <= 2.")
    print(f"{'body':18s} {'layout':11s} {'dtype':5s} {'launches':>8s} {'worst rel-L2':>12s} {'restated':>10s} {'bound':>8s} "
          f"{'worst row':>10s} {'restated':>10s} {'worst ratio':>11s}  at")

    def order(key):
        body, layout, dtype = key
        return (body.startswith("exact"), int(body.split("<")[1].split(",")[0].rstrip(">")), body, layout, dtype != "fp16")

    for key in sorted(groups, key=order):
        g = groups[key]
        rel = max(g, key=lambda nc: nc[1][".rel"][0] / nc[1][".rel"][1])[1]
        ratio = lambda c: c[".row.kernel"][0] / c[".row.restated"][0] if c[".row.restated"][0] > 0 else 0.0
        name, row = max(g, key=lambda nc: ratio(nc[1]))
        print(f"{key[0]:18s} {key[1]:11s} {key[2]:5s} {len(g):8d} {rel['.rel'][0]:12.3e} {rel['.rel.restated'][0]:10.3e} "
              f"{rel['.rel'][1]:8.1e} {row['.row.kernel'][0]:10.3e} {row['.row.restated'][0]:10.3e} {ratio(row):11.2f}  "
              f"{'.'.join(name.split('.')[3:])}")


if __name__ == "__main__":
    main(sys.argv[1])
