#!/usr/bin/env python3
"""profiles/igemm_rows.txt from the MOBI_RECORD_ERRORS rows of tests/test_gpu_igemm_rows.py:

    MOBI_RECORD_ERRORS=rows.tsv pytest -m gpu tests/test_gpu_igemm_rows.py --durations=15        (one MI355X)
    python tools/igemm_rows_table.py rows.tsv > profiles/igemm_rows.txt

Per (kernel body, epilogue form, storage type): the cases and launches judged by test_rows_and_channels, the worst
whole-tensor rel-L2 against float64 over its bound, the worst row and channel measure of the kernel over the fp32
restatement's on the same case (asserted <= 2), and the worst |got - ref| over the a-priori fp32 bound (k + 8) 2^-24 A of
the fp32 outputs and deferred slabs (asserted <= 1).  The launch totals of the other tests follow."""
import collections
import sys

FIGURES = ("rel.restated", "row.restated", "channel.restated", "f32.restated", "slab.f32", "launches", "rel", "row", "channel", "f32")


def main(path):
    cases = collections.defaultdict(dict)
    totals = []
    for line in open(path):
        parts = line.rstrip("\n").split("\t")
        if len(parts) != 4 or "test_gpu_igemm_rows" not in parts[0]:
            continue
        name, value, bound = parts[1], float(parts[2]), float(parts[3])
        if name.endswith(".launches") and name.count(".") == 2:
            totals.append((name, int(value)))
            continue
        for fig in FIGURES:
            if name.endswith("." + fig):
                cases[name[:-len(fig) - 1]][fig] = (value, bound)
                break
    groups = collections.defaultdict(list)
    for name, c in cases.items():
        groups[tuple(name.split(".")[:3])].append((".".join(name.split(".")[3:]), c))
    print("# mobi_igemm per output row and channel on the MI355X, from the MOBI_RECORD_ERRORS rows of tests/test_gpu_igemm_rows.py")
    print("# (tools/igemm_rows_table.py).  rel / bound: worst whole-tensor rel-L2 against float64 over TOL (1.5 TOL under a LayerNorm")
    print("# fold); row, channel: worst measure of the kernel over the fp32 restatement's (tests/igemm_ref.py), asserted <= 2;")
    print("# f32: worst |got - ref| / ((k + 8) 2^-24 A) over fp32 outputs and deferred slabs, asserted <= 1.")
    print(f"{'body':10s} {'epilogue form':18s} {'dtype':5s} {'cases':>5s} {'launches':>8s} {'rel':>10s} {'rel/bound':>9s} "
          f"{'row k/r':>8s} {'chan k/r':>8s} {'f32/bound':>9s}  worst row ratio at")
    ratio = lambda c, k: c[k][0] / c[k + ".restated"][0] if k in c and c[k + ".restated"][0] > 0 else 0.0
    worst = collections.defaultdict(float)
    for key in sorted(groups):
        g = groups[key]
        launches = sum(int(c.get("launches", (0, 0))[0]) for _, c in g)
        rel = max((c["rel"] for _, c in g if "rel" in c), key=lambda v: v[0] / v[1], default=(0.0, 1.0))
        name, _ = max(g, key=lambda nc: ratio(nc[1], "row"))
        row, chan = max(ratio(c, "row") for _, c in g), max(ratio(c, "channel") for _, c in g)
        f32 = max([c[k][0] for _, c in g for k in ("f32", "slab.f32") if k in c], default=float("nan"))
        worst[("ratio", key[2])] = max(worst[("ratio", key[2])], row, chan)
        if f32 == f32:
            worst[("f32", key[2])] = max(worst[("f32", key[2])], f32)
        print(f"{key[0]:10s} {key[1]:18s} {key[2]:5s} {len(g):5d} {launches:8d} {rel[0]:10.3e} {rel[0] / rel[1]:9.2f} {row:8.2f} "
              f"{chan:8.2f} {f32:9.3f}  {name}")
    for dtype in ("fp16", "bf16"):
        print(f"# {dtype}: worst kernel / restated measure {worst[('ratio', dtype)]:.3f}, worst fp32 / bound {worst[('f32', dtype)]:.4f}")
    for name, n in totals:
        print(f"# launches {name[:-len('.launches')]}: {n}")
    print(f"# launches in all: {sum(n for _, n in totals)}")


if __name__ == "__main__":
    main(sys.argv[1])
