#!/usr/bin/env python3
"""profiles/ff_rows.txt from the MOBI_RECORD_ERRORS rows of tests/test_gpu_ff_rows.py:

    MOBI_RECORD_ERRORS=rows.tsv pytest -m gpu tests/test_gpu_ff_rows.py --durations=15        (one MI355X)
    python tools/ff_rows_table.py rows.tsv > profiles/ff_rows.txt

Per <group>.<form>.<dtype>: the cases and launches judged by test_rows_and_channels, the worst whole-tensor rel-L2 against
float64 over TOL, and for the row and the channel measure the worst kernel figure, the worst restated figure and the worst
kernel / restated ratio of one case (asserted <= 2).  The launch totals of the other tests follow."""
import collections
import sys

FIGURES = ("rel.restated", "row.restated", "channel.restated", "launches", "rel", "row", "channel")


def main(path):
    cases = collections.defaultdict(dict)
    totals = []
    for line in open(path):
        parts = line.rstrip("\n").split("\t")
        if len(parts) != 4 or "test_gpu_ff_rows" not in parts[0]:
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
    print("# mobi_ff_geglu per output row and channel on the MI355X, from the MOBI_RECORD_ERRORS rows of tests/test_gpu_ff_rows.py")
    print("# (tools/ff_rows_table.py).  rel / TOL: worst whole-tensor rel-L2 against float64 over TOL; row, channel: the worst")
    print("# measure of the kernel, the worst of the fp32 restatement (tests/ff_ref.py) and the worst kernel / restated ratio of")
    print("# one case, asserted <= 2.")
    print(f"{'group':7s} {'form':14s} {'dtype':5s} {'cases':>5s} {'launches':>8s} {'rel':>10s} {'rel/TOL':>7s} {'row kernel':>10s} "
          f"{'restated':>10s} {'k/r':>5s} {'chan kernel':>11s} {'restated':>10s} {'k/r':>5s}  worst row ratio at")
    ratio = lambda c, k: c[k][0] / c[k + ".restated"][0] if k in c and c[k + ".restated"][0] > 0 else 0.0
    worst = collections.defaultdict(float)
    for key in sorted(groups):
        g = groups[key]
        launches = sum(int(c.get("launches", (0, 0))[0]) for _, c in g)
        rel = max((c["rel"] for _, c in g if "rel" in c), key=lambda v: v[0] / v[1], default=(0.0, 1.0))
        name, _ = max(g, key=lambda nc: ratio(nc[1], "row"))
        top = lambda k: max(c[k][0] for _, c in g)
        row, chan = max(ratio(c, "row") for _, c in g), max(ratio(c, "channel") for _, c in g)
        worst[key[2]] = max(worst[key[2]], row, chan)
        print(f"{key[0]:7s} {key[1]:14s} {key[2]:5s} {len(g):5d} {launches:8d} {rel[0]:10.3e} {rel[0] / rel[1]:7.2f} "
              f"{top('row'):10.3e} {top('row.restated'):10.3e} {row:5.2f} {top('channel'):11.3e} {top('channel.restated'):10.3e} "
              f"{chan:5.2f}  {name}")
    for dtype in ("fp16", "bf16"):
        print(f"# {dtype}: worst kernel / restated measure {worst[dtype]:.3f}")
    for name, n in totals:
        print(f"# launches {name[:-len('.launches')]}: {n}")
    print(f"# launches in all: {sum(n for _, n in totals)}")


if __name__ == "__main__":
    main(sys.argv[1])
