#!/usr/bin/env python3
"""profiles/norm_groups.txt from the MOBI_RECORD_ERRORS rows of tests/test_gpu_norm_groups.py:

    MOBI_RECORD_ERRORS=rows.tsv pytest -m gpu tests/test_gpu_norm_groups.py        (one MI355X)
    python tools/norm_groups_table.py rows.tsv > profiles/norm_groups.txt

Per (form, kernel body, storage type): the cases judged (each with and without SiLU; LayerNorm: once), and for every figure
the worst value of the kernel next to the worst of the fp32 restatement (tests/norm_ref.py) over those cases, then the worst
kernel / restatement ratio of a single case (asserted <= 2, or the case's margin in tests/norm_cases.py).  rel: whole-tensor
rel-L2 against float64; group, channel: worst rel-L2 of an (image, group) / (image, channel) -- LayerNorm: of a row / of a
channel over all rows; rstd, mean: the statistics recovered from the rounded output of the launches without SiLU."""
import collections
import sys

FIGURES = ("rel", "group", "channel", "rstd", "mean")
WITH_BODY = ("regs", "slabs", "ln")


def main(path):
    cases = collections.defaultdict(dict)
    for line in open(path):
        parts = line.rstrip("\n").split("\t")
        if len(parts) != 4 or "test_gpu_norm_groups" not in parts[0]:
            continue
        name, value = parts[1].split("."), float(parts[2])
        nkey = 3 if name[0] in WITH_BODY else 2
        key = (name[0], name[1] if nkey == 3 else "-", name[nkey - 1])
        rest = name[nkey:]
        if rest[-1] == "launches":
            continue
        if name[0] == "precise":                                     # fp32 outputs (out_mode 2) apart: another scale of figures
            key = (name[0], "f32 out" if "mode2" in rest else "T out", key[2])
        fig = rest[-1] if rest[-1] != "restated" else rest[-2] + ".restated"
        case = ".".join(rest[:-2] if rest[-1] == "restated" else rest[:-1])
        cases[key + (case,)][fig] = value
    groups = collections.defaultdict(list)
    for k, c in cases.items():
        groups[k[:3]].append((k[3], c))
    print("# GroupNorm / LayerNorm per group, channel and row on the MI355X, from the MOBI_RECORD_ERRORS rows of")
    print("# tests/test_gpu_norm_groups.py (tools/norm_groups_table.py).  Each figure: worst of the kernel / worst of the fp32")
    print("# restatement over the form's cases; k/r: the worst kernel / restatement ratio of one case over group, channel, rstd and")
    print("# mean (asserted <= 2).  rel against TOL 5e-4 (fp16) / 4e-3 (bf16), 2e-6 for fp32 outputs.")
    print(f"{'form':8s} {'body':10s} {'dtype':5s} {'cases':>5s}  " + "  ".join(f"{f + ' k / r':>21s}" for f in FIGURES) + "    k/r  worst ratio at")
    worst_all = collections.defaultdict(float)
    for key in sorted(groups):
        g = groups[key]
        cols = []
        for f in FIGURES:
            k = max((c[f] for _, c in g if f in c), default=float("nan"))
            r = max((c[f + ".restated"] for _, c in g if f + ".restated" in c), default=float("nan"))
            cols.append(f"{k:10.3e} {r:10.3e}")
        ratio, at = 0.0, "-"
        for name, c in g:
            for f in FIGURES[1:]:
                if f in c and c[f + ".restated"] > 0 and c[f] / c[f + ".restated"] > ratio:
                    ratio, at = c[f] / c[f + ".restated"], f"{name} ({f})"
        worst_all[key[2]] = max(worst_all[key[2]], ratio)
        print(f"{key[0]:8s} {key[1]:10s} {key[2]:5s} {len(g):5d}  " + "  ".join(cols) + f"  {ratio:5.2f}  {at}")
    for dtype, v in sorted(worst_all.items()):
        print(f"# {dtype}: worst kernel / restatement ratio {v:.3f}")
    print("# margins: the restatement and its twin with permuted sums meet every criterion against each other at 2 on every case")
    print("# (tests/test_norm_ref_cpu.py): no case has a raised margin.  Unreachable bodies: regs 256x16x8 and 1024x1x8, slabs 1024x1x8.")
    print("# precise, f32 out, with the group's first element as the shift of the statistics (gn_shift; the precise forms now use")
    print("# gn_shift_x and fold in fp64): f32src.mode2.plain rel 3.134e-07, group 1.549e-06, channel 1.585e-06, rstd 1.544e-06,")
    print("# mean 4.483e-07 against the restatement's 7.727e-08, 1.653e-07, 1.808e-07, 1.517e-07, 5.534e-08: k/r 10.18, over the margin.")


if __name__ == "__main__":
    main(sys.argv[1])
