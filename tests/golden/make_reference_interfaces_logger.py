#!/usr/bin/env python3
"""tests/golden/reference_interfaces_logger.json: the reference's signatures that tests/test_image_logger_cpu.py compares
`LatentDiffusion.log_images` / `sample_log` and `train.ImageLogger` with, so that the test needs no reference tree.  Nothing of
the reference is copied: argument names, literal defaults and the name of the `**` argument, read with ast (not imported).
    python tests/golden/make_reference_interfaces_logger.py REFERENCE_TREE      (or MOBI_REFERENCE names it)"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SIGNATURES = [("ldm/models/diffusion/ddpm.py", "LatentDiffusion", "log_images"),
              ("ldm/models/diffusion/ddpm.py", "LatentDiffusion", "sample_log"),
              ("main.py", "ImageLogger", "__init__"),
              ("main.py", "ImageLogger", "check_frequency")]


def ref_args(path, cls, fn):
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name == fn:
                    return {"names": [a.arg for a in f.args.args if a.arg != "self"],
                            "defaults": [ast.literal_eval(d) for d in f.args.defaults],
                            "kwarg": f.args.kwarg.arg if f.args.kwarg else None}
    raise KeyError((cls, fn))


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("MOBI_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    out = {"signatures": {f"{cls}.{fn}": ref_args(os.path.join(ref, path), cls, fn) for path, cls, fn in SIGNATURES}}
    with open(os.path.join(HERE, "reference_interfaces_logger.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote reference_interfaces_logger.json:", sorted(out["signatures"]))


if __name__ == "__main__":
    main(sys.argv)
