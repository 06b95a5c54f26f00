#!/usr/bin/env python3
"""tests/golden/reference_interfaces.json: what tests/test_dropin_cpu.py and tests/test_abi_cpu.py compare the engine's
drop-in surface with, so that neither needs the reference tree at test time.  Nothing of the reference is copied:
  signatures -- argument names and literal defaults of the entry points the harness calls (read with ast, not imported);
  configs    -- sha256 of every reference config file's parsed values, before and after `${}` resolution by the engine's
                loader (canonical JSON, sorted keys).
    python tests/golden/make_reference_interfaces.py          (MOBI_REFERENCE names the reference tree)"""
import ast
import hashlib
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MOBI_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

SIGNATURES = [("ldm/models/diffusion/ddim.py", "DDIMSampler", "sample"),
              ("ldm/models/diffusion/ddpm.py", "LatentDiffusion", "log_data"),
              ("ldm/models/diffusion/ddpm.py", "LatentDiffusion", "decode_sample")]
CONFIGS = ["mobi_nusc-mini_256", "mobi_nusc-mini_512", "mobi_nusc_256", "mobi_nusc_512", "mobi_nusc_all-classes_256",
           "mobi_nusc_all-classes_512", "range_autoencoder", "pbe"]


def digest(obj):
    """sha256 of a parsed config: the same for two configs exactly when they compare equal as dicts."""
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def ref_args(path, cls, fn):
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for f in node.body:
                if isinstance(f, ast.FunctionDef) and f.name == fn:
                    return {"names": [a.arg for a in f.args.args if a.arg != "self"],
                            "defaults": [ast.literal_eval(d) for d in f.args.defaults]}
    raise KeyError((cls, fn))


def main():
    from mobi_amd.ldm.util import load_config
    out = {"signatures": {f"{cls}.{fn}": ref_args(os.path.join(REF, path), cls, fn) for path, cls, fn in SIGNATURES},
           "configs": {}}
    for name in CONFIGS:
        path = os.path.join(REF, "configs", name + ".yaml")
        with open(path) as f:
            raw = yaml.safe_load(f)
        out["configs"][name] = {"raw_sha256": digest(raw), "resolved_sha256": digest(load_config(path))}
    with open(os.path.join(HERE, "reference_interfaces.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote reference_interfaces.json:", sorted(out["signatures"]), len(out["configs"]), "configs")


if __name__ == "__main__":
    main()
