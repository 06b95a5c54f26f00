#!/usr/bin/env python3
"""tests/golden/train_cli.json: the command line of the reference's main.py (`get_parser`) as data -- every `add_argument` call's
flags, default, type, const and nargs, read with ast (the script is never imported, nothing of its text is copied) -- so that
tests/test_main_cpu.py can hold `mobi_amd.main`'s parser against it without the reference tree.
    MOBI_REFERENCE=<reference tree> python tests/golden/make_train_cli.py"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def cli_arguments(path):
    tree = ast.parse(open(path).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "get_parser")
    out = []
    for node in ast.walk(fn):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {}
            for k in node.keywords:
                if k.arg in ("help", "metavar"):
                    continue
                kw[k.arg] = k.value.id if k.arg == "type" else ast.literal_eval(k.value)
            out.append({"flags": [ast.literal_eval(a) for a in node.args], **kw})
    return sorted(out, key=lambda a: a["flags"])


def main():
    ref = os.environ.get("MOBI_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        raise SystemExit("name the reference tree: MOBI_REFERENCE=<path>")
    args = cli_arguments(os.path.join(ref, "main.py"))
    with open(os.path.join(HERE, "train_cli.json"), "w") as f:
        json.dump({"arguments": args}, f, indent=1)
        f.write("\n")
    print("wrote train_cli.json:", len(args), "arguments")


if __name__ == "__main__":
    main()
