#!/usr/bin/env python3
"""tests/golden/test_bench_cli.json: the command line of the reference's scripts/inference_test_bench.py as data -- every
`add_argument` call's flags, default, action, type, choices and nargs, read with ast (the script is never imported, nothing of its
text is copied) -- so that tests/test_test_bench_cpu.py can hold `mobi_amd.test_bench`'s parser against it without the reference tree.
    MOBI_REFERENCE=<reference tree> python tests/golden/make_reference_interfaces_test_bench.py"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def cli_arguments(path):
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {}
            for k in node.keywords:
                if k.arg == "help":
                    continue
                if k.arg == "type":
                    kw["type"] = k.value.id
                elif k.arg == "nargs" and not isinstance(k.value, ast.Constant):
                    kw["nargs"] = k.value.attr                             # argparse.REMAINDER
                else:
                    kw[k.arg] = ast.literal_eval(k.value)
            out.append({"flags": [ast.literal_eval(a) for a in node.args], **kw})
    return out


def main():
    ref = os.environ.get("MOBI_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        raise SystemExit("name the reference tree: MOBI_REFERENCE=<path>")
    args = cli_arguments(os.path.join(ref, "scripts", "inference_test_bench.py"))
    with open(os.path.join(HERE, "test_bench_cli.json"), "w") as f:
        json.dump({"arguments": args}, f, indent=1)
        f.write("\n")
    print("wrote test_bench_cli.json:", len(args), "arguments")


if __name__ == "__main__":
    main()
