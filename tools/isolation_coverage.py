#!/usr/bin/env python3
"""The search of DESIGN 4.1: every SSAD_API entry point of include/ssad_kernels.h against the GPU test files that run
launchers inside a sentinel arena (tests/guarded.py) or otherwise isolate them.  An entry point counts as reached when
such a file names it, or calls a Python wrapper (any function of the package other than the ctypes binding `lib`)
whose body names it.  Prints the entry points not reached; profiles/default_engine_tests.md keeps the last result.

usage: python tools/isolation_coverage.py"""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "semi-supervised-adaptive-distillation_amd")


def read(path):
    with open(path) as f:
        return f.read()


def main():
    header = read(os.path.join(ROOT, "include", "ssad_kernels.h"))
    entries = list(dict.fromkeys(re.findall(r"SSAD_API\s+[\w\s\*]+?\b(ssad_\w+)\s*\(", header)))
    files = [f for f in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu*.py")))
             if re.search(r"guarded|test_gpu_isolation|default_engine", os.path.basename(f) + read(f))]
    text = "\n".join(read(f) for f in files)
    wrappers = {}
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        src = read(path)
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, ast.FunctionDef) and node.name != "lib":
                for e in set(re.findall(r"\b(ssad_\w+)\b", ast.get_source_segment(src, node))):
                    wrappers.setdefault(e, set()).add(node.name)
    missing = []
    for e in entries:
        named = re.search(r"\b%s\b" % e, text) is not None
        via = [w for w in wrappers.get(e, ()) if re.search(r"\.%s\(" % re.escape(w), text)]
        if not named and not via:
            missing.append(e)
    print("%d entry points, %d test files, %d not reached" % (len(entries), len(files), len(missing)))
    for e in missing:
        print("  " + e)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
