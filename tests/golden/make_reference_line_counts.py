#!/usr/bin/env python3
"""Generates tests/golden/reference_line_counts_v1.json: the line count of every file of the reference checkout (path
relative to the checkout -> lines), .git excluded. Data only, no source text: tests/test_citations.py resolves the
`path:line` citations of this repository against it where the checkout itself is absent.
Run from the repo root:  python tests/golden/make_reference_line_counts.py <reference checkout>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def line_counts(ref):
    out = {}
    for dirpath, dirs, names in os.walk(ref):
        dirs[:] = sorted(d for d in dirs if d != ".git")
        for n in sorted(names):
            path = os.path.join(dirpath, n)
            with open(path, errors="replace") as f:
                out[os.path.relpath(path, ref)] = sum(1 for _ in f)
    return out


def main():
    counts = line_counts(sys.argv[1])
    with open(os.path.join(ROOT, "tests", "golden", "reference_line_counts_v1.json"), "w") as f:
        json.dump(counts, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(counts), "files")


if __name__ == "__main__":
    main()
