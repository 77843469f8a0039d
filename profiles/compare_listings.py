#!/usr/bin/env python3
"""Compare the device listings (csrc/Makefile's `%.s` rule) of two builds kernel by kernel: which kernels have the same instruction stream -- comments, directives
and local label names stripped -- and, for those that differ, registers, LDS and instruction counts before and after.

    python profiles/compare_listings.py <dir of the parent's *.s> <dir of the change's *.s>"""
import os
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [instruction lines]} and {mangled name: metadata} of one listing"""
    text = open(path).read()
    body, meta = {}, {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.section\s+\.rodata", text, re.M | re.S):
        lines = []
        for ln in m.group(2).split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") and not ln.endswith(":"):
                continue
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        body[m.group(1)] = lines
    for block in re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return body, meta


def demangle(names):
    try:
        out = subprocess.run(["c++filt", "-p"] + names, capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def main(before_dir, after_dir):
    for f in sorted(os.listdir(after_dir)):
        if not f.endswith(".s") or not os.path.exists(os.path.join(before_dir, f)):
            continue
        b_body, b_meta = kernels(os.path.join(before_dir, f))
        a_body, a_meta = kernels(os.path.join(after_dir, f))
        names = demangle(sorted(set(b_body) | set(a_body)))
        print(f"== {f}")
        for k in sorted(names, key=names.get):
            if k not in b_body or k not in a_body:
                print(f"  {names[k]}: only in the {'parent' if k in b_body else 'change'}")
            elif b_body[k] == a_body[k]:
                print(f"  {names[k]}: identical ({len(a_body[k])} lines, {a_meta[k]['vgpr_count']} VGPRs)")
            else:
                b, a = b_meta[k], a_meta[k]
                print(f"  {names[k]}: DIFFERS  VGPRs {b['vgpr_count']} -> {a['vgpr_count']}, SGPRs {b['sgpr_count']} -> {a['sgpr_count']}, LDS {b['group_segment_fixed_size']} -> "
                      f"{a['group_segment_fixed_size']}, scratch {b['private_segment_fixed_size']} -> {a['private_segment_fixed_size']}, lines {len(b_body[k])} -> {len(a_body[k])}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
