#!/usr/bin/env python
"""Two builds of one csrc/*.hip, kernel for kernel: the register / LDS / scratch metadata and the instruction stream.

    python tools/compare_kernels.py PARENT/decnet_amd/csrc/x.hip decnet_amd/csrc/x.hip [OUT.json [RENAMES.json]]

Compiles both with the flags of decnet_amd/build.py plus `--cuda-device-only -S` (no GPU needed), drops comments, `.loc`,
`.file`, `.ident` and the other directives, and matches the kernels by demangled name and template arguments (without the
parameter list and the unnamed namespace, so a parameter type that moved to a header does not unmatch a kernel).  Prints
one line per kernel that differs and a count; OUT.json gets every kernel: metadata of both, waves per SIMD of both (512
unified registers per lane and SIMD on gfx950, allocated in eights, at most 8 waves), instruction counts, `same_code`.
Either side may be several files joined by commas (kernels that moved between files): their kernels are taken together.
RENAMES.json, {tree kernel: parent kernel}, pairs kernels whose names changed (several tree kernels may name one parent
kernel); such a pair is compared like any other and reported as "parent kernel -> tree kernel".
Exit status 1 when a kernel is unmatched."""
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decnet_amd import build as B  # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


def assembly(src):
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=" + B.ARCH, "-O3",
                               "-std=c++17", "-fPIC", "-w"] + B.EXTRA_FLAGS.get(os.path.basename(src), []) +
                              ["--cuda-device-only", "-S", src, "-o", f.name])
        return open(f.name).read()


def kernels(asm):
    """-> {name<template arguments>: {"meta": {...}, "code": [instruction, ...]}}"""
    meta = {}
    for blk in asm.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        sym = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
        meta[sym] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in META}
    names = subprocess.run(["c++filt"], input="\n".join(meta), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, dem in zip(meta, names):
        body = asm[asm.index("\n%s:" % sym):]                      # the symbol's label ... its .Lfunc_end: every exit block
        body = body[:body.index("\n.Lfunc_end")].split("\n")[2:]
        code = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in body]
        code = [ln for ln in code if ln and not (ln.startswith(".") and not ln.startswith(".LBB_"))]
        key = re.sub(r"^void ", "", dem.replace("(anonymous namespace)::", "")).split("(")[0]
        assert key not in out, key
        out[key] = {"meta": meta[sym], "code": code}
    return out


def waves(m):
    return min(8, 512 // (-(-max(m["vgpr_count"], 1) // 8) * 8))


def all_kernels(srcs):
    out = {}
    for src in srcs.split(","):
        ks = kernels(assembly(src))
        assert not set(ks) & set(out), sorted(set(ks) & set(out))
        out.update(ks)
    return out


def main(parent, tree, out=None, renames=None):
    a, b = all_kernels(parent), all_kernels(tree)
    if renames:
        with open(renames) as f:
            renames = json.load(f)
        assert not set(renames) & set(a) and not set(renames.values()) & set(b), "a renamed kernel kept its name"
        a.update({"%s -> %s" % (old, new): a[old] for new, old in renames.items()})
        b.update({"%s -> %s" % (old, new): b.pop(new) for new, old in renames.items()})
        for old in set(renames.values()):
            del a[old]
    doc, differ = {}, 0
    for k in sorted(set(a) & set(b)):
        same = a[k]["code"] == b[k]["code"]
        doc[k] = {"parent": a[k]["meta"], "tree": b[k]["meta"], "waves_per_simd": [waves(a[k]["meta"]), waves(b[k]["meta"])],
                  "instructions": [len(a[k]["code"]), len(b[k]["code"])], "same_code": same}
        if not same or a[k]["meta"] != b[k]["meta"]:
            differ += 1
            print(k, {m: (a[k]["meta"][m], b[k]["meta"][m]) for m in META if a[k]["meta"][m] != b[k]["meta"][m]},
                  "instructions", doc[k]["instructions"], "waves", doc[k]["waves_per_simd"])
    unmatched = sorted(set(a) ^ set(b))
    print("%d kernels, %d differ, unmatched: %s" % (len(doc), differ, unmatched))
    if out:
        with open(out, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
            f.write("\n")
    return 1 if unmatched else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
