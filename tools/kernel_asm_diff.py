#!/usr/bin/env python3
"""Device assembly of two trees, compared function by function (CPU): did a change move any pre-existing kernel?

  git archive <base-commit> pilot_amd include | tar -x -C /tmp/base
  python tools/kernel_asm_diff.py /tmp/base/pilot_amd/csrc            # every translation unit of both trees

The units of a tree are the *.hip files of its csrc, with sk_inst.hip expanded to the parts (-DSK_PART) and flags of that tree's
Makefile.  Each unit is compiled with the Makefile's flags to gfx950 assembly (--cuda-device-only -S) and split at the function
labels (comments dropped, basic-block label numbers normalised); each kernel's entry in the code object metadata is compared too.
A name can occur in several units (a static kernel of a shared header, a device function that is not inlined), so the two trees
are compared per name on the multiset of bodies over ALL of their units: a kernel that moved from one translation unit to another
counts as identical.  Prints identical / changed / missing / new; exit status 1 if a base function changed or disappeared."""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilot_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wall -Wno-unused-function".split()


def units(csrc):
    """(name, source, extra flags) of every translation unit of the tree at csrc."""
    mk = open(os.path.join(csrc, "Makefile")).read()
    parts = re.search(r"^PARTS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    no_vgpr_form = re.search(r"\$\(if \$\(filter ([\d ]+),\$\*\)", mk).group(1).split()     # parts built without the MFMA VGPR form
    out = []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        src = os.path.basename(path)
        if src != "sk_inst.hip":
            out.append((src, src, []))
            continue
        for p in parts:
            extra = ["-DSK_PART=" + p] + ([] if p in no_vgpr_form else ["-mllvm", "-amdgpu-mfma-vgpr-form=1"])
            out.append(("%s:%s" % (src, p), src, extra))
    return out


def functions(text):
    """(name, body) of every function of an assembly file, comments dropped and basic-block numbers normalised, and of every
    kernel's entry in the code object metadata (registers, LDS, scratch, arguments) as "<kernel> (metadata)"."""
    funcs, cur, meta = [], None, None
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            meta = []
            continue
        if meta is not None:
            if line.startswith("  - "):
                meta.append([line])
            elif line.startswith("    ") and meta:
                meta[-1].append(line)
            elif not line.startswith(" "):
                break
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "__", "amdhsa.")):
            cur = (m.group(1), [])
            funcs.append(cur)
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip())
        if line:
            cur[1].append(line)
    out = [(name, "\n".join(body)) for name, body in funcs]
    for entry in meta or []:
        name = next(l.split(":", 1)[1].strip() for l in entry if l.startswith("    .name:"))
        out.append((name + " (metadata)", "\n".join(entry)))
    return out


def tree_functions(csrc, out_dir, tag, jobs):
    """name -> Counter of bodies over every unit of the tree; name -> units it occurs in."""
    def compile_one(unit):
        name, src, extra = unit
        out = os.path.join(out_dir, "%s_%s.s" % (tag, re.sub(r"[:.]", "_", name)))
        subprocess.run([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", "-o", out, src], cwd=csrc, check=True,
                       stderr=subprocess.DEVNULL)
        return name, functions(open(out).read())
    bodies, where = collections.defaultdict(collections.Counter), collections.defaultdict(list)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for unit, funcs in ex.map(compile_one, units(csrc)):
            for name, body in funcs:
                bodies[name][body] += 1
                where[name].append(unit)
    return bodies, where


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base_csrc", help="pilot_amd/csrc of the base tree")
    ap.add_argument("-j", "--jobs", type=int, default=min(16, os.cpu_count() or 1), help="parallel compilations")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, where_a = tree_functions(os.path.abspath(args.base_csrc), tmp, "base", args.jobs)
        b, where_b = tree_functions(CSRC, tmp, "this", args.jobs)
    changed = sorted(k for k in a if k in b and a[k] != b[k])
    missing = sorted(k for k in a if k not in b)
    new = sorted(k for k in b if k not in a)
    moved = sorted(k for k in a if k in b and a[k] == b[k] and sorted(where_a[k]) != sorted(where_b[k]))
    print("%d device functions and kernel metadata entries in base: %d identical (%d of them in other units now), %d changed, %d missing; %d new"
          % (len(a), len(a) - len(changed) - len(missing), len(moved), len(changed), len(missing), len(new)))
    for title, names, where in (("changed", changed, where_a), ("missing", missing, where_a), ("new", new, where_b)):
        for k in names:
            print("  %-8s %s  (%s)" % (title, k, ", ".join(sorted(set(where[k])))))
    sys.exit(1 if changed or missing else 0)


if __name__ == "__main__":
    main()
