#!/usr/bin/env python3
"""Device assembly of two trees, compared function by function (CPU): did a change move any pre-existing kernel?

  git archive <base-commit> pilot_amd include | tar -x -C /tmp/base
  python tools/kernel_asm_diff.py /tmp/base/pilot_amd/csrc            # every translation unit of the Makefile

Each translation unit is compiled with the Makefile's flags to gfx950 assembly (--cuda-device-only -S) in both trees, split at the
function labels, and each function of the base compared with the same-named one of this tree (basic-block label numbers
normalised).  Prints identical / changed / missing / new per unit; exit status 1 if a base function changed or disappeared."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilot_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC -fvisibility=hidden --offload-arch=gfx950 -Wall -Wno-unused-function".split()
UNITS = ["pilot_ot.hip", "pilot_ot_multi.hip", "pilot_ot_consumers.hip", "pilot_ot_labels.hip", "sk_wide.hip"] + \
        ["sk_inst.hip:%d" % p for p in range(10)]


def assembly(csrc, unit, out_dir, tag):
    src, _, part = unit.partition(":")
    extra = ["-DSK_PART=" + part] if part else []
    if part in ("0", "1", "2", "3", "4", "5"):
        extra += ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    out = os.path.join(out_dir, "%s_%s.s" % (tag, unit.replace(":", "_").replace(".", "_")))
    subprocess.run([HIPCC, *FLAGS, *extra, "--cuda-device-only", "-S", "-o", out, src], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def functions(text):
    funcs, cur = collections.OrderedDict(), None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_.$][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "__")):
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        funcs[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base_csrc", help="pilot_amd/csrc of the base tree")
    ap.add_argument("units", nargs="*", default=UNITS, help="translation units (sk_inst.hip:N for part N)")
    args = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in args.units:
            a = functions(assembly(args.base_csrc, unit, tmp, "base"))
            b = functions(assembly(CSRC, unit, tmp, "this"))
            changed = [k for k in a if k in b and a[k] != b[k]]
            missing = [k for k in a if k not in b]
            new = [k for k in b if k not in a]
            print("%-22s %3d functions in base: %3d identical, changed %s, missing %s, new %s"
                  % (unit, len(a), len(a) - len(changed) - len(missing), changed, missing, new), flush=True)
            bad += len(changed) + len(missing)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
