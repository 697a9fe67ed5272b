#!/usr/bin/env python3
"""The compiler's resource lines of every kernel, from the .remarks files a build leaves beside its objects
(csrc/Makefile: -Rpass-analysis=kernel-resource-usage), by demangled name -- the table profiles/*/resource_usage.txt hold, so
that two commits' tables can be compared with diff.

    python3 tools/resource_lines.py [REMARKS_DIR] > profiles/NAME/resource_usage.txt
"""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
        ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def table(directory):
    out = ["# hipcc -Rpass-analysis=kernel-resource-usage with the flags of csrc/Makefile (the .remarks files of the build), per source file",
           "# kernel | VGPRs | SGPRs | scratch bytes per lane | occupancy (waves per SIMD) | LDS bytes per workgroup"]
    for f in sorted(glob.glob(os.path.join(directory, "*.remarks"))):
        rows, cur = [], None
        for line in open(f, errors="replace"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = {"name": m.group(1)}
                rows.append(cur)
                continue
            for key, pat in KEYS:
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = m.group(1)
        if not rows:
            continue
        names = subprocess.run(["c++filt"] + [r["name"] for r in rows], capture_output=True, text=True).stdout.split("\n")
        out.append("## " + os.path.basename(f).replace(".remarks", ".hip"))
        for r, n in zip(rows, names):
            out.append(" | ".join([re.sub(r"\(.*", "", n).replace("void ", "")] + [r.get(k, "?") for k, _ in KEYS]))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    sys.stdout.write(table(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "practical_path_guiding_lab_amd", "csrc")))
