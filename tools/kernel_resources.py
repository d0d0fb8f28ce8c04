#!/usr/bin/env python3
"""Per-kernel register / LDS / scratch / occupancy table of one .hip file (hipcc -Rpass-analysis=kernel-resource-usage).

    python tools/kernel_resources.py ei-nexus_official_amd/csrc/conv.hip [filter-substring] [-D...] [--json]

--json: the rows as one JSON list instead of the table (tests/test_event_reps_cpu.py reads it).
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    src = sys.argv[1]
    flt = [a for a in sys.argv[2:] if not a.startswith("-")]
    extra = [a for a in sys.argv[2:] if a.startswith("-") and a != "--json"]
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/dev/null"] + extra
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            cur = {"name": dem.replace("(anonymous namespace)::", "")}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    rows = [r for r in rows if not flt or all(f in r["name"] for f in flt)]
    if "--json" in sys.argv[2:]:
        print(json.dumps(rows))
        return
    print("%-90s %5s %5s %5s %6s %4s %6s %7s" % ("kernel", "VGPR", "AGPR", "SGPR", "LDS", "occ", "spill", "scratch"))
    for r in rows:
        print("%-90s %5s %5s %5s %6s %4s %6s %7s" % (r["name"][:90], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"),
                                                     r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]"), r.get("VGPRs Spill"),
                                                     r.get("ScratchSize [bytes/lane]")))


if __name__ == "__main__":
    main()
