#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy table of one kernel translation unit (cross-compiles, no GPU needed):
    tools/kres.py METRIC PART [extra -D flags ...]      e.g.  tools/kres.py 0 0
    tools/kres.py exact [extra -D flags ...]            the kernels of exact_knn.hip, exact_range.hip and knn_graph.hip (every
                                                        instantiation of the two slab kernels)
    tools/kres.py dbscan [extra -D flags ...]           the kernels of dbscan.hip (both passes of its slab kernel per metric)"""
import os
import re
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
flags = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "--offload-arch=gfx950",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage"]
if sys.argv[1] in ("exact", "dbscan"):
    units = ("exact_knn", "exact_range", "knn_graph") if sys.argv[1] == "exact" else ("dbscan",)
    cmds = [[*flags, *sys.argv[2:], "-c", unit + ".hip", "-o", f"/tmp/kres_{unit}.o"] for unit in units]
else:
    metric, part, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
    cmds = [[*flags, *extra, f"-DHNSW_THIS_METRIC={metric}", f"-DHNSW_PART={part}", "-c", "search_kernels_tu.hip", "-o", f"/tmp/kres_{metric}_{part}.o"]]
runs = [subprocess.run(cmd, cwd=os.path.join(root, "hnswlib-rs_amd", "csrc"), capture_output=True, text=True) for cmd in cmds]
rows, cur = [], {}
for line in "".join(p.stderr for p in runs).splitlines():
    m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
    if not m:
        if "error" in line:
            print(line)
        continue
    k, v = m.groups()
    if k == "Function Name":
        cur = {"name": v}
        rows.append(cur)
    else:
        cur[k.split()[0]] = v
for r in rows:
    name = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"hnswgpu::\(anonymous namespace\)::", "", name).split("(")[0].replace("void ", "")
    print(f"{name:58s} vgpr {r.get('VGPRs', '?'):>4s} sgpr {r.get('TotalSGPRs', '?'):>4s} scratch {r.get('ScratchSize', '?'):>4s} occ {r.get('Occupancy', '?')}")
sys.exit(max(p.returncode for p in runs))
