#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy table of one kernel translation unit (cross-compiles, no GPU needed):
    tools/kres.py METRIC PART [extra -D flags ...]      e.g.  tools/kres.py 0 0
    tools/kres.py exact [extra -D flags ...]            the kernels of exact_knn.hip, exact_range.hip and knn_graph.hip (every
                                                        instantiation of the two slab kernels)
    tools/kres.py dbscan [extra -D flags ...]           the kernels of dbscan.hip (both passes of its slab kernel per metric)
    tools/kres.py screen [extra -D flags ...]           the kernels of exact_screen.hip (screen and rerank per metric, each with its
                                                        SELF variant -- the last template argument -- for the screened exact graph;
                                                        built, like the library's unit, without packed f32 instructions)
    tools/kres.py range_screen [extra -D flags ...]     the kernels of exact_range_screen.hip (screen per metric and register tile,
                                                        rerank per metric; the same flags as screen)
    tools/kres.py dbscan_screen [extra -D flags ...]    the kernels of dbscan_screen.hip (screen per metric, pass and register tile,
                                                        rerank per metric and pass; the same flags as screen)
    tools/kres.py screen_long [extra -D flags ...]      the kernels of exact_screen_long.hip (the streamed screen per metric and its
                                                        SELF variant, the rerank it shares with screen; the same flags as screen; -DHNSW_LONG_NT=2,
                                                        -DHNSW_LONG_WAVES_PER_SIMD=1 for the variants)
    tools/kres.py range_screen_long [extra -D flags ...]  the kernels of exact_range_screen_long.hip (the streamed range screen per metric
                                                        and register tile, the rerank and the scatter it shares with range_screen; the
                                                        same flags as screen; -DHNSW_RANGE_LONG_NT=2 changes the default only)
    tools/kres.py dbscan_screen_long [extra -D flags ...]  the kernels of dbscan_screen_long.hip (the streamed DBSCAN screen per metric, pass
                                                        and register tile, the prep, cut and rerank it shares with dbscan_screen; the
                                                        same flags as screen; -DHNSW_DBSCAN_LONG_NT=2 changes the default only)"""
import os
import re
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
flags = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "--offload-arch=gfx950",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage"]
if sys.argv[1] in ("exact", "dbscan", "screen", "range_screen", "dbscan_screen", "screen_long", "range_screen_long", "dbscan_screen_long"):
    units = {"exact": ("exact_knn", "exact_range", "knn_graph"), "dbscan": ("dbscan",), "screen": ("exact_screen",), "range_screen": ("exact_range_screen",), "dbscan_screen": ("dbscan_screen",), "screen_long": ("exact_screen_long",), "range_screen_long": ("exact_range_screen_long",), "dbscan_screen_long": ("dbscan_screen_long",)}[sys.argv[1]]
    if sys.argv[1] in ("screen", "range_screen", "dbscan_screen", "screen_long", "range_screen_long", "dbscan_screen_long"):
        flags += ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
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
