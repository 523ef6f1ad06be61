#!/usr/bin/env python3
"""Runs tools/queue_probe (built from tools/queue_probe.hip) once plainly and once under `rocprofv3 --kernel-trace`, and counts
the distinct hardware queue ids that the kernels of each stream kind ran on.  python tools/queue_probe.py [out_dir]"""
import collections
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
exe = os.path.join(ROOT, "tools", "queue_probe")
if not os.path.exists(exe):
    sys.exit("build it first: hipcc --offload-arch=gfx950 -O2 -o tools/queue_probe tools/queue_probe.hip")
print("== alone ==", flush=True)
subprocess.run([exe], check=True, timeout=120)
out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="queue_probe_")
print("== under rocprofv3 --kernel-trace ==", flush=True)
subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", exe], check=True, timeout=300)
traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
if not traces:
    sys.exit("no kernel trace under " + out)
queues = collections.defaultdict(collections.Counter)
for r in csv.DictReader(open(traces[0])):
    m = re.search(r"k_probe<(\d+)>", r["Kernel_Name"])
    if m:
        queues[int(m.group(1))][r["Queue_Id"]] += 1
print("== distinct queue ids per kind (kernel trace) ==")
for kind in sorted(queues):
    print("kind %d  %2d distinct queues  %s" % (kind, len(queues[kind]), dict(sorted(queues[kind].items(), key=lambda kv: int(kv[0])))))
