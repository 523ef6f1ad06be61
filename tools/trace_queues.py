#!/usr/bin/env python3
"""Hardware queues in use and per-launch averages of the proving chain's kernels from a rocprofv3 --kernel-trace CSV of bench.py,
over the same window of the prove() loop as tools/busy.py.  python tools/trace_queues.py <kernel_trace.csv>"""
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
q = [int(r["Start_Timestamp"]) for r in rows if "k_quotient<false>" in r["Kernel_Name"]]
lo, hi = q[int(len(q) * 0.3)], q[-1 - max(3, len(q) // 50)]
win = [r for r in rows if lo <= int(r["Start_Timestamp"]) <= hi]
qs = collections.Counter(r["Queue_Id"] for r in win)
print("distinct queues in the window of the prove loop: %d  (launches per queue: %s)" % (len(qs), dict(qs)))
by = collections.defaultdict(list)
for r in win:
    by[r["Kernel_Name"].split("(")[0].replace("void ", "")[:48]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for k in ("k_merkle_level", "k_merkle_top_coop", "k_merkle_leaves_coop", "k_fri_fold", "k_pow_grind", "__amd_rocclr_copyBuffer", "k_merkle_leaves<5>", "k_quotient<false>", "k_quotient<true>",
          "ntt_col_pass<9, false, true>", "ntt_row_pass<9, false, false>"):
    v = by.get(k)
    if v: print("  %-36s %6d launches  avg %8.1f us" % (k, len(v), sum(v) / len(v) / 1e3))
print("proofs in window: %d" % len([1 for r in win if "k_quotient<false>" in r["Kernel_Name"]]))
