#!/usr/bin/env python3
"""Print the device timeline (queue, start, duration, gap, completion-to-completion interval) of the last N kernel
dispatches of a rocprofv3 --kernel-trace CSV, and for that window the union of the time the device was busy:
tools/kernel_timeline.py <dir-or-csv> [N]

Sweeps chained on two lanes (ipcr_scratch_chain_after) overlap: a dispatch's own duration then says little, the
interval from the previous completion to its own is what it added to the window, and busy time / dispatches is what
a step costs the device."""
import csv
import glob
import os
import sys

path = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
if os.path.isdir(path):
    path = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = list(csv.DictReader(open(path, newline="")))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
rows = rows[-n:]
t0 = int(rows[0]["Start_Timestamp"])
prev_end = t0
busy = 0          # union of [start, end) over the window
overlapped = 0    # dispatches that started before every earlier one had ended
for i, r in enumerate(rows):
    st, en = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print("q%-3s %-28s start %9.1f us  dur %8.1f us  gap-after-prev-end %8.1f us  end-to-end %8.1f us" % (
        r["Queue_Id"], r["Kernel_Name"][:28], (st - t0) / 1e3, (en - st) / 1e3, (st - prev_end) / 1e3,
        (en - prev_end) / 1e3 if i else (en - st) / 1e3))
    if i and st < prev_end:
        overlapped += 1
    busy += max(0, en - max(st, prev_end))
    prev_end = max(prev_end, en)
span = prev_end - t0
print("window: %d dispatches on queues {%s}, span %.1f us, busy (union) %.1f us = %.1f %%, busy / dispatch %.2f us, "
      "span / dispatch %.2f us, %d started before their predecessors had ended" % (
          len(rows), ", ".join(sorted({r["Queue_Id"] for r in rows})), span / 1e3, busy / 1e3, 100.0 * busy / max(span, 1),
          busy / 1e3 / len(rows), span / 1e3 / len(rows), overlapped))
