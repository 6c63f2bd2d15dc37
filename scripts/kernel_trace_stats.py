"""Per-kernel launches, average, median, standard deviation and minimum (us) from a rocprofv3 --kernel-trace CSV:
python scripts/kernel_trace_stats.py TRACE.csv OUT.csv   (the profiles/r*_kernel_stats_*.csv files; template arguments are dropped)"""
import csv
import re
import statistics as st
import sys

by = {}
for r in csv.DictReader(open(sys.argv[1])):
    name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Kernel_Name"]))
    by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
with open(sys.argv[2], "w") as f:
    f.write('"Name","Calls","AverageUs","MedianUs","StdDevUs","MinUs"\n')
    for name in sorted(by):
        v = by[name]
        f.write('"%s",%d,%.2f,%.2f,%.2f,%.2f\n' % (name, len(v), st.mean(v), st.median(v), st.pstdev(v), min(v)))
