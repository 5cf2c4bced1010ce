"""The last N kernels (default 45) of a `rocprofv3 --kernel-trace --output-format csv -d DIR` run in time order: start (us from the
first one shown), duration, gap to the end of the kernel before.  python tools/step_timeline.py DIR [N]"""
import csv, glob, sys
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
ker = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
n = int(sys.argv[2]) if len(sys.argv) > 2 else 45
ker = ker[-n:]
t0, prev = ker[0][0], ker[0][0]
for s, e, name in ker:
    print("%9.1f  dur %7.1f  gap %6.1f  %s" % ((s - t0) / 1e3, (e - s) / 1e3, (s - prev) / 1e3, name[:70]))
    prev = e
