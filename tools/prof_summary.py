#!/usr/bin/env python
"""Summarise a rocprofv3 results.db (kernel trace) into a per-kernel table (stdout, markdown-ish).

prof_summary.py <dir or .db> [tail [marker]]: with `tail` (0 < tail < 1) only the kernels that start in the last `tail` of the
trace's span are counted (the steady state of a run whose warm-up and set-up are in the same trace); `marker`: a substring of a
kernel that runs once per step -- the table is then also given per step (dispatches and kernel time per call of that kernel)."""
import glob
import sqlite3
import sys

path = sys.argv[1]
dbs = glob.glob(path + "/**/*_results.db", recursive=True) if not path.endswith(".db") else [path]
db = sqlite3.connect(dbs[0])
cur = db.cursor()
tail = float(sys.argv[2]) if len(sys.argv) > 2 else None
marker = sys.argv[3] if len(sys.argv) > 3 else None
where = ""
if tail is not None:
    lo, hi = cur.execute("select min(start), max(end) from kernels").fetchone()
    where = "where start >= %d " % int(hi - tail * (hi - lo))
    print("\n# steady state: kernels that start in the last %g of the trace's span" % tail)
rows = cur.execute("select name, count(*), avg(end-start), min(end-start), max(end-start), sum(end-start) "
                   "from kernels " + where + "group by name order by sum(end-start) desc").fetchall()
tot = sum(r[5] for r in rows)
span = cur.execute("select min(start), max(end) from kernels " + where).fetchone()
if marker:
    steps = sum(r[1] for r in rows if marker in r[0])
    if steps:
        print("per step (%d calls of *%s*): %.1f dispatches, %.2f us of kernel time, %.2f us of wall time" %
              (steps, marker, sum(r[1] for r in rows) / steps, tot / 1e3 / steps, (span[1] - span[0]) / 1e3 / steps))
print("kernel-time total %.3f ms over a %.3f ms span (GPU busy %.1f%%), %d dispatches" %
      (tot / 1e6, (span[1] - span[0]) / 1e6, 100.0 * tot / (span[1] - span[0]), sum(r[1] for r in rows)))
print("%-100s %8s %10s %10s %10s %7s" % ("kernel", "calls", "avg_us", "min_us", "max_us", "share"))
for r in rows[:45]:
    print("%-100s %8d %10.2f %10.2f %10.2f %6.1f%%" % (r[0][:100], r[1], r[2] / 1e3, r[3] / 1e3, r[4] / 1e3, 100 * r[5] / tot))
