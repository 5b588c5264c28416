"""Dispatches and kernel time of one window of a rocprofv3 kernel trace (`--kernel-trace`, the rocpd SQLite database it
writes by default): the timed pass of a tool that prints its CLOCK_MONOTONIC window (tools/eval_bench.py
`timed_pass_monotonic_ns`), per batch, with the kernels that take the most time in it and their launch shapes.

    python tools/trace_window.py RESULTS.db T0 T1 BATCHES [TOP]
"""
import sqlite3
import sys
from collections import defaultdict


def main():
    path, t0, t1, nb = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    top = int(sys.argv[5]) if len(sys.argv) > 5 else 15
    db = sqlite3.connect(path)
    rows = db.execute("select name, start, end, grid_x, grid_y, grid_z, workgroup_x from kernels where start >= ? and end <= ?",
                      (t0, t1)).fetchall()
    busy = sum(e - s for _, s, e, *_ in rows)
    per = defaultdict(lambda: [0, 0, set()])
    for name, s, e, gx, gy, gz, wx in rows:
        k = per[name]
        k[0] += 1
        k[1] += e - s
        k[2].add((gx // max(wx, 1), gy, gz))
    print("window %.3f ms, %d batches: %.1f dispatches / batch, kernel time %.3f ms / batch (%.3f ms wall / batch)"
          % ((t1 - t0) / 1e6, nb, len(rows) / nb, busy / nb / 1e6, (t1 - t0) / nb / 1e6))
    for name, (c, t, grids) in sorted(per.items(), key=lambda kv: -kv[1][1])[:top]:
        g = sorted(grids)[:3]
        print("%9.1f us/batch %6.1f calls/batch  %s  grids %s%s" % (t / nb / 1e3, c / nb, name[:110], g,
                                                                     " ..." if len(grids) > 3 else ""))


if __name__ == "__main__":
    main()
