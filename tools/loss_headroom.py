"""Runs tests/test_loss_kernels_gpu.py on the MI355X and prints, per kernel form and output, the largest derived bound and
the largest observed error in units of its own bound: the table of profiles/loss_kernels/README.md.
    python tools/loss_headroom.py"""
import collections
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rc = pytest.main(["-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_loss_kernels_gpu.py")])
    rows = sys.modules["test_loss_kernels_gpu"].HEADROOM
    agg = collections.OrderedDict()
    for kernel, case, form, output, bound, used in rows:
        a = agg.setdefault((kernel, output), [0.0, "", 0.0, 0])
        if used >= a[0]:
            a[0], a[1] = used, "%s, %s" % (case, form)
        a[2] = max(a[2], bound)
        a[3] += 1
    print("| kernels | output | largest bound | largest error / bound | at (case, form) | checks |\n|---|---|---|---|---|---|")
    for (kernel, output), a in agg.items():
        print("| %s | `%s` | %.3g | %.3f | %s | %d |" % (kernel, output, a[2], a[0], a[1], a[3]))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
