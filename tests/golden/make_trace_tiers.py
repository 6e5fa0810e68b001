"""Writes tests/golden/trace_tiers.npz: the tallies of the counting traversal (node records, triangle tests, 4-wide records, rays)
for one chain case per stack tier, by the CPU debugging harness -- the walk templates of csrc/bvh.h with counters, which the
counting kernels instantiate as well (tests/test_trace_tiers.py: test_counting_tallies_*).

    python tests/golden/make_trace_tiers.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np          # noqa: E402
import torch                # noqa: E402


def main():
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'tests', 'hostsim'), '-j8'], stdout=subprocess.DEVNULL)
    from redner_amd import _capi
    _capi.load(os.path.join(ROOT, 'tests', 'hostsim', '_build', 'libredner_hostsim.so'))
    from redner_amd import redner
    import test_trace_tiers as t
    got = t.tallies(redner, torch.device('cpu'))
    np.savez(t.GOLDEN, **got)
    for name in sorted(got):
        print(name, got[name].tolist())


if __name__ == '__main__':
    main()
