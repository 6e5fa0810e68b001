"""Which traversal kernel a launch gets (redner_amd/csrc/trace_plan.h: exec::plan_trace, seen through rdr_debug_trace_plan).

Every form of the kernels returns the same hits, so a slip in a threshold or a tier shows in no other test: it only changes
speed.  The table below is written out by hand from the rules -- family by queue size, stack tiers, index width, staging,
octant order, grid size -- with a case on each side of every boundary.  Each case passes an explicit rdr_tuning for every
numeric parameter (a field that is set wins over its environment variable)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM_LIB = os.path.join(ROOT, 'tests', 'hostsim', '_build', 'libredner_hostsim.so')

FIELDS = ('form', 'stack', 'short_index', 'stage_top', 'sorted', 'counting', 'blocks', 'rays_per_lane', 'idle_min', 'steps')
WIDE, REFILL, PLAIN = 0, 1, 2
BINARY, REFILL_OFF, REFILL_ALL, NO_LDS_TOP = 1 << 8, 1 << 6, 1 << 7, 1 << 9          # rdr_tune_flags (include/redner_amd.h)
# the facts of the issue's family table: a hierarchy like bunny_box's
FACTS = dict(num_nodes=30000, stack_need=22, has_wide=1, wide_stack_need=20)
TUNING = dict(wide_max_rays=1 << 19, refill_rays_per_lane=4, refill_idle_lanes=24, refill_steps=4, refill_order=2)


def wide(stack, blocks, counting=0):
    return (WIDE, stack, 0, 0, 0, counting, blocks, 0, 0, 0)


def refill(stack, short, blocks, k=4, sorted_=1, idle=24, steps=4):
    return (REFILL, stack, short, 0, sorted_, 0, blocks, k, idle, steps)


def plain(stack, short, top, blocks, counting=0):
    return (PLAIN, stack, short, top, 0, counting, blocks, 0, 0, 0)


def _call(lib, n, any_hit=0, coherent=0, counting=0, flags=0, out=True, **kw):
    from redner_amd import _capi
    facts = dict(FACTS, **{k: kw.pop(k) for k in list(kw) if k in FACTS})
    t = _capi.Tuning(flags=flags, **dict(TUNING, **kw))
    res = np.full(10, -7, np.int32)
    rc = lib.rdr_debug_trace_plan(facts['num_nodes'], facts['stack_need'], facts['has_wide'], facts['wide_stack_need'], n, any_hit,
                                  coherent, counting, ctypes.byref(t), res.ctypes.data_as(ctypes.c_void_p) if out else None)
    return rc, tuple(int(v) for v in res)


CASES = []


def case(name, expected, **kw):
    CASES.append(pytest.param(kw, expected, id=name))


# ---- family by queue size: 4-wide records up to 2^19 rays, refilling kernel from 2^22 on queues not marked coherent ----
for coh in (0, 1):
    c = 'coherent' if coh else 'incoherent'
    case('family_n1_' + c, wide(20, 1), n=1, coherent=coh)
    case('family_2^18-1_' + c, wide(20, 1024), n=(1 << 18) - 1, coherent=coh)
    case('family_2^18_' + c, wide(20, 1024), n=1 << 18, coherent=coh)
    case('family_2^19_' + c, wide(20, 2048), n=1 << 19, coherent=coh)
    case('family_2^19+1_' + c, plain(24, 1, 1, 2049), n=(1 << 19) + 1, coherent=coh)
    case('family_2^22-1_' + c, plain(24, 1, 1, 16384), n=(1 << 22) - 1, coherent=coh)
case('family_2^22_incoherent', refill(24, 1, 4096), n=1 << 22, coherent=0)
case('family_2^22_coherent', plain(24, 1, 1, 16384), n=1 << 22, coherent=1)
case('family_any_hit_same_rules', refill(24, 1, 4096), n=1 << 22, any_hit=1)
case('family_no_wide_records', plain(24, 1, 0, 4), n=1000, has_wide=0)

# ---- 4-wide tiers 12 / 16 / 20 / 24 / 32 / 48; deeper than 48: the binary records ----
for need, stack in ((12, 12), (13, 16), (16, 16), (17, 20), (20, 20), (21, 24), (24, 24), (25, 32), (32, 32), (33, 48), (48, 48)):
    case('wide_need_%d' % need, wide(stack, 4), n=1000, wide_stack_need=need)
case('wide_need_49', plain(24, 1, 0, 4), n=1000, wide_stack_need=49)

# ---- plain tiers 16 / 24 / 32 / 40, index width by the number of node records ----
for need, stack in ((16, 16), (17, 24), (24, 24), (25, 32), (32, 32), (33, 40), (40, 40)):
    case('plain_need_%d' % need, plain(stack, 1, 0, 4), n=1000, has_wide=0, stack_need=need)
case('plain_nodes_65535', plain(24, 1, 0, 4), n=1000, has_wide=0, num_nodes=65535)
case('plain_nodes_65536', plain(24, 0, 0, 4), n=1000, has_wide=0, num_nodes=65536)
case('plain_stage_2^18-1', plain(24, 1, 0, 1024), n=(1 << 18) - 1, flags=BINARY)
case('plain_stage_2^18', plain(24, 1, 1, 1024), n=1 << 18, flags=BINARY)

# ---- refilling tiers: (nodes, stack_need) -> plan.  41 entries are more than any refilling kernel has: the plain kernel ----
REFILL_TIERS_HYBRID = {
    (65535, 24): refill(24, 1, 1), (65535, 25): refill(16, 0, 1), (65535, 32): refill(16, 0, 1), (65535, 33): refill(16, 0, 1),
    (65535, 40): refill(16, 0, 1), (65535, 41): plain(40, 1, 0, 4),
    (65536, 24): refill(16, 0, 1), (65536, 25): refill(16, 0, 1), (65536, 32): refill(16, 0, 1), (65536, 33): refill(16, 0, 1),
    (65536, 40): refill(16, 0, 1), (65536, 41): plain(40, 0, 0, 4)}
REFILL_TIERS_NO_HYBRID = {
    (65535, 24): refill(24, 1, 1), (65535, 25): refill(32, 0, 1), (65535, 32): refill(32, 0, 1), (65535, 33): refill(40, 0, 1),
    (65535, 40): refill(40, 0, 1), (65535, 41): plain(40, 1, 0, 4),
    (65536, 24): refill(32, 0, 1), (65536, 25): refill(32, 0, 1), (65536, 32): refill(32, 0, 1), (65536, 33): refill(40, 0, 1),
    (65536, 40): refill(40, 0, 1), (65536, 41): plain(40, 0, 0, 4)}
for (nodes, need), expected in REFILL_TIERS_HYBRID.items():
    case('refill_hybrid_nodes_%d_need_%d' % (nodes, need), expected, n=1000, has_wide=0, flags=REFILL_ALL, num_nodes=nodes, stack_need=need)

# ---- flags and parameters ----
case('flag_trace_binary', plain(24, 1, 0, 4), n=1000, flags=BINARY)
case('flag_refill_off', plain(24, 1, 1, 16384), n=1 << 22, flags=REFILL_OFF)
case('flag_refill_off_beats_all', plain(24, 1, 1, 16384), n=1 << 22, flags=REFILL_OFF | REFILL_ALL)
case('flag_refill_all_coherent', refill(24, 1, 513), n=(1 << 19) + 1, coherent=1, flags=REFILL_ALL)
case('flag_refill_all_small_queue_stays_wide', wide(20, 4), n=1000, flags=REFILL_ALL)
case('flag_no_lds_top', plain(24, 1, 0, 2049), n=(1 << 19) + 1, flags=NO_LDS_TOP)
case('wide_max_at', wide(20, 4), n=1000, wide_max_rays=1000)
case('wide_max_above', plain(24, 1, 0, 4), n=1001, wide_max_rays=1000)
case('refill_k2_unsorted', refill(24, 1, 8192, k=2, sorted_=0), n=1 << 22, refill_rays_per_lane=2)
case('refill_k4_sorted', refill(24, 1, 4096, k=4, sorted_=1), n=1 << 22, refill_rays_per_lane=4)
case('refill_order_1_queue', refill(24, 1, 4096, sorted_=0), n=1 << 22, refill_order=1)
case('refill_order_2_octant', refill(24, 1, 4096, sorted_=1), n=1 << 22, refill_order=2)
case('refill_order_3_octant_axis', refill(24, 1, 4096, sorted_=1), n=1 << 22, refill_order=3)
case('refill_order_3_k2', refill(24, 1, 8192, k=2, sorted_=0), n=1 << 22, refill_order=3, refill_rays_per_lane=2)
case('refill_idle_steps', refill(24, 1, 4096, idle=8, steps=2), n=1 << 22, refill_idle_lanes=8, refill_steps=2)

# ---- counting: the instrumented variants exist for the wide and the plain kernel only ----
case('counting_wide', wide(20, 4, counting=1), n=1000, counting=1)
case('counting_plain', plain(24, 1, 1, 2049, counting=1), n=(1 << 19) + 1, counting=1)
case('counting_2^22_not_refill', plain(24, 1, 1, 16384, counting=1), n=1 << 22, counting=1)
case('counting_refill_all_not_refill', plain(24, 1, 0, 4, counting=1), n=1000, counting=1, flags=REFILL_ALL | BINARY)

# ---- grid sizes: 256 rays per workgroup, 256 k per workgroup of the refilling kernel ----
for n, blocks in ((1, 1), (256, 1), (257, 2)):
    case('blocks_wide_%d' % n, wide(20, blocks), n=n)
    case('blocks_plain_%d' % n, plain(24, 1, 0, blocks), n=n, flags=BINARY)
case('blocks_refill_k2_2^22', refill(24, 1, 8192, k=2, sorted_=0), n=1 << 22, refill_rays_per_lane=2)
case('blocks_refill_k2_2^22+1', refill(24, 1, 8193, k=2, sorted_=0), n=(1 << 22) + 1, refill_rays_per_lane=2)
case('blocks_refill_k4_2^22', refill(24, 1, 4096), n=1 << 22)
case('blocks_refill_k4_2^22+1', refill(24, 1, 4097), n=(1 << 22) + 1)


@pytest.mark.parametrize('kw,expected', CASES)
def test_plan_table(hostsim_backend, kw, expected):
    from redner_amd import _capi
    rc, got = _call(_capi.lib(), **kw)
    assert rc == 0, _capi.last_error()
    assert dict(zip(FIELDS, got)) == dict(zip(FIELDS, expected))


HYBRID_OFF_WORKER = r"""
import ctypes, json, sys
sys.path[:0] = [%(root)r, %(root)r + '/tests']
import test_trace_plan as t
from redner_amd import _capi
lib = _capi.load(%(lib)r)
out = []
for nodes in (65535, 65536):
    for need in (24, 25, 32, 33, 40, 41):
        rc, got = t._call(lib, n=1000, has_wide=0, flags=t.REFILL_ALL, num_nodes=nodes, stack_need=need)
        assert rc == 0
        out.append([nodes, need, list(got)])
print(json.dumps(out))
"""


def test_plan_refill_tiers_without_hybrid_stack(hostsim_backend):
    """RDR_TRACE_HYBRID=0 (read once per process, no field of rdr_tuning: one child process): the 32- and 40-entry LDS tiers."""
    r = subprocess.run([sys.executable, '-c', HYBRID_OFF_WORKER % {'root': ROOT, 'lib': HOSTSIM_LIB}],
                       env=dict(os.environ, RDR_TRACE_HYBRID='0'), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {(nodes, need): tuple(plan) for nodes, need, plan in json.loads(r.stdout.strip().splitlines()[-1])}
    assert got == REFILL_TIERS_NO_HYBRID


def test_plan_bad_arguments(hostsim_backend):
    from redner_amd import _capi
    lib = _capi.lib()
    for kw in (dict(n=0), dict(n=-1), dict(n=1000, out=False), dict(n=1000, num_nodes=-1), dict(n=1000, stack_need=-1)):
        rc, got = _call(lib, **kw)
        assert rc == 1, kw
        assert 'rdr_debug_trace_plan' in _capi.last_error()
        assert got == (-7,) * 10, kw          # nothing written
    assert lib.rdr_debug_scene_trace_plan(None, 1000, 0, 0, 0, None, None) == 1
