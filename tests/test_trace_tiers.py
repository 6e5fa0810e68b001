"""Every traversal kernel tier (redner_amd/csrc/hip/trace.hip) on hierarchies that fill its stack.

exec::plan_trace picks an instantiation by family (4-wide records, plain binary, refilling), per-lane stack tier, entry width,
staged top and octant order; tests/test_trace_plan.py pins that choice.  What differs between the tiers is the stack: an LDS
column of STACK entries per lane, where one entry too many lands in another lane's column.  The `chain` scenes (tests/scenes.py)
have a hierarchy of a chosen depth, and the rays below walk it with the stack full: each case's facts and the highest stack index
its rays write are read through rdr_debug_trace_occupancy (the host builder's hierarchy and the shared walk templates over a
stack that shows every write) and ASSERTED, so a change to the builder that moves a case off its tier fails here instead of
silently losing the coverage.  rdr_debug_scene_trace then runs the planned kernel -- any tier, in one process -- and the hits
must equal the numpy brute force of tests/test_raytri.py: (shape, triangle) for closest hit, the verdict for any hit.

The harness legs (unmarked) check the cases, the plans, the reference and the hooks; its walk has a private stack, so the tiers
themselves run in the GPU legs only, on both builds.  `pytest -s` lists, per family and tier, the case that ran it, the planned
instantiation and the measured occupancy."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scenes
from redner_amd import _capi as K
from redner_amd.render_pytorch import RenderFunction
from test_raytri import _brute_force

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'trace_tiers.npz')
WIDE, REFILL, PLAIN = 0, 1, 2
FAMILY = {WIDE: 'wide', REFILL: 'refill', PLAIN: 'plain'}
PLAIN_FLAGS = K.TUNE_TRACE_BINARY | K.TUNE_REFILL_OFF
REFILL_FLAGS = K.TUNE_TRACE_BINARY | K.TUNE_REFILL_ALL
N_UNIQUE, N_FILL, N_RANDOM = 2048, 1536, 256          # the unique rays of a case: stack fillers, uniform ones, aimed ones
PERM = np.random.default_rng(7).permutation(N_UNIQUE)  # longer and shorter queues: the unique rays under this permutation, tiled
SENTINEL = 7


def _ptr(a):
    return ctypes.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)


def chain_rays(tri):
    """The N_UNIQUE rays of a case whose triangles are tri [n, 3, 3].
    Stack fillers (slot r < N_FILL): from -0.5 a (r even) or 2.5 a (r odd) along -+ the chain's axis a, perturbed by
    j U(-1, 1)^3 with j = 0 for r = 0, else 10^(-1 - 7 (r mod 64) / 64): those from the small end enter the nested box first and
    push one large leaf per level.  Then N_RANDOM uniform rays and rays aimed at vertices and edge midpoints (ties between
    leaves); every 17th slot has a finite tmax, every 29th is dead, as in test_raytri._rays."""
    rng = np.random.default_rng(2024)
    a = scenes.CHAIN_AXIS
    n = len(tri)
    r = np.arange(N_FILL)
    even = (r % 2 == 0)[:, None]
    j = 10.0 ** (-1.0 - 7.0 * (r % 64) / 64.0)
    j[0] = 0.0
    o = np.where(even, -0.5 * a, 2.5 * a)
    d = np.where(even, a, -a) + j[:, None] * rng.uniform(-1.0, 1.0, (N_FILL, 3))
    rest = N_UNIQUE - N_FILL
    flat = tri.reshape(-1, 3).astype(np.float64)
    o2 = rng.uniform(flat.min(0) - 0.5, flat.max(0) + 0.5, (rest, 3))
    d2 = rng.normal(size=(rest, 3))
    k = np.arange(rest - N_RANDOM)
    t, c = k % n, (k // n) % 3
    corner, nxt = tri[t, c].astype(np.float64), tri[t, (c + 1) % 3].astype(np.float64)
    half = len(k) // 2
    target = np.concatenate([corner[:half], 0.5 * (corner[half:] + nxt[half:])])
    d2[N_RANDOM:] = target - o2[N_RANDOM:]
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((N_UNIQUE, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-3, d, np.inf
    rays[::17, 7] = 1.5
    rays[::29, 7] = -1.0
    return rays


_REFERENCE = {}          # (ratio, n, scale) -> (rays, closest ids, any verdicts): computed once, shared, never written again


def reference(ratio, n, scale=1.0):
    key = (ratio, n, scale)
    if key not in _REFERENCE:
        sc = scenes.chain(torch.device('cpu'), ratio, n, scale=scale)
        v, ind = sc.shapes[0].vertices.numpy(), sc.shapes[0].indices.numpy()
        rays = chain_rays(v[ind.astype(np.int64)])
        closest = _brute_force([v], [ind], rays, 0)
        hit = closest[:, 0] >= 0          # a ray has an accepted triangle or it has none: the any-hit verdict
        assert hit[:N_FILL].mean() > 0.9 and not hit[::29].any()          # the comparison is not vacuous; dead slots miss
        for a in (rays, closest, hit):
            a.setflags(write=False)
        _REFERENCE[key] = (rays, closest, hit)
    return _REFERENCE[key]


class Case:
    """One chain scene on one library: its handle, its facts and per-ray stack occupancy, its rays in the Scene's memory."""

    def __init__(self, backend, dev, ratio, n, scale=1.0, fresh=True):
        self.name = 'chain(%g, %d)' % (ratio, n)
        self.dev, self.lib = dev, K.lib()
        self.rays, self.closest, self.hit = reference(ratio, n, scale)
        if fresh:
            backend.set_build_flags(K.BUILD_NO_REFIT)          # chains of one length share their index buffer: build, never refit
        try:
            sc = scenes.chain(dev, ratio, n, scale=scale)
            args = RenderFunction.serialize_scene(sc, 1, 1, sampler_type=backend.SamplerType.sobol, device=dev, backend=backend,
                                                  use_primary_edge_sampling=False, use_secondary_edge_sampling=False)
            self.u = RenderFunction.unpack_args((1, 2), args[0], args[1:])
        finally:
            if fresh:
                backend.set_build_flags(0)
        self.scene = self.u.scene._handle
        self.d_rays = torch.from_numpy(np.array(self.rays)).to(dev)
        self.occ = {}
        for wide in (0, 1):
            for any_hit in (0, 1):
                out = np.full(N_UNIQUE + 4, -1, np.int32)
                assert self.lib.rdr_debug_trace_occupancy(self.scene, _ptr(self.rays), N_UNIQUE, any_hit, wide, _ptr(out)) == 0, K.last_error()
                self.occ[wide, any_hit] = out[:N_UNIQUE]
                self.nodes, self.need, self.wide_nodes, self.wide_need = (int(x) for x in out[N_UNIQUE:])
        if fresh and dev.type != 'cpu':          # the occupancy was measured on the host builder's hierarchy: the kernels' is the same
            assert self.lib.rdr_debug_bvh_check(self.scene) == 0

    def occupancy(self, wide):
        """the highest stack index any ray writes, plus one (the same for closest and any hit, which is asserted)"""
        top = int(self.occ[wide, 0].max())
        assert top == int(self.occ[wide, 1].max())
        return top

    def plan(self, n, tuning, any_hit=0, coherent=0, counting=0):
        out = np.full(10, -7, np.int32)
        assert self.lib.rdr_debug_scene_trace_plan(self.scene, n, any_hit, coherent, counting, ctypes.byref(tuning), _ptr(out)) == 0
        return tuple(int(x) for x in out)

    def trace(self, index, tuning, any_hit, hybrid=-1, coherent=0, count=None, d_rays=None):
        """hits of the queue unique[index] (or of d_rays) -> int32 [n, 2]; slots the launch leaves alone keep SENTINEL"""
        if d_rays is None:
            d_rays = self.d_rays[torch.from_numpy(np.asarray(index, np.int64)).to(self.dev)].contiguous()
        n = len(d_rays)
        d_hits = torch.full((max(n, 1), 2), SENTINEL, dtype=torch.int32, device=self.dev)
        d_count = None if count is None else torch.tensor([count], dtype=torch.int32, device=self.dev)
        rc = self.lib.rdr_debug_scene_trace(self.scene, _ptr(d_rays), _ptr(d_hits), n, any_hit, coherent, ctypes.byref(tuning), hybrid,
                                            None if d_count is None else _ptr(d_count))
        assert rc == 0, K.last_error()
        return d_hits.cpu().numpy()[:n]

    def check(self, hits, index, any_hit, what):
        """`hits` of the queue unique[index] against the brute force (gathered, not recomputed)"""
        index = np.asarray(index)
        if any_hit:
            assert np.array_equal(hits[:, 0] >= 0, self.hit[index]), (self.name, what)
        else:
            assert np.array_equal(hits, self.closest[index]), (self.name, what)


_CASES = {}


def get_case(backend, dev, ratio, n):
    key = (K.library_path(), ratio, n)
    if key not in _CASES:
        _CASES[key] = Case(backend, dev, ratio, n)
    return _CASES[key]


def queue_index(n):
    return PERM[np.arange(n) % N_UNIQUE]


def tuning(flags=0, k=4, idle=24, steps=4, order=2, wide_max=1 << 19):
    """every numeric plan input stated (a field that is set wins over its environment variable)"""
    return K.Tuning(flags=flags, refill_rays_per_lane=k, refill_idle_lanes=idle, refill_steps=steps, refill_order=order, wide_max_rays=wide_max)


PROCESS_HYBRID = os.environ.get('RDR_TRACE_HYBRID', '1')[0] != '0'


def refill_stack(case, hybrid):
    """trace_plan.h: 16-bit entries and 24 of them while that covers the hierarchy; else the hybrid stack (16 LDS entries + scratch)
    or, with it off, 32 int entries up to a need of 32 and 40 beyond -> (stack, short_index)"""
    assert case.need <= 40
    if case.nodes < 65536 and case.need <= 24:
        return 24, 1
    on = PROCESS_HYBRID if hybrid < 0 else bool(hybrid)
    return (16 if on else (32 if case.need <= 32 else 40)), 0


def expected_plan(case, family, n, t, hybrid=-1, top=0, counting=0):
    """the launch of `n` rays under tuning `t`, from the case's facts, as test_trace_plan.py tabulates the rules"""
    if family == WIDE:
        tier = next(s for s in (12, 16, 20, 24, 32, 48) if case.wide_need <= s)
        return (WIDE, tier, 0, 0, 0, counting, (n + 255) // 256, 0, 0, 0)
    if family == PLAIN:
        tier = next(s for s in (16, 24, 32, 40) if case.need <= s)
        return (PLAIN, tier, 1, top, 0, counting, (n + 255) // 256, 0, 0, 0)
    k = t.refill_rays_per_lane
    stack, short = refill_stack(case, hybrid)
    order = t.refill_order or (int(os.environ['RDR_REFILL_SORT']) + 1 if 'RDR_REFILL_SORT' in os.environ else 2)      # 0: the default, octant order
    return (REFILL, stack, short, 0, int(order >= 2 and k == 4), 0, (n + 256 * k - 1) // (256 * k), k, t.refill_idle_lanes, t.refill_steps)


def assert_plan(case, family, n, t, hybrid=-1, top=0, counting=0, any_hit=0):
    """rdr_debug_scene_trace_plan reports the launch under the PROCESS's hybrid setting; rdr_debug_scene_trace's override changes the
    refilling kernel's int-entry tier alone, to what refill_stack() says -- which for a need above 24 is the plain kernel's tier of
    the same hierarchy, read through the hook as well"""
    got = case.plan(n, t, any_hit=any_hit, counting=counting)
    assert got == expected_plan(case, family, n, t, -1, top, counting), (case.name, FAMILY[family])
    want = expected_plan(case, family, n, t, hybrid, top, counting)
    if family == REFILL and hybrid == 0 and want[2] == 0:
        assert want[1] == case.plan(n, tuning(PLAIN_FLAGS))[1]
    return want


# ---- every tier of every family ------------------------------------------------------------------------------------------
# (tier, (ratio, n)): the case's need is asserted to land on the tier; TIER_NEEDS says which needs the list must contain
PLAIN_ROWS = [(16, (2, 24)), (16, (4, 15)), (24, (4, 16)), (24, (4, 23)), (32, (4, 25)), (32, (4, 39)), (40, (6, 38)), (40, (6, 52)),
              (40, (6, 55))]
WIDE_ROWS = [(12, (4, 12)), (16, (4, 13)), (16, (4, 16)), (20, (4, 17)), (20, (4, 20)), (24, (4, 21)), (24, (4, 24)), (32, (4, 25)),
             (32, (6, 38)), (48, (5, 33)), (48, (2, 53))]
# (stack, trace_hybrid, (ratio, n)): the 24-entry tier with 16-bit entries, the hybrid stack, the 32- and 40-entry tiers with it off
REFILL_ROWS = [(24, -1, (4, 16)), (24, -1, (4, 23)), (16, 1, (4, 25)), (16, 1, (6, 52)), (16, 1, (6, 55)), (32, 0, (4, 25)), (32, 0, (4, 39)),
               (40, 0, (6, 38)), (40, 0, (6, 52)), (40, 0, (6, 55))]
# a need equal to the tier where the builder gives one, and the first need above the tier below
TIER_NEEDS = {PLAIN: {16, 24, 32, 17, 25, 33}, WIDE: {12, 16, 20, 24, 32, 48, 13, 17, 21, 25, 33}, REFILL: {24, 32, 17, 25, 33}}
HYBRID_LDS = 16


def _tier_row(backend, dev, family, tier, hybrid, key):
    case = get_case(backend, dev, *key)
    wide = family == WIDE
    occ, need = case.occupancy(wide), case.wide_need if wide else case.need
    flags = {WIDE: 0, PLAIN: PLAIN_FLAGS, REFILL: REFILL_FLAGS}[family]
    for any_hit in (0, 1):
        for order in ((0, 1, 2, 3) if family == REFILL else (2,)):          # rdr_tuning::refill_order: default, queue, octant, octant x axis
            t = tuning(flags, order=order)
            plan = assert_plan(case, family, N_UNIQUE, t, hybrid, any_hit=any_hit)
            assert plan[1] == tier and plan[0] == family
            hits = case.trace(np.arange(N_UNIQUE), t, any_hit, hybrid)
            case.check(hits, np.arange(N_UNIQUE), any_hit, (FAMILY[family], tier, order))
    print('%-6s tier %2d%s  %-14s need %2d  occupancy %2d  plan (form, stack, 16-bit, staged, sorted) = %s'
          % (FAMILY[family], tier, {-1: '', 0: ' (hybrid off)', 1: ' (hybrid)'}[hybrid], case.name, need, occ, plan[:5]))
    return case, need, occ


def _tier_conditions(backend, dev):
    """The case list fills every tier (on the reference walk: the kernels use the same templates over their columns)."""
    for family, rows in ((PLAIN, [(t, -1, k) for t, k in PLAIN_ROWS]), (WIDE, [(t, -1, k) for t, k in WIDE_ROWS]), (REFILL, REFILL_ROWS)):
        wide = family == WIDE
        seen = {}
        for tier, hybrid, key in rows:
            case = get_case(backend, dev, *key)
            need, occ = (case.wide_need, case.occupancy(1)) if wide else (case.need, case.occupancy(0))
            # the bounds every kernel takes on trust are reached exactly on a chain, and never passed
            for kind in (0, 1):
                assert int(case.occ[int(wide), kind].max()) == (need - 1 if wide else need - 2), (case.name, FAMILY[family])
            if family == REFILL:
                assert refill_stack(case, hybrid)[0] == tier, case.name
                covers = 40 if tier == HYBRID_LDS else tier
            else:
                tiers = (12, 16, 20, 24, 32, 48) if wide else (16, 24, 32, 40)
                assert next(s for s in tiers if need <= s) == tier, (case.name, need)
                covers = tier
            assert occ <= covers - (1 if wide else 2)
            seen.setdefault(tier, []).append((need, occ))
        tiers = sorted(t for t in seen if not (family == REFILL and t == HYBRID_LDS))
        for lower, tier in zip([0] + tiers, tiers):
            assert max(occ for _, occ in seen[tier]) > lower, (FAMILY[family], tier)          # a walk that a lower tier could not hold
        if family == REFILL:
            assert max(occ for _, occ in seen[HYBRID_LDS]) >= HYBRID_LDS + 8                      # the spill half, eight entries deep
        needs = {need for rows_ in seen.values() for need, _ in rows_}
        assert TIER_NEEDS[family] <= needs, (FAMILY[family], sorted(TIER_NEEDS[family] - needs))


PLAIN_PARAMS = [pytest.param(PLAIN, t, -1, k, id='plain%d_chain_%g_%d' % (t, *k)) for t, k in PLAIN_ROWS]
WIDE_PARAMS = [pytest.param(WIDE, t, -1, k, id='wide%d_chain_%g_%d' % (t, *k)) for t, k in WIDE_ROWS]
REFILL_PARAMS = [pytest.param(REFILL, t, h, k, id='refill%d_%s_chain_%g_%d' % (t, {-1: 'short', 0: 'tiers', 1: 'hybrid'}[h], *k)) for t, h, k in REFILL_ROWS]
TIER_PARAMS = PLAIN_PARAMS + WIDE_PARAMS + REFILL_PARAMS
CPU = torch.device('cpu')


def _gpu():
    return torch.device('cuda:0')


@pytest.mark.parametrize('family,tier,hybrid,key', TIER_PARAMS)
def test_tier_harness(hostsim_backend, family, tier, hybrid, key):
    _tier_row(hostsim_backend, CPU, family, tier, hybrid, key)


@pytest.mark.gpu
@pytest.mark.parametrize('family,tier,hybrid,key', TIER_PARAMS)
def test_tier_gpu(gpu_backend, family, tier, hybrid, key):
    _tier_row(gpu_backend, _gpu(), family, tier, hybrid, key)


def test_case_list_fills_every_tier_harness(hostsim_backend):
    _tier_conditions(hostsim_backend, CPU)


@pytest.mark.gpu
def test_case_list_fills_every_tier_gpu(gpu_backend):
    _tier_conditions(gpu_backend, _gpu())


# ---- suspension with a deep stack: the refilling kernel resumes a ray from (cur, sp) and its column -------------------------
NEED_38 = (6, 52)
SUSPEND = [(1, 1, 1), (2, 4, 2), (4, 24, 4), (4, 64, 1)]          # (rays per lane, idle lanes, steps)


def _suspension(backend, dev, k, idle, steps, hybrid):
    case = get_case(backend, dev, *NEED_38)
    assert case.need == 38 and case.occupancy(0) == 36
    index = queue_index(9 * 256 + 1)          # (a lane's column is reused by its next ray; the last chunk holds one ray)
    for order in (1, 2):
        t = tuning(REFILL_FLAGS, k=k, idle=idle, steps=steps, order=order)
        plan = assert_plan(case, REFILL, len(index), t, hybrid)
        assert plan[1] == (16 if hybrid else 40) and plan[7:] == (k, idle, steps)
        for any_hit in (0, 1):
            case.check(case.trace(index, t, any_hit, hybrid), index, any_hit, ('suspend', k, idle, steps, hybrid, order))


@pytest.mark.parametrize('hybrid', [0, 1], ids=['tier40', 'hybrid'])
@pytest.mark.parametrize('k,idle,steps', SUSPEND)
def test_suspension_harness(hostsim_backend, k, idle, steps, hybrid):
    _suspension(hostsim_backend, CPU, k, idle, steps, hybrid)


@pytest.mark.gpu
@pytest.mark.parametrize('hybrid', [0, 1], ids=['tier40', 'hybrid'])
@pytest.mark.parametrize('k,idle,steps', SUSPEND)
def test_suspension_gpu(gpu_backend, k, idle, steps, hybrid):
    _suspension(gpu_backend, _gpu(), k, idle, steps, hybrid)


# ---- queue shapes and device-side counts --------------------------------------------------------------------------------
QUEUES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025]
FAMILY_CASE = {PLAIN: (PLAIN_FLAGS, (6, 52), -1), WIDE: (0, (2, 53), -1), REFILL: (REFILL_FLAGS, (6, 52), 1)}          # deep stacks


def _queue_shapes(backend, dev, family):
    flags, key, hybrid = FAMILY_CASE[family]
    case = get_case(backend, dev, *key)
    t = tuning(flags)
    for n in QUEUES + ([511, 513] if family == REFILL else []):          # (256 k +- 1 for k = 2, 4: 1023 and 1025 are in the list)
        index = queue_index(n)
        assert_plan(case, family, n, t, hybrid)
        for any_hit in (0, 1):
            case.check(case.trace(index, t, any_hit, hybrid), index, any_hit, (FAMILY[family], n))


def _device_counts(backend, dev, family):
    """if (count) n = min(*count, n) in all three kernels: slots at or past the count keep what was there, those below are right"""
    flags, key, hybrid = FAMILY_CASE[family]
    case = get_case(backend, dev, *key)
    t = tuning(flags)
    n = 600
    index = queue_index(n)
    assert_plan(case, family, n, t, hybrid)
    for count in (0, 1, n - 1, n, n + 5):
        live = min(count, n)
        for any_hit in (0, 1):
            hits = case.trace(index, t, any_hit, hybrid, count=count)
            assert (hits[live:] == SENTINEL).all(), (FAMILY[family], count)
            case.check(hits[:live], index[:live], any_hit, (FAMILY[family], 'count', count))


@pytest.mark.parametrize('family', [PLAIN, WIDE, REFILL], ids=['plain', 'wide', 'refill'])
def test_queue_shapes_harness(hostsim_backend, family):
    _queue_shapes(hostsim_backend, CPU, family)


@pytest.mark.gpu
@pytest.mark.parametrize('family', [PLAIN, WIDE, REFILL], ids=['plain', 'wide', 'refill'])
def test_queue_shapes_gpu(gpu_backend, family):
    _queue_shapes(gpu_backend, _gpu(), family)


@pytest.mark.parametrize('family', [PLAIN, WIDE, REFILL], ids=['plain', 'wide', 'refill'])
def test_device_counts_harness(hostsim_backend, family):
    _device_counts(hostsim_backend, CPU, family)


@pytest.mark.gpu
@pytest.mark.parametrize('family', [PLAIN, WIDE, REFILL], ids=['plain', 'wide', 'refill'])
def test_device_counts_gpu(gpu_backend, family):
    _device_counts(gpu_backend, _gpu(), family)


# ---- the staged top: the first 255 node records in LDS (191 in the sorted 32-entry refilling kernel) -------------------------
STAGED = [((4, 39), 77), ((1.5, 128), 255), ((1.5, 136), 265)]          # fewer records than the copy holds, exactly as many, more
STAGED_191 = [((2, 80), 153), ((1.5, 100), 199)]                        # needs of 25 .. 32 on either side of the smaller copy


def _staged_top(backend, dev, key, nodes):
    case = get_case(backend, dev, *key)
    assert case.nodes == nodes
    n = 1 << 18
    index = queue_index(n)
    d_rays = case.d_rays[torch.from_numpy(index).to(dev)].contiguous()
    for top, flags in ((1, PLAIN_FLAGS), (0, PLAIN_FLAGS | K.TUNE_TRACE_NO_LDS_TOP)):
        t = tuning(flags)
        assert_plan(case, PLAIN, n, t, top=top)
        for any_hit in (0, 1):
            case.check(case.trace(index, t, any_hit, d_rays=d_rays), index, any_hit, ('staged', top))


def _staged_191(backend, dev, key, nodes):
    case = get_case(backend, dev, *key)
    assert case.nodes == nodes and 24 < case.need <= 32
    index = queue_index(4 * 256 + 77)
    for order in (1, 2, 3):          # queue order: the 255-record copy; sorted: 191
        t = tuning(REFILL_FLAGS, order=order)
        plan = assert_plan(case, REFILL, len(index), t, 0)
        assert plan[1] == 32 and plan[4] == int(order > 1)
        for any_hit in (0, 1):
            case.check(case.trace(index, t, any_hit, 0), index, any_hit, ('staged 191', order))


@pytest.mark.parametrize('key,nodes', STAGED, ids=['below', 'exactly', 'above'])
def test_staged_top_harness(hostsim_backend, key, nodes):
    _staged_top(hostsim_backend, CPU, key, nodes)


@pytest.mark.gpu
@pytest.mark.parametrize('key,nodes', STAGED, ids=['below', 'exactly', 'above'])
def test_staged_top_gpu(gpu_backend, key, nodes):
    _staged_top(gpu_backend, _gpu(), key, nodes)


@pytest.mark.parametrize('key,nodes', STAGED_191, ids=['below', 'above'])
def test_staged_top_of_sorted_refill_harness(hostsim_backend, key, nodes):
    _staged_191(hostsim_backend, CPU, key, nodes)


@pytest.mark.gpu
@pytest.mark.parametrize('key,nodes', STAGED_191, ids=['below', 'above'])
def test_staged_top_of_sorted_refill_gpu(gpu_backend, key, nodes):
    _staged_191(gpu_backend, _gpu(), key, nodes)


# ---- a wide form deeper than the widest tier: the binary kernel ---------------------------------------------------------------
def _wide_fallback(backend, dev):
    case = get_case(backend, dev, 2, 128)
    assert case.wide_need > 48 and case.wide_nodes > 0 and case.occupancy(1) > 48
    index = queue_index(1000)
    t = tuning(0)
    assert case.plan(len(index), t) == expected_plan(case, PLAIN, len(index), t)
    for any_hit in (0, 1):
        case.check(case.trace(index, t, any_hit), index, any_hit, 'wide fallback')


def test_wide_fallback_harness(hostsim_backend):
    _wide_fallback(hostsim_backend, CPU)


@pytest.mark.gpu
def test_wide_fallback_gpu(gpu_backend):
    _wide_fallback(gpu_backend, _gpu())


# ---- one refit ---------------------------------------------------------------------------------------------------------
def _refit(backend, dev):
    """The need-24 chain, then the same connectivity with every vertex scaled by 1.01: the second hierarchy is a refit of the first
    (on the GPU; the harness reports every hierarchy as not built by kernels), its stack needs are the first build's, and they
    cover what a fresh build of the moved triangles needs; hits are the brute force's on the moved triangles."""
    first = Case(backend, dev, 4, 23)          # a build of its own: the topology cache holds it
    assert first.need == 24
    moved = Case(backend, dev, 4, 23, scale=1.01, fresh=False)
    assert moved.lib.rdr_debug_bvh_check(moved.scene) == -1
    index = np.arange(N_UNIQUE)
    for family, flags in ((WIDE, 0), (PLAIN, PLAIN_FLAGS), (REFILL, REFILL_FLAGS)):
        t = tuning(flags)
        plan = moved.plan(N_UNIQUE, t)
        assert plan == first.plan(N_UNIQUE, t) and plan[0] == family
        assert (40 if (family == REFILL and plan[1] == 16) else plan[1]) >= (moved.wide_need if family == WIDE else moved.need)
        for any_hit in (0, 1):
            moved.check(moved.trace(index, t, any_hit), index, any_hit, ('refit', FAMILY[family]))


def test_refit_harness(hostsim_backend):
    _refit(hostsim_backend, CPU)


@pytest.mark.gpu
def test_refit_gpu(gpu_backend):
    _refit(gpu_backend, _gpu())


# ---- the counting instantiations: the numerator of bench.py's roofline figures ---------------------------------------------
TALLY_QUEUES = [N_UNIQUE, 1000]          # whole waves; a last wave of 40 lanes (wave_tally's other branch)
TALLY_STAGED = ((6, 52), (1 << 18) + 37)          # the counting plain kernel with the staged top, its last wave partial too


def tally_runs():
    """(name, family, case key, queue length)"""
    runs = []
    for family, rows in ((PLAIN, PLAIN_ROWS), (WIDE, WIDE_ROWS)):
        for tier in sorted({t for t, _ in rows}):
            key = [k for t, k in rows if t == tier][-1]          # the deepest case of the tier
            runs += [('%s%d_chain_%g_%d_n%d' % (FAMILY[family], tier, *key, n), family, key, n) for n in TALLY_QUEUES]
    runs.append(('plain40_staged_chain_%g_%d_n%d' % (*TALLY_STAGED[0], TALLY_STAGED[1]), PLAIN, *TALLY_STAGED))
    return runs


def tallies(backend, dev):
    """name -> [[rays, node records, triangle tests, 4-wide records] for closest, the same for any hit], exact integers"""
    lib = K.lib()
    out = {}
    lib.rdr_trace_stats_enable(0, 1)
    try:
        for name, family, key, n in tally_runs():
            case = get_case(backend, dev, *key)
            t = tuning(PLAIN_FLAGS if family == PLAIN else 0)
            index = queue_index(n)
            assert_plan(case, family, n, t, top=int(family == PLAIN and n >= 1 << 18), counting=1)
            lib.rdr_trace_stats_reset()
            for any_hit in (0, 1):
                case.check(case.trace(index, t, any_hit), index, any_hit, name)
            s = K.TraceStats()
            lib.rdr_trace_stats_get(ctypes.byref(s))
            assert s.closest_launches == 1 and s.any_launches == 1
            out[name] = np.array([[s.closest_rays, s.closest_nodes, s.closest_tris, s.closest_wide_nodes],
                                  [s.any_rays, s.any_nodes, s.any_tris, s.any_wide_nodes]], np.int64)
            assert out[name][0, 0] == n and out[name][1, 0] == n and out[name][0, 2] > 0
            assert (out[name][:, 1] > 0).all() == (family == PLAIN) and (out[name][:, 3] > 0).all() == (family == WIDE)
    finally:
        lib.rdr_trace_stats_enable(0, 0)
        lib.rdr_trace_stats_reset()
    return out


def _tallies_equal_golden(backend, dev):
    gold = np.load(GOLDEN)
    got = tallies(backend, dev)
    assert sorted(got) == sorted(gold.files)
    for name in got:
        assert np.array_equal(got[name], gold[name]), (name, got[name].tolist(), gold[name].tolist())


def test_counting_tallies_harness(hostsim_backend):
    """the harness still produces tests/golden/trace_tiers.npz (tests/golden/make_trace_tiers.py)"""
    _tallies_equal_golden(hostsim_backend, CPU)


@pytest.mark.gpu
def test_counting_tallies_gpu(gpu_backend):
    """the counting kernels tally what the harness tallies with the same walk templates: exact integers"""
    _tallies_equal_golden(gpu_backend, _gpu())


def test_hook_arguments(hostsim_backend):
    lib = K.lib()
    assert lib.rdr_debug_scene_trace(None, None, None, 0, 0, 0, None, -1, None) == 1 and 'rdr_debug_scene_trace' in K.last_error()
    assert lib.rdr_debug_trace_occupancy(None, None, 0, 0, 0, None) == 1 and 'rdr_debug_trace_occupancy' in K.last_error()
    case = get_case(hostsim_backend, CPU, 4, 12)
    hits = np.zeros((4, 2), np.int32)
    assert lib.rdr_debug_scene_trace(case.scene, _ptr(case.rays), _ptr(hits), 4, 0, 0, None, 2, None) == 1 and 'trace_hybrid' in K.last_error()
    assert lib.rdr_debug_scene_trace(case.scene, None, _ptr(hits), 4, 0, 0, None, -1, None) == 1
    assert lib.rdr_debug_scene_trace(case.scene, _ptr(case.rays), _ptr(hits), -1, 0, 0, None, -1, None) == 1
    assert lib.rdr_debug_trace_occupancy(case.scene, _ptr(case.rays), 4, 0, 0, None) == 1
