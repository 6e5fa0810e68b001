"""The three integer primitives that decide order, each on its own and bit for bit:

  * the stable stream compaction (compact_count / compact_scan / compact_scatter, compact_dev, compact; csrc/hip/exec.h) through
    rdr_debug_compact -- Sobol' slots are assigned by compacted rank, so a misplaced item is another sample, not a crash;
  * the walk kernels with lane refill (persistent_kernel, chunked_kernel, and the plain stage_kernel beside them) through
    rdr_debug_walk, over a walker that counts every begin and finish per item and folds item and step numbers into a checksum;
  * the stable 64-bit LSD radix sort of the edge hierarchies' builder (radix_hist / radix_scan / radix_scatter,
    csrc/edges_gpu.cpp) through rdr_debug_sort_pairs.

Everything is integers and every comparison is np.array_equal against a few lines of numpy in this file: there is no tolerance.
Output arrays travel to the hook pre-filled with sentinels and come back whole, so a store outside the expected range shows.
The sizes aim at the paths the code takes by size: the wave (64), the workgroup (256), the compaction tile (1024) and its scan
with more than 256 workgroup counts (n > 262 144), the sort tile (2048), more chunks than the launch has waves, a device count
below / at / above the bound, an empty list, a lap of the 4096-entry counter ring.

On the CPU harness the primitives are `for` loops and std::stable_sort (tests/hostsim/exec.h, edges_gpu_stub.cpp): the legs on
`hostsim_backend` hold those stand-ins -- what the oracle is compared with -- to the same contract, and check this file's own
references and the hooks' argument checks; the legs on `gpu_backend` check the kernels, on both builds.

What the legs were seen to catch (each change built once into a scratch library, never committed; one run each):
    compact_scatter without the sum over earlier waves      (GPU) every compaction case that keeps items in more than one wave
                                                            of a workgroup: 20 of 23 -- all but the sizes legs of none / last / first
    radix_scatter_kernel without that sum                   (GPU) all 18 sort cases
    the harness walk skipping finish when begin is false    (harness) the 26 walk cases that hold an item of length 0: zeros,
                                                            alt01, mix, more items than lanes, device counts, gate, ring lap"""
import numpy as np
import pytest
import torch                                              # noqa: F401  (the hooks run on torch's current stream)

from redner_amd import _capi

SENT_OUT, SENT_POS = -77, -99                             # what `out` / `pos_out` hold where nothing may be written
BEGUN0, FINISHED0, STEPS0, ACC0 = 3, 7, -5, 0xDEADBEEF    # pre-fill of the walk's four outputs
BOUNDARY = (1, 63, 64, 65, 255, 256, 257)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _lib(backend):
    lib = _capi.lib()
    backend._use_torch_stream(lib, _capi.is_product_library(), 0)
    return lib


# ---- compaction -------------------------------------------------------------------------------------------------------------------------
COMPACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 262144, 262145, 1048577)
FORM_SIZES = (1025, 262145)                               # a boundary of the tile, and one past the scan's 256 counts
KEEPS = ('none', 'all', 'half', 'sparse', 'waves', 'last', 'first')


def _keep(kind, n, rng):
    """The predicate's table over the values 0 .. n - 1."""
    i = np.arange(n)
    k = {'none': lambda: np.zeros(n, bool), 'all': lambda: np.ones(n, bool), 'half': lambda: rng.random(n) < 0.5,
         'sparse': lambda: rng.random(n) < 0.02, 'waves': lambda: (i // 64) % 2 == 0, 'last': lambda: i == n - 1,
         'first': lambda: i == 0}[kind]()
    return k.astype(np.uint8)


def _compact(backend, n, keep, count=-1, inp=None, append=None, dyn_inc=0, scratch=0, host_form=0, pos=False, sentinel=SENT_OUT,
             expect=0):
    """One call of the hook, checked against the reference.  Returns (out, count after the call)."""
    lib = _lib(backend)
    keep = np.ascontiguousarray(keep, np.uint8)
    inp = None if inp is None else np.ascontiguousarray(inp, np.int32)
    app_upper, app_count = append if append is not None else (-1, 0)
    total = max(app_upper, 0) + n
    out = np.full(total, sentinel, np.int32)
    pos_out = np.full(total, SENT_POS, np.int32) if pos else None
    dyn0 = 11
    result = np.asarray([-1, -1, dyn0, -2], np.int32)
    rc = lib.rdr_debug_compact(n, count, _ptr(inp), _ptr(keep), len(keep), app_upper, app_count, dyn_inc, scratch, host_form,
                               _ptr(out), _ptr(pos_out), _ptr(result))
    assert rc == expect, lib.rdr_last_error()
    if expect:
        assert 'rdr_debug_compact' in lib.rdr_last_error().decode()
        assert (out == sentinel).all() and result.tolist() == [-1, -1, dyn0, -2]
        assert pos_out is None or (pos_out == SENT_POS).all()
        return out, None
    # the reference
    m = n if count < 0 else min(count, n)
    vals = (np.arange(n, dtype=np.int32) if inp is None else inp)[:m]
    mask = keep[vals] != 0
    kept, positions = vals[mask], np.flatnonzero(mask)
    base = app_count if append is not None else 0
    want = np.full(total, sentinel, np.int32)
    want[base:base + len(kept)] = kept
    assert np.array_equal(out, want), (n, count, np.flatnonzero(out != want)[:8])
    if pos:
        want_pos = np.full(total, SENT_POS, np.int32)
        want_pos[base:base + len(kept)] = positions
        assert np.array_equal(pos_out, want_pos), (n, count, np.flatnonzero(pos_out != want_pos)[:8])
    assert result[0] == base + len(kept) and result[1] == n + max(app_upper, 0), (n, count, result)
    assert result[2] == dyn0 + (dyn_inc if m > 0 else 0), (n, count, result)
    assert result[3] == (len(kept) if host_form else -1), (n, count, result)
    return out, int(result[0])


def _compact_sizes_case(backend, kind):
    for n in COMPACT_SIZES:
        rng = np.random.default_rng(100 + 7 * KEEPS.index(kind) + n)
        keep = _keep(kind, n, rng)
        _compact(backend, n, keep, pos=True)
        if n <= 4096 or n == 262145:
            _compact(backend, n, keep, count=n)            # the same through a device-side count


@pytest.mark.parametrize('kind', KEEPS)
def test_compact_sizes_hostsim(hostsim_backend, kind):
    _compact_sizes_case(hostsim_backend, kind)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KEEPS)
def test_compact_sizes_gpu(gpu_backend, kind):
    _compact_sizes_case(gpu_backend, kind)


def _form_in(backend, n, rng):
    keep_len = n + 13                                      # values the identity never produces, duplicates, any order
    for kind in ('half', 'sparse', 'waves'):
        _compact(backend, n, _keep(kind, keep_len, rng), inp=rng.integers(0, keep_len, n), pos=True)
    _compact(backend, n, _keep('half', keep_len, rng), inp=rng.permutation(keep_len)[:n].astype(np.int32), count=n - 1, pos=True)


def _form_count(backend, n, rng):
    for kind in ('all', 'half', 'last', 'first'):
        keep = _keep(kind, n, rng)
        for count in (0, 1, n - 1, n, n + 5):
            _compact(backend, n, keep, count=count, pos=True, dyn_inc=7)
            _compact(backend, n, keep, count=count, inp=rng.integers(0, n, n))


def _form_append(backend, n, rng):
    for kind in ('all', 'half', 'sparse', 'none'):
        keep = _keep(kind, n, rng)
        for app_upper in (7, 300):
            for app_count in (0, 7, app_upper):
                _compact(backend, n, keep, append=(app_upper, app_count), pos=True)
                _compact(backend, n, keep, append=(app_upper, app_count), count=n - 1, dyn_inc=3)
    _compact(backend, n, _keep('half', n, rng), append=(0, 0))          # an empty earlier list with a zero bound


def _form_pos(backend, n, rng):
    for kind in KEEPS:
        _compact(backend, n, _keep(kind, n, rng), pos=True, count=n + 5)


def _form_scratch(backend, n, rng):
    for kind in ('half', 'waves'):
        keep = _keep(kind, n, rng)
        _compact(backend, n, keep, scratch=1, pos=True)
        _compact(backend, n, keep, scratch=0, count=n)
        _compact(backend, n, keep, scratch=1, count=n, append=(7, 7), dyn_inc=7)


def _form_dyn(backend, n, rng):
    for kind in ('none', 'half'):
        keep = _keep(kind, n, rng)
        for count in (-1, 0, 1, n):
            for inc in (7, -2):
                _compact(backend, n, keep, count=count, dyn_inc=inc)


def _form_chain(backend, n, rng):
    """Two compactions, the second fed the first's kept list and count.  The first's free slots hold a value (n) that the second
    predicate would KEEP: reading past the first count shows."""
    keep1 = np.append(_keep('half', n, rng), 0).astype(np.uint8)
    keep2 = np.append(rng.random(n) < 0.3, 1).astype(np.uint8)
    out1, c1 = _compact(backend, n, keep1, sentinel=n)
    assert 0 < c1 < n and (out1[c1:] == n).all()
    out2, c2 = _compact(backend, n, keep2, count=c1, inp=out1, pos=True)
    want = np.flatnonzero((keep1[:n] != 0) & (keep2[:n] != 0))
    assert c2 == len(want) and np.array_equal(out2[:c2], want)


FORMS = {'in': _form_in, 'count': _form_count, 'append': _form_append, 'pos': _form_pos, 'scratch': _form_scratch, 'dyn': _form_dyn,
         'chain': _form_chain}
FORM_CASES = [(f, n) for f in FORMS for n in FORM_SIZES]
FORM_IDS = ['%s-%d' % c for c in FORM_CASES]


def _compact_form_case(backend, form, n):
    FORMS[form](backend, n, np.random.default_rng(900 + 31 * list(FORMS).index(form) + n))


@pytest.mark.parametrize('case', FORM_CASES, ids=FORM_IDS)
def test_compact_forms_hostsim(hostsim_backend, case):
    _compact_form_case(hostsim_backend, *case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', FORM_CASES, ids=FORM_IDS)
def test_compact_forms_gpu(gpu_backend, case):
    _compact_form_case(gpu_backend, *case)


def _compact_host_form_case(backend):
    """exec::compact spins on the ticket that the scan publishes: small, then large (the scratch grows in between), then small."""
    for round_, n in enumerate((10, 1048577, 10)):
        rng = np.random.default_rng(40 + round_)
        for kind in ('half', 'none', 'all'):
            _compact(backend, n, _keep(kind, n, rng), host_form=1)
        _compact(backend, n, _keep('half', n + 5, rng), inp=rng.integers(0, n + 5, n), host_form=1)
    for n in BOUNDARY + (1023, 1024, 1025):
        _compact(backend, n, _keep('half', n, np.random.default_rng(n)), host_form=1)


def test_compact_host_form_hostsim(hostsim_backend):
    _compact_host_form_case(hostsim_backend)


@pytest.mark.gpu
def test_compact_host_form_gpu(gpu_backend):
    _compact_host_form_case(gpu_backend)


def _compact_refusal_case(backend):
    n = 100
    keep = np.ones(n, np.uint8)
    bad_in = np.arange(n, dtype=np.int32)
    bad_in[57] = n
    neg_in = np.arange(n, dtype=np.int32)
    neg_in[0] = -1
    _compact(backend, n, keep, inp=bad_in, expect=1)                    # a value past the keep table
    _compact(backend, n, keep, inp=neg_in, expect=1)
    _compact(backend, n, keep, inp=bad_in, count=10, expect=1)          # ... also where the count would never reach it
    _compact(backend, n, keep[:n - 1], expect=1)                        # identity needs keep_len >= upper
    _compact(backend, n, keep, append=(5, 6), expect=1)                 # append_count > append_upper
    _compact(backend, n, keep, append=(5, -1), expect=1)
    _compact(backend, n, keep, scratch=2, expect=1)
    _compact(backend, n, keep, scratch=-1, expect=1)
    _compact(backend, n, keep, host_form=2, expect=1)
    _compact(backend, n, keep, host_form=1, count=n, expect=1)          # the host form: host count, no append / dyn / pos, scratch 0
    _compact(backend, n, keep, host_form=1, append=(5, 0), expect=1)
    _compact(backend, n, keep, host_form=1, dyn_inc=7, expect=1)
    _compact(backend, n, keep, host_form=1, pos=True, expect=1)
    _compact(backend, n, keep, host_form=1, scratch=1, expect=1)
    lib = _lib(backend)
    out, result = np.full(4, SENT_OUT, np.int32), np.zeros(4, np.int32)
    for args in ((-1, -1, None, _ptr(keep), n), ((1 << 24) + 1, -1, None, _ptr(keep), n), (4, -1, None, None, n),
                 (4, -1, None, _ptr(keep), -1), (4, 1 << 30, None, _ptr(keep), n)):
        assert lib.rdr_debug_compact(*args, -1, 0, 0, 0, 0, _ptr(out), None, _ptr(result)) == 1
        assert 'rdr_debug_compact' in lib.rdr_last_error().decode()
    assert lib.rdr_debug_compact(4, -1, None, _ptr(keep), n, -1, 0, 0, 0, 0, None, None, _ptr(result)) == 1
    assert lib.rdr_debug_compact(4, -1, None, _ptr(keep), n, -1, 0, 0, 0, 0, _ptr(out), None, None) == 1
    assert (out == SENT_OUT).all() and not result.any()
    _compact(backend, n, keep, inp=np.full(n, n - 1, np.int32), append=(5, 5), pos=True)      # and the edges of the range are in it


def test_compact_hook_refuses_out_of_range_hostsim(hostsim_backend):
    _compact_refusal_case(hostsim_backend)


@pytest.mark.gpu
def test_compact_hook_refuses_out_of_range_gpu(gpu_backend):
    _compact_refusal_case(gpu_backend)


# ---- walks ------------------------------------------------------------------------------------------------------------------------------
PERSISTENT, CHUNKED, PLAIN = 0, 1, 2
WALK_SIZES = BOUNDARY + (100003,)
LENS = ('ones', 'zeros', 'alt01', 'mix', 'long_per_64', 'last_long')
# (kind, items_per_lane, idle_min, steps): the persistent walk, then the chunked walk with the production descent's parameters,
# the leaves walk's, the pickh_walk_params row of test_tuning.py, and the two corners of what rdr_tuning clamps to
WALKERS = [(PERSISTENT, 1, 1, 1), (CHUNKED, 1, 8, 8), (CHUNKED, 1, 8, 2), (CHUNKED, 4, 32, 3), (CHUNKED, 64, 64, 1), (CHUNKED, 1, 1, 1024)]
WALKER_IDS = ['persistent'] + ['chunked-%d-%d-%d' % w[1:] for w in WALKERS[1:]]


def _lens(kind, n, rng):
    i = np.arange(n)
    if kind == 'ones':
        v = np.ones(n)
    elif kind == 'zeros':
        v = np.zeros(n)
    elif kind == 'alt01':
        v = i % 2
    elif kind == 'mix':                                    # nothing to walk with p = 0.1, else geometric (mean 20), 1 % very long
        v = rng.geometric(1.0 / 20.0, n)
        v[rng.random(n) < 0.1] = 0
        v[rng.random(n) < 0.01] = 3000
    elif kind == 'long_per_64':
        v = np.where(i % 64 == 0, 2000, 1)
    elif kind == 'last_long':
        v = np.ones(n)
        v[n - 1] = 4000
    else:
        assert kind == 'short'                             # 0 .. 3 steps: for the launches with more items than lanes
        v = rng.integers(0, 4, n)
    return np.minimum(v, 65536).astype(np.int32)


def _walk(backend, walker, lens, count=-1, gate_closed=0, repeat=1, expect=0):
    lib = _lib(backend)
    kind, ipl, idle, steps = walker
    lens = np.ascontiguousarray(lens, np.int32)
    n = len(lens)
    begun, finished = np.full(n, BEGUN0, np.int32), np.full(n, FINISHED0, np.int32)
    taken, acc = np.full(n, STEPS0, np.int32), np.full(n, ACC0, np.uint32)
    rc = lib.rdr_debug_walk(kind, n, count, _ptr(lens), ipl, idle, steps, gate_closed, repeat, _ptr(begun), _ptr(finished), _ptr(taken),
                            _ptr(acc))
    assert rc == expect, lib.rdr_last_error()
    m = n if count < 0 else min(count, n)
    if expect:
        assert 'rdr_debug_walk' in lib.rdr_last_error().decode()
    if expect or gate_closed:
        m = 0                                              # nothing begun and nothing finished
    ran = np.arange(n) < m
    ctx = (walker, n, count, repeat)
    assert np.array_equal(begun, np.where(ran, BEGUN0 + repeat, BEGUN0)), (ctx, np.flatnonzero(begun != np.where(ran, BEGUN0 + repeat, BEGUN0))[:8])
    assert np.array_equal(finished, np.where(ran, FINISHED0 + repeat, FINISHED0)), (ctx, np.flatnonzero(finished != np.where(ran, FINISHED0 + repeat, FINISHED0))[:8])
    assert np.array_equal(taken, np.where(ran, lens, STEPS0)), (ctx, np.flatnonzero(taken != np.where(ran, lens, STEPS0))[:8])
    L, I = lens.astype(np.uint64), np.arange(n, dtype=np.uint64)
    closed_form = ((L * I * np.uint64(31) + L * (L + np.uint64(1)) // np.uint64(2)) % np.uint64(1 << 32)).astype(np.uint32)
    want_acc = np.where(ran, closed_form, np.uint32(ACC0)).astype(np.uint32)
    assert np.array_equal(acc, want_acc), (ctx, np.flatnonzero(acc != want_acc)[:8])


def _walker_sizes(walker):
    ipl = walker[1]
    extra = [s for b in (64 * ipl, 256 * ipl) for s in (b - 1, b + 1)] if walker[0] == CHUNKED else []
    return sorted(set(WALK_SIZES) | set(extra))


def _walk_case(backend, walker, kind):
    for n in _walker_sizes(walker):
        rng = np.random.default_rng(3000 + 101 * WALKERS.index(walker) + 13 * LENS.index(kind) + n)
        _walk(backend, walker, _lens(kind, n, rng))


WALK_CASES = [(w, k) for w in WALKERS for k in LENS]
WALK_IDS = ['%s-%s' % (WALKER_IDS[WALKERS.index(w)], k) for w, k in WALK_CASES]


@pytest.mark.parametrize('case', WALK_CASES, ids=WALK_IDS)
def test_walk_hostsim(hostsim_backend, case):
    _walk_case(hostsim_backend, *case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', WALK_CASES, ids=WALK_IDS)
def test_walk_gpu(gpu_backend, case):
    _walk_case(gpu_backend, *case)


def _walk_many_items_case(backend, walker, n):
    """More items than the launch has lanes (2048 workgroups of the persistent walk, 1536 of the chunked one): every wave refills."""
    _walk(backend, walker, _lens('short', n, np.random.default_rng(n)))


MANY = [((PERSISTENT, 1, 1, 1), 600001), ((CHUNKED, 1, 8, 8), 400003)]


@pytest.mark.parametrize('case', MANY, ids=['persistent', 'chunked'])
def test_walk_more_items_than_lanes_hostsim(hostsim_backend, case):
    _walk_many_items_case(hostsim_backend, *case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', MANY, ids=['persistent', 'chunked'])
def test_walk_more_items_than_lanes_gpu(gpu_backend, case):
    _walk_many_items_case(gpu_backend, *case)


def _walk_counts_case(backend, walker):
    for n in (65, 257, 1025):
        rng = np.random.default_rng(7000 + n)
        for kind in ('ones', 'mix'):
            lens = _lens(kind, n, rng)
            for count in (0, 1, n - 1, n, n + 5):
                _walk(backend, walker, lens, count=count)


COUNT_WALKERS = WALKERS[:2] + [WALKERS[3], (PLAIN, 1, 1, 1)]
COUNT_WALKER_IDS = [WALKER_IDS[0], WALKER_IDS[1], WALKER_IDS[3], 'plain']


@pytest.mark.parametrize('walker', COUNT_WALKERS, ids=COUNT_WALKER_IDS)
def test_walk_device_counts_hostsim(hostsim_backend, walker):
    _walk_counts_case(hostsim_backend, walker)


@pytest.mark.gpu
@pytest.mark.parametrize('walker', COUNT_WALKERS, ids=COUNT_WALKER_IDS)
def test_walk_device_counts_gpu(gpu_backend, walker):
    _walk_counts_case(gpu_backend, walker)


def _walk_plain_case(backend):
    for n in WALK_SIZES + (1023, 1024, 1025):
        rng = np.random.default_rng(8000 + n)
        for kind in ('alt01', 'mix', 'last_long'):
            _walk(backend, (PLAIN, 1, 1, 1), _lens(kind, n, rng))


def test_walk_plain_launch_hostsim(hostsim_backend):
    _walk_plain_case(hostsim_backend)


@pytest.mark.gpu
def test_walk_plain_launch_gpu(gpu_backend):
    _walk_plain_case(gpu_backend)


def _walk_gate_case(backend):
    for n in (1, 65, 257, 100003):
        lens = _lens('mix', n, np.random.default_rng(8500 + n))
        _walk(backend, WALKERS[0], lens, gate_closed=1)
        _walk(backend, WALKERS[0], lens, gate_closed=1, count=n - 1, repeat=3)
        _walk(backend, WALKERS[0], lens, gate_closed=0)    # the same launch with the gate open walks


def test_walk_gate_closed_hostsim(hostsim_backend):
    _walk_gate_case(hostsim_backend)


@pytest.mark.gpu
def test_walk_gate_closed_gpu(gpu_backend):
    _walk_gate_case(gpu_backend)


def _walk_ring_case(backend, walker):
    """4200 launches back to back: each takes the next counter of the 4096-entry ring, so the last 104 reuse the first ones'."""
    lens = _lens('mix', 65, np.random.default_rng(8800))
    lens[lens == 3000] = 40
    _walk(backend, walker, lens, repeat=4200)
    _walk(backend, walker, lens, repeat=2, count=64)


@pytest.mark.parametrize('walker', WALKERS[:2], ids=WALKER_IDS[:2])
def test_walk_laps_the_counter_ring_hostsim(hostsim_backend, walker):
    _walk_ring_case(hostsim_backend, walker)


@pytest.mark.gpu
@pytest.mark.parametrize('walker', WALKERS[:2], ids=WALKER_IDS[:2])
def test_walk_laps_the_counter_ring_gpu(gpu_backend, walker):
    _walk_ring_case(gpu_backend, walker)


def _walk_refusal_case(backend):
    """Only arguments out of range: nothing is launched."""
    lens = np.ones(100, np.int32)
    for walker in ((3, 1, 1, 1), (-1, 1, 1, 1), (CHUNKED, 0, 8, 8), (CHUNKED, 65, 8, 8), (CHUNKED, -1, 8, 8), (CHUNKED, 1, 0, 8),
                   (CHUNKED, 1, 65, 8), (CHUNKED, 1, 8, 0), (CHUNKED, 1, 8, 1025), (PERSISTENT, 0, 1, 1), (PLAIN, 1, 1, 0)):
        _walk(backend, walker, lens, expect=1)
    for repeat in (0, -1, 65537):
        _walk(backend, WALKERS[1], lens, repeat=repeat, expect=1)
    _walk(backend, WALKERS[1], lens, gate_closed=1, expect=1)           # only the persistent walk has a gate
    _walk(backend, (PLAIN, 1, 1, 1), lens, gate_closed=1, expect=1)
    _walk(backend, WALKERS[0], lens, gate_closed=2, expect=1)
    _walk(backend, WALKERS[0], lens, count=1 << 30, expect=1)
    for bad in (-1, 65537):
        worse = lens.copy()
        worse[99] = bad
        _walk(backend, WALKERS[0], worse, expect=1)
        _walk(backend, WALKERS[0], worse, count=5, expect=1)            # ... also where the count would never reach it
    lib = _lib(backend)
    a = np.zeros(4, np.int32)
    assert lib.rdr_debug_walk(0, -1, -1, _ptr(a), 1, 1, 1, 0, 1, _ptr(a), _ptr(a), _ptr(a), _ptr(a)) == 1
    assert lib.rdr_debug_walk(0, (1 << 24) + 1, -1, _ptr(a), 1, 1, 1, 0, 1, _ptr(a), _ptr(a), _ptr(a), _ptr(a)) == 1
    assert lib.rdr_debug_walk(0, 4, -1, None, 1, 1, 1, 0, 1, _ptr(a), _ptr(a), _ptr(a), _ptr(a)) == 1
    assert lib.rdr_debug_walk(0, 4, -1, _ptr(a), 1, 1, 1, 0, 1, _ptr(a), _ptr(a), _ptr(a), None) == 1
    assert 'rdr_debug_walk' in lib.rdr_last_error().decode() and not a.any()


def test_walk_hook_refuses_out_of_range_hostsim(hostsim_backend):
    _walk_refusal_case(hostsim_backend)


@pytest.mark.gpu
def test_walk_hook_refuses_out_of_range_gpu(gpu_backend):
    _walk_refusal_case(gpu_backend)


# ---- sort -------------------------------------------------------------------------------------------------------------------------------
SORT_SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4097, 100003, 600001)
KEYS = ('uniform', 'byte0', 'byte7', 'equal', 'three', 'ascending', 'descending', 'bytes_00_ff', 'morton')


def _keys(kind, n, rng):
    u64 = np.uint64
    if kind == 'uniform':
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if kind in ('byte0', 'byte7'):                         # one radix pass decides everything, the other seven must keep it
        return u64(0x5A5A5A5A5A5A5A5A) & ~(u64(0xFF) << u64(8 * int(kind[4]))) | (rng.integers(0, 256, n, dtype=np.uint64) << u64(8 * int(kind[4])))
    if kind == 'equal':
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if kind == 'three':
        return np.asarray([0xFFFFFFFFFFFFFFFF, 0, 0x8000000000000000], np.uint64)[rng.integers(0, 3, n)]
    if kind in ('ascending', 'descending'):
        k = np.arange(n, dtype=np.uint64) * u64((1 << 43) + 12345)
        return k if kind == 'ascending' else k[::-1].copy()
    if kind == 'bytes_00_ff':                              # every digit is the first or the last bin of its pass
        bits = rng.integers(0, 2, (n, 8), dtype=np.uint64)
        return (bits * u64(0xFF) << (np.arange(8, dtype=np.uint64) * u64(8))).sum(axis=1, dtype=np.uint64)
    assert kind == 'morton'                                # 30-bit codes in four clusters that share 18 leading bits, ~8 copies each
    clusters = rng.integers(0, 1 << 18, 4, dtype=np.uint64) << u64(12)
    distinct = clusters[rng.integers(0, 4, n // 8 + 1)] | rng.integers(0, 1 << 12, n // 8 + 1, dtype=np.uint64)
    return distinct[rng.integers(0, len(distinct), n)]


def _sort(backend, keys, vals, expect=0):
    lib = _lib(backend)
    keys, vals = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(vals, np.int32)
    n = len(keys)
    keys_out, vals_out = np.full(n + 2, 0xABCD, np.uint64), np.full(n + 2, SENT_OUT, np.int32)      # one guard on either side
    rc = lib.rdr_debug_sort_pairs(_ptr(keys), _ptr(vals), n, keys_out[1:].ctypes.data, vals_out[1:].ctypes.data)
    assert rc == expect, lib.rdr_last_error()
    assert keys_out[0] == keys_out[-1] == 0xABCD and vals_out[0] == vals_out[-1] == SENT_OUT
    if expect:
        return
    order = np.argsort(keys, kind='stable')
    assert np.array_equal(keys_out[1:-1], keys[order]), (n, np.flatnonzero(keys_out[1:-1] != keys[order])[:8])
    assert np.array_equal(vals_out[1:-1], vals[order]), (n, np.flatnonzero(vals_out[1:-1] != vals[order])[:8])


def _sort_case(backend, kind, permuted):
    for n in SORT_SIZES:
        rng = np.random.default_rng(5000 + 17 * KEYS.index(kind) + n)
        keys = _keys(kind, n, rng)
        vals = rng.permutation(n).astype(np.int32) if permuted else np.arange(n, dtype=np.int32)
        _sort(backend, keys, vals)


SORT_CASES = [(k, p) for k in KEYS for p in (False, True)]
SORT_IDS = ['%s-%s' % (k, 'permuted' if p else 'arange') for k, p in SORT_CASES]


@pytest.mark.parametrize('case', SORT_CASES, ids=SORT_IDS)
def test_sort_pairs_hostsim(hostsim_backend, case):
    _sort_case(hostsim_backend, *case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', SORT_CASES, ids=SORT_IDS)
def test_sort_pairs_gpu(gpu_backend, case):
    _sort_case(gpu_backend, *case)


def _sort_refusal_case(backend):
    lib = _lib(backend)
    k, v = np.zeros(4, np.uint64), np.zeros(4, np.int32)
    ko, vo = np.full(4, 9, np.uint64), np.full(4, 9, np.int32)
    for n in (0, -1, (1 << 24) + 1):
        assert lib.rdr_debug_sort_pairs(_ptr(k), _ptr(v), n, _ptr(ko), _ptr(vo)) == 1
        assert 'rdr_debug_sort_pairs' in lib.rdr_last_error().decode()
    assert lib.rdr_debug_sort_pairs(None, _ptr(v), 4, _ptr(ko), _ptr(vo)) == 1
    assert lib.rdr_debug_sort_pairs(_ptr(k), _ptr(v), 4, _ptr(ko), None) == 1
    assert (ko == 9).all() and (vo == 9).all()


def test_sort_hook_refuses_out_of_range_hostsim(hostsim_backend):
    _sort_refusal_case(hostsim_backend)


@pytest.mark.gpu
def test_sort_hook_refuses_out_of_range_gpu(gpu_backend):
    _sort_refusal_case(gpu_backend)


# ---- of this file's own generators ------------------------------------------------------------------------------------------------------
def test_patterns_are_what_they_claim():
    """What the cases rely on, so that none of them can become vacuous without this test noticing."""
    for n in (4096, 262145):
        rng = np.random.default_rng(n)
        keep = {k: _keep(k, n, rng) for k in KEEPS}
        per_wave = {k: np.add.reduceat(v.astype(int), np.arange(0, n, 64)) for k, v in keep.items()}
        assert keep['none'].sum() == 0 and keep['all'].sum() == n
        assert 0.45 < keep['half'].mean() < 0.55 and 0.01 < keep['sparse'].mean() < 0.03
        assert keep['last'].sum() == 1 and keep['last'][n - 1] and keep['first'].sum() == 1 and keep['first'][0]
        full = np.minimum(64, n - np.arange(0, n, 64))
        assert (per_wave['waves'] == 0).sum() >= n // 128 - 1 and (per_wave['waves'] == full).sum() >= n // 128
        assert (per_wave['sparse'] == 0).any() and (per_wave['sparse'] > 0).any()       # empty waves among busy ones
        assert ((per_wave['half'] > 0) & (per_wave['half'] < 64))[:n // 64].all()       # every whole wave partly kept
    for n in (257, 100003):
        rng = np.random.default_rng(n)
        lens = {k: _lens(k, n, rng) for k in LENS + ('short',)}
        assert (lens['ones'] == 1).all() and (lens['zeros'] == 0).all() and lens['alt01'][:4].tolist() == [0, 1, 0, 1]
        assert lens['long_per_64'].max() == 2000 and (lens['long_per_64'] == 2000).sum() == (n + 63) // 64
        assert (lens['long_per_64'][lens['long_per_64'] != 2000] == 1).all()
        assert lens['last_long'][n - 1] == 4000 and (lens['last_long'][:n - 1] == 1).all()
        assert lens['short'].min() == 0 and lens['short'].max() == 3
        assert max(v.max() for v in lens.values()) == 4000                              # the longest walk of any case
        mix = lens['mix']
        assert mix.max() == 3000 and (mix == 0).any()
        if n > 1000:
            assert 0.08 < (mix == 0).mean() < 0.12 and 0.007 < (mix == 3000).mean() < 0.013
            ordinary = mix[(mix > 0) & (mix < 3000)]
            assert 19 < ordinary.mean() < 21 and ordinary.max() > 100
    assert (_lens('mix', 65, np.random.default_rng(8800)) == 0).any()                   # the ring-lap case has both kinds of item
    n = 100003
    distinct = {k: len(np.unique(_keys(k, n, np.random.default_rng(1)))) for k in KEYS}
    assert distinct['uniform'] == n and distinct['ascending'] == n and distinct['descending'] == n
    assert distinct['byte0'] == 256 and distinct['byte7'] == 256 and distinct['bytes_00_ff'] == 256
    assert distinct['equal'] == 1 and distinct['three'] == 3
    assert n // 12 < distinct['morton'] <= n // 8 + 1
    morton = _keys('morton', n, np.random.default_rng(1))
    assert morton.max() < (1 << 30) and len(np.unique(morton >> np.uint64(12))) <= 4
    for k in ('byte0', 'byte7'):
        keys = _keys(k, n, np.random.default_rng(1))
        assert len(np.unique(keys & ~(np.uint64(0xFF) << np.uint64(8 * int(k[4]))))) == 1
    asc = _keys('ascending', n, np.random.default_rng(1))
    assert (asc[1:] > asc[:-1]).all() and np.array_equal(_keys('descending', n, np.random.default_rng(1)), asc[::-1])
    # the sizes straddle what the kernels switch on
    assert {1023, 1024, 1025, 262144, 262145} <= set(COMPACT_SIZES) and {2047, 2048, 2049} <= set(SORT_SIZES)
    assert {255, 257, 1023, 1025} <= set(_walker_sizes((CHUNKED, 4, 32, 3))) and set(WALK_SIZES) == set(_walker_sizes(WALKERS[0]))
    assert {4095, 4097, 16383, 16385} <= set(_walker_sizes((CHUNKED, 64, 64, 1)))
    assert 600001 > 2048 * 256 and 400003 > 1536 * 256
