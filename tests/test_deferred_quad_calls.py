"""deferred_quad under the ways a training loop calls it: conditions A to I of tests/test_native_op_calls.py (that module's
docstring states them) on one case of tests/test_deferred_quad.py -- two images, the three quads, per-image ranges, aa 2, alpha.

The case object is that module's `Case`, and conditions A (views), B (upstream gradients), C (gradient subsets), D (retain_graph),
E (edits in place), F (the quad table on the host), G (a side stream) and I (create_graph) are its own runners, imported.  H (two
host threads) is restated here: that module's runner looks into the word outputs of its own shadowed case.  The plain call is
held to the fp64 definition under parity_util.TOL, every condition to the plain call with torch.equal."""
import threading

import pytest
import torch

import test_deferred_quad as t_quad
import test_native_op_calls as calls
from golden import make_deferred_golden as mk

CPU, GPU = calls.CPU, calls.GPU
LETTERS = 'ABCDEFGHI'
NAME = 'grid_5x7_aa2_alpha1'


def _quad_case(seed=None):
    """DeferredQuad on a case of test_deferred_quad.  `seed`, condition H: the same shapes from the generator at another seed (no
    texel is taken off the kink: such a case is held to its own plain bits only)."""
    if seed is None:
        base = t_quad._definition_case(NAME)
    else:
        n, h, w, aa, alpha, which, ranges = t_quad._shape_of(NAME)
        rows, flags = t_quad.three_quads(seed + 5000)
        base = dict(g=t_quad.generate(seed, n, h, w, aa, alpha), quads=rows, flags=flags, ranges=ranges, aa=aa, alpha=alpha)
    n, hg, wg = base['g'].shape[:3]
    inputs = {'g_buffer': base['g'].clone(), 'quads': torch.from_numpy(base['quads']).clone()}
    up = mk.upstream((n, hg // base['aa'], wg // base['aa'], 3))

    def call(rd, t):
        return [calls._modules()[1].DeferredQuad.apply(t['g_buffer'], t['quads'], tuple(base['flags']), tuple(base['ranges']), base['aa'],
                                                       bool(base['alpha']), rd)], []

    def definition(case, plain, backend, device):
        assert seed is None and torch.equal(base['up'], up)
        out = {'image': plain['outs'][0], 'd_g_buffer': plain['grads']['g_buffer'], 'd_quads': plain['grads']['quads']}
        t_quad._assert_parity(out, base['want'], str(case))

    label = 'quad_%dx%d_aa%d_alpha%d' % (hg // base['aa'], wg // base['aa'], base['aa'], base['alpha'])
    return calls.Case('deferred_quad', label + ('' if seed is None else '_%d' % seed), inputs, call, definition, diff=('g_buffer', 'quads'),
                      cotangents=[up], reads=tuple(inputs), subsets=(('g_buffer',), ('quads',)), small=('quads',))


_BUILT = {}


def _case():
    if 'case' not in _BUILT:
        _BUILT['case'] = _quad_case()
    return _BUILT['case']


def test_the_case_takes_every_condition():
    """what test_native_op_calls.test_table_is_complete holds its own cases to"""
    import redner_amd
    case = _case()
    assert callable(redner_amd.deferred_quad) and case.op == 'deferred_quad' and case.diff and case.small
    assert set(LETTERS) == set(calls.CONDITIONS) | {'H'} and set(calls.HARNESS_CONDITIONS) | set('FGH') == set(LETTERS)
    assert set(case.small) <= set(case.diff) and not case.saved_extras
    assert set(case.reads) | set(case.unread) == set(case.inputs) and not set(case.reads) & set(case.unread)


def test_plain_is_the_definition_hostsim(hostsim_backend):
    case = _case()
    case.definition(case, calls._plain(case, hostsim_backend, CPU), hostsim_backend, CPU)


@pytest.mark.gpu
def test_plain_is_the_definition_gpu(gpu_backend):
    case = _case()
    case.definition(case, calls._plain(case, gpu_backend, GPU), gpu_backend, GPU)


@pytest.mark.parametrize('letter', [l for l in LETTERS if l in calls.HARNESS_CONDITIONS])
def test_calls_hostsim(hostsim_backend, letter):
    calls.CONDITIONS[letter](_case(), hostsim_backend, CPU)


@pytest.mark.gpu
@pytest.mark.parametrize('letter', [l for l in LETTERS if l in calls.GPU_CONDITIONS])
def test_calls_gpu(gpu_backend, letter):
    calls.CONDITIONS[letter](_case(), gpu_backend, GPU)


@pytest.mark.gpu
def test_two_host_threads_gpu(gpu_backend):
    """H: rdr_set_stream is state of the calling host thread.  Two Python threads, each under its own side stream, started
    together, each run deferred_quad forward and backward ten times on their own inputs and get the plain bits of those inputs
    every time.  (One process, two threads; as in test_native_op_calls, this covers the forward launches: autograd runs the
    backward node on its one worker thread of the device.)"""
    work = [_quad_case(3100 + 10 * k) for k in range(2)]
    plains = [calls._plain(case, gpu_backend, GPU) for case in work]
    assert not torch.equal(plains[0]['outs'][0], plains[1]['outs'][0])
    staged = [({n: x.clone().to(GPU) for n, x in case.inputs.items()}, calls._cotangents(case, GPU)) for case in work]
    torch.cuda.synchronize(GPU)
    start, failures = threading.Barrier(2), []

    def worker(k):
        try:
            side = torch.cuda.Stream(device=GPU)
            with torch.cuda.stream(side):
                start.wait(timeout=20)
                inputs, weights = staged[k]
                for it in range(10):
                    place = {n: (lambda x, d, n=n: inputs[n].clone()) for n in work[k].inputs}
                    got = calls._run(work[k], gpu_backend, GPU, place=place, cotangents=[w.clone() for w in weights])
                    calls._same(got, plains[k], 'thread %d, pass %d' % (k, it))
                side.synchronize()
        except BaseException as error:                                          # (reported by the main thread)
            failures.append((k, error))
            start.abort()

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
