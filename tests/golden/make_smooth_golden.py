#!/usr/bin/env python3
"""Generate the smoothing fixtures under tests/golden/ (run in the BUILD container only).

The expected values come from the REFERENCE's own `pyredner.smooth` and `pyredner.bound_vertices` executed by torch on the CPU
(make_deferred_golden.reference_package()); the meshes are those of make_mesh_golden.py.

  smooth_<mesh>.npz   bound                      the reference's bound_vertices
                      shift_<scheme>_<control>   after - before of smooth(lmd = 1): the displacement, the fp64 difference of the
                                                 two fp32 tensors; scheme in SCHEMES, control in 'default' (None: the boundary
                                                 mask) and 'ones'
                      half_<scheme>_<control>    the same at lmd = 0.5
                      vertices_sum, indices_sum  make_mesh_golden.checksum() of the input

Checked here, for every mesh but the hand-made degenerate one: every displacement is finite; no |W| is below 1 (measured: 1.76
at least), so no quotient is decided by rounding; the reference's fp32 displacement lies within 5e-6 relative L2 (a twentieth
of the tests' bar; measured 4e-8 ... 4.3e-6, the largest on fan300 under 'cotangent') of an fp64 evaluation with index_add sums
and cot = e1 . e2 / |e1 x e2|; the number of interior vertices is INTERIOR[mesh].  On the degenerate mesh: `bound` is
DEGENERATE_BOUND and the reference is finite exactly on the rows DEGENERATE_FINITE[scheme].  If a seed trips an assertion,
change the seed, not the bar.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]
import make_deferred_golden as mk          # noqa: E402
import make_mesh_golden as mg              # noqa: E402

SCHEMES = ('reciprocal', 'uniform', 'cotangent')
CONTROLS = ('default', 'ones')
INTERIOR = {'box4': 98, 'box9': 488, 'sphere6x8': 40, 'sphere40x64': 2496, 'grid7x9': 35, 'fan300': 1, 'fan5': 1}
DEGENERATE_BOUND = [0, 0, 0, 0, 1, 0, 1, 1]
DEGENERATE_FINITE = {'reciprocal': [0, 1, 2, 3, 5, 7], 'uniform': [0, 1, 2, 3, 5, 7], 'cotangent': [2, 3]}


def finite_rows(displacement):
    return [i for i, ok in enumerate(np.isfinite(displacement).all(axis=1)) if ok]


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def sums_fp64(vertices, indices, scheme):
    """(C [V, 3], W [V]) in fp64 on a mesh without degenerate corners"""
    v, idx = vertices.double(), indices.long()
    C, W = torch.zeros_like(v), torch.zeros(len(v), dtype=torch.float64)
    for i in range(3):
        p0, p1, p2 = v[idx[:, i]], v[idx[:, (i + 1) % 3]], v[idx[:, (i + 2) % 3]]
        e1, e2 = p1 - p0, p2 - p0
        l1, l2 = e1.norm(dim=1), e2.norm(dim=1)
        if scheme == 'reciprocal':
            C.index_add_(0, idx[:, i], e1 / l1[:, None] + e2 / l2[:, None])
            W.index_add_(0, idx[:, i], 1.0 / l1 + 1.0 / l2)
        elif scheme == 'uniform':
            C.index_add_(0, idx[:, i], e1 + e2)
            W.index_add_(0, idx[:, i], torch.full_like(l1, 2.0))
        else:
            cot = (e1 * e2).sum(1) / torch.linalg.cross(e1, e2, dim=1).norm(dim=1)
            w = (p2 - p1) * cot[:, None]
            C.index_add_(0, idx[:, (i + 1) % 3], w)
            C.index_add_(0, idx[:, (i + 2) % 3], -w)
            W.index_add_(0, idx[:, (i + 1) % 3], cot)
            W.index_add_(0, idx[:, (i + 2) % 3], cot)
    return C, W


def displacement(pyredner, vertices, indices, lmd, scheme, control):
    after = vertices.clone()
    pyredner.smooth(after, indices, lmd, scheme, control)
    return (after.double() - vertices.double()).numpy()


def main():
    _, pyredner = mk.reference_package()
    min_w, worst = float('inf'), (0.0, None)
    for name in mg.MESHES:
        vertices, indices = mg.mesh(name)
        bound = pyredner.bound_vertices(vertices, indices)
        out = {'vertices_sum': np.asarray(mg.checksum(vertices)), 'indices_sum': np.asarray(mg.checksum(indices)),
               'bound': bound.numpy()}
        if name == 'degenerate':
            assert bound.tolist() == DEGENERATE_BOUND, bound.tolist()
        else:
            assert int(bound.sum()) == INTERIOR[name], (name, int(bound.sum()))
        for scheme in SCHEMES:
            for ctl in CONTROLS:
                control = None if ctl == 'default' else torch.ones(len(vertices))
                key = '%s_%s' % (scheme, ctl)
                out['shift_' + key] = displacement(pyredner, vertices, indices, 1.0, scheme, control)
                out['half_' + key] = displacement(pyredner, vertices, indices, 0.5, scheme, control)
                if name == 'degenerate':
                    for k in ('shift_', 'half_'):
                        assert finite_rows(out[k + key]) == DEGENERATE_FINITE[scheme], (scheme, ctl, finite_rows(out[k + key]))
                    continue
                assert np.isfinite(out['shift_' + key]).all() and np.isfinite(out['half_' + key]).all(), (name, key)
                C, W = sums_fp64(vertices, indices, scheme)
                min_w = min(min_w, float(W.abs().min()))
                want = (C / W[:, None] * (bound.double() if control is None else control.double())[:, None]).numpy()
                distance = float(np.linalg.norm(out['shift_' + key] - want) / np.linalg.norm(want))
                worst = max(worst, (distance, name + ' ' + key))
                assert distance < 5e-6, (name, key, distance)
                print('%-12s %-18s fp32 reference vs fp64: %.2e' % (name, key, distance))
        np.savez_compressed(os.path.join(HERE, 'smooth_%s.npz' % name), **out)
    assert min_w >= 1.0, min_w
    print('min |W| = %.3g; largest fp32-vs-fp64 distance %.2e (%s)' % (min_w, worst[0], worst[1]))


if __name__ == '__main__':
    main()
