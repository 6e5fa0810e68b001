#!/usr/bin/env python3
"""Generate the pose fixtures under tests/golden/ (run in the BUILD container only).

The expected values come from the REFERENCE's own `pyredner.gen_rotate_matrix` and the expression its pose-estimation scripts
write (make_deferred_golden.reference_package()), evaluated by torch in fp32 on the CPU:

    R = pyredner.gen_rotate_matrix(angles)
    center = torch.mean(torch.cat(sets), 0)                 (or the given centre)
    out_k = (v_k - center) @ torch.t(R) + center + translation
    loss = sum_k (out_k * upstream_k).sum();  loss.backward()

  pose_<case>.npz     <pose>_R, <pose>_out<k>, <pose>_d_angles, <pose>_d_translation, <pose>_d_center (a given centre only),
                      <pose>_d_vertices<k>, with <pose> = a<i>_own | a<i>_given, i into ANGLES;
                      inputs_sum: checksum of the regenerated inputs (vertex sets and upstream gradients)
                      harness_sha256: digest() of what the CPU debugging harness computes for every pose of the case: the bits
                      both GPU builds have to reproduce

The vertex sets are those of make_mesh_golden.mesh() (6, 8, 56, 63, 98, 301, 488 and 2624 vertices), regenerated and checksummed,
not stored; the upstream gradients are seeded normal numbers, regenerated the same way.  Every case runs every angle triple of
ANGLES under the sets' own centre and under CENTER.

  pose_switches.npz   for the set sizes on both sides of every switch of the launch plan (switch_sizes(): random sets, no
                      reference values; tests/test_pose.py holds them to its fp64 definition): sizes_<i> and harness_sha256_<i>,
                      the harness's bits at sizes where a workgroup owns more than one chunk

Checked here: every fp32 tensor of the reference lies within 5e-6 relative L2 (a twentieth of the tests' bar) of an fp64
evaluation of the closed form of csrc/pose.h (measured: d_center 2.6e-6, d_angles 1.1e-6, the other tensors at most 1.5e-7); a
tensor that is exactly zero in fp64 (d_angles of the single vertex about itself) is exactly zero in the reference.  If a seed
trips an assertion, change the seed, not the bar.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]
import make_mesh_golden as mg              # noqa: E402

ANGLES = ((-0.2, 0.1, -0.1), (0.1, -0.1, 0.1), (2.9, -1.4, 0.7), (0.0, 0.0, 0.0))
TRANSLATION = (0.1, 0.4, 0.1)
CENTER = (0.3, -0.2, 0.5)
# case -> the meshes whose vertices are its sets; 'vertex' is one vertex cut from box4
CASES = {
    'fan5': ('fan5',), 'degenerate': ('degenerate',), 'sphere6x8': ('sphere6x8',), 'grid7x9': ('grid7x9',), 'box4': ('box4',),
    'fan300': ('fan300',), 'box9': ('box9',), 'sphere40x64': ('sphere40x64',),
    'box4_sphere6x8': ('box4', 'sphere6x8'), 'sphere40x64_fan5_grid7x9': ('sphere40x64', 'fan5', 'grid7x9'),
    'vertex': ('vertex',),
}
UPSTREAM_SEED = 7100


def fixture_path(case):
    return os.path.join(HERE, 'pose_%s.npz' % case)


def sets_of(case):
    """The vertex sets of a case as contiguous CPU fp32 tensors."""
    out = []
    for name in CASES[case]:
        out.append(mg.mesh('box4')[0][17:18].clone() if name == 'vertex' else mg.mesh(name)[0].float().contiguous())
    return out


def upstream_of(case):
    """One seeded normal tensor per set."""
    gen = torch.Generator().manual_seed(UPSTREAM_SEED + sorted(CASES).index(case))
    return [torch.randn(v.shape[0], 3, generator=gen) for v in sets_of(case)]


def inputs_sum(case):
    return sum(mg.checksum(t) for t in sets_of(case) + upstream_of(case))


def poses(case=None):
    """[(key, angles, own centre?)]: every angle triple under the sets' own centre and under CENTER, the same for every case"""
    return [('a%d_%s' % (i, 'own' if own else 'given'), ANGLES[i], own) for i in range(len(ANGLES)) for own in (True, False)]


def closed_form(angles):
    """R of csrc/pose.h's header from a [3] tensor, in its dtype (differentiable)"""
    st, ct, sp, cp, ss, cs = angles[0].sin(), angles[0].cos(), angles[1].sin(), angles[1].cos(), angles[2].sin(), angles[2].cos()
    return torch.stack([torch.stack([cs * cp, cs * sp * st - ss * ct, -cs * sp * ct - ss * st]),
                        torch.stack([ss * cp, ss * sp * st + cs * ct, -ss * sp * ct + cs * st]),
                        torch.stack([sp, -cp * st, cp * ct])])


def evaluate(rotate, sets, upstream, angles, own, dtype):
    """The scripts' expression and its gradients by torch autograd on the CPU in `dtype`, R from `rotate(angles)`.
    -> {'R', 'out<k>', 'd_angles', 'd_translation', 'd_center' (given), 'd_vertices<k>'} as numpy arrays"""
    a = torch.tensor(angles, dtype=dtype, requires_grad=True)
    t = torch.tensor(TRANSLATION, dtype=dtype, requires_grad=True)
    vs = [v.to(dtype).clone().requires_grad_(True) for v in sets]
    given = None if own else torch.tensor(CENTER, dtype=dtype, requires_grad=True)
    R = rotate(a)
    center = torch.mean(torch.cat(vs), 0) if own else given
    outs = [(v - center) @ torch.t(R) + center + t for v in vs]
    sum((o * u.to(dtype)).sum() for o, u in zip(outs, upstream)).backward()
    res = {'R': R.detach().numpy(), 'd_angles': a.grad.numpy(), 'd_translation': t.grad.numpy()}
    if not own:
        res['d_center'] = given.grad.numpy()
    for k, (o, v) in enumerate(zip(outs, vs)):
        res['out%d' % k] = o.detach().numpy()
        res['d_vertices%d' % k] = v.grad.numpy()
    return res


def run_native(backend, device, sets, upstream, angles, own, translation=TRANSLATION, center=CENTER):
    """The same quantities as evaluate() by redner_amd.pose_vertices on `backend` (the library tests/conftest.py loaded), every
    tensor moved to `device`; also checks shape, dtype and device of every output."""
    from redner_amd import pose_vertices
    a = torch.tensor(angles, dtype=torch.float32, device=device, requires_grad=True)
    t = torch.tensor(translation, dtype=torch.float32, device=device, requires_grad=True)
    vs = [v.detach().clone().to(device).requires_grad_(True) for v in sets]
    given = None if own else torch.tensor(center, dtype=torch.float32, device=device, requires_grad=True)
    outs = pose_vertices(vs, a, t, center=given, backend=backend)
    assert isinstance(outs, list) and len(outs) == len(vs)
    for o, v in zip(outs, vs):
        assert o.shape == v.shape and o.dtype == torch.float32 and o.device == v.device and o.is_contiguous()
    sum((o * u.to(device)).sum() for o, u in zip(outs, upstream)).backward()
    res = {'R': constants(outs)[0].cpu().numpy(), 'd_angles': a.grad.cpu().numpy(),
           'd_translation': t.grad.cpu().numpy()}
    if not own:
        res['d_center'] = given.grad.cpu().numpy()
    for k, (o, v) in enumerate(zip(outs, vs)):
        assert v.grad.shape == v.shape and v.grad.dtype == torch.float32 and v.grad.device == v.device
        res['out%d' % k] = o.detach().cpu().numpy()
        res['d_vertices%d' % k] = v.grad.cpu().numpy()
    return res


def constants(outs):
    """(R [3, 3], centre [3]) as the forward call that made `outs` formed and used them: what PoseVertices keeps for its backward
    call (needs an input that requires a gradient, so that the outputs have a node)"""
    saved = (outs[0] if isinstance(outs, (list, tuple)) else outs).grad_fn.saved
    return saved[:9].reshape(3, 3).clone(), saved[9:].clone()


# ---- the launch plan's switches -------------------------------------------------------------------------------------------------
SWITCH_PATH = os.path.join(HERE, 'pose_switches.npz')
SWITCH_POSES = (('a2_own', ANGLES[2], True), ('a0_given', ANGLES[0], False))


def switch_sizes(backend):
    """Set sizes on both sides of every switch of the launch plan, found through the plan query"""
    chunk, most, groups = backend.pose_plan([1])
    assert chunk >= 2 and most >= 2 and groups == 1
    assert backend.pose_plan([chunk])[2] == 1 and backend.pose_plan([chunk + 1])[2] == 2
    assert backend.pose_plan([chunk * most])[2] == most and backend.pose_plan([chunk * most + 1])[2] == most
    assert backend.pose_plan([chunk, 1, chunk + 1])[2] == 4                     # chunks do not span sets
    return [[1], [chunk - 1], [chunk], [chunk + 1], [2 * chunk + 77],           # one vertex; around a chunk; a partial last chunk
            [chunk * most], [chunk * most + 1],                                 # the first size at which a workgroup owns two chunks
            [chunk + 1, 5, 2 * chunk, 1],                                       # unequal sets in one call
            [chunk * most + 3, 2 * chunk + 1, 7]]                               # ... of which a workgroup owns chunks of two sets


def switch_inputs(i, sizes):
    """(sets, upstream gradients) of entry i of switch_sizes(): seeded normal numbers, the sets off the origin"""
    gen = torch.Generator().manual_seed(900 + i)
    sets = [torch.randn(n, 3, generator=gen) + torch.tensor([0.5, -1.0, 2.0]) for n in sizes]
    return sets, [torch.randn(n, 3, generator=gen) for n in sizes]


def run_switch(backend, device, i, sizes):
    """{pose key: run_native()} of entry i of switch_sizes()"""
    sets, ups = switch_inputs(i, sizes)
    return {key: run_native(backend, device, sets, ups, angles, own) for key, angles, own in SWITCH_POSES}


def digest(results):
    """SHA-256 of the bits of every tensor of {pose key: run_native()} in sorted (pose, tensor) order, as 32 uint8"""
    import hashlib
    h = hashlib.sha256()
    for key in sorted(results):
        for name in sorted(results[key]):
            h.update(np.ascontiguousarray(results[key][name]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def harness_backend():
    """The CPU debugging harness (tests/hostsim), built and loaded: its bits are recorded in the fixtures"""
    import subprocess
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path[:0] = [p for p in (root,) if p not in sys.path]
    subprocess.check_call(['make', '-C', os.path.join(root, 'tests', 'hostsim'), '-j8'], stdout=subprocess.DEVNULL)
    from redner_amd import _capi, redner
    _capi.load(os.path.join(root, 'tests', 'hostsim', '_build', 'libredner_hostsim.so'))
    return redner


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def main():
    import make_deferred_golden as mk
    _, pyredner = mk.reference_package()
    harness = harness_backend()
    worst = {}
    for case in CASES:
        sets, ups = sets_of(case), upstream_of(case)
        out = {'inputs_sum': np.asarray(inputs_sum(case))}
        for key, angles, own in poses(case):
            ref = evaluate(pyredner.gen_rotate_matrix, sets, ups, angles, own, torch.float32)
            want = evaluate(closed_form, sets, ups, angles, own, torch.float64)
            for name, value in ref.items():
                assert value.dtype == np.float32 and np.isfinite(value).all(), (case, key, name)
                norm = float(np.linalg.norm(want[name]))
                if norm == 0.0:
                    assert not value.any(), (case, key, name, 'zero in fp64, not in the reference')
                else:
                    distance = float(np.linalg.norm(value.astype(np.float64) - want[name]) / norm)
                    kind = name.rstrip('0123456789')
                    worst[kind] = max(worst.get(kind, 0.0), distance)
                    assert distance < 5e-6, (case, key, name, distance)
                out['%s_%s' % (key, name)] = value
        if case == 'vertex':
            assert not any(out['%s_d_angles' % key].any() for key, _, own in poses(case) if own)
        out['harness_sha256'] = digest({key: run_native(harness, torch.device('cpu'), sets, ups, angles, own)
                                        for key, angles, own in poses(case)})
        np.savez_compressed(fixture_path(case), **out)
        print('%-28s %d poses, %d bytes' % (case, len(poses(case)), os.path.getsize(fixture_path(case))))
    switches = {}
    for i, sizes in enumerate(switch_sizes(harness)):
        switches['sizes_%d' % i] = np.asarray(sizes, dtype=np.int64)
        switches['harness_sha256_%d' % i] = digest(run_switch(harness, torch.device('cpu'), i, sizes))
    np.savez_compressed(SWITCH_PATH, **switches)
    print('largest fp32-reference vs fp64 distances:', ', '.join('%s %.2e' % kv for kv in sorted(worst.items())))


if __name__ == '__main__':
    main()
