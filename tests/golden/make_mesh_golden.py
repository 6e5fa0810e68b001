#!/usr/bin/env python3
"""Generate the vertex-normal fixtures under tests/golden/ (run in the BUILD container only).

The expected values come from the REFERENCE's own `pyredner.compute_vertex_normal` executed by torch on the CPU (gradients from
torch autograd); nothing here restates its formula.  Needs the reference checkout (its unmodified Python package, imported on
top of the oracle build of its `redner` module: make_deferred_golden.reference_package()) and, for the end-to-end case, the
oracle build itself (oracle/_ref).

  vertex_normal_<mesh>.npz   for a seeded mesh (MESHES) and every scheme it is checked under: normals_<scheme>, and
                             d_vertices_<scheme> under loss = sum(normals * upstream(V, 0)).  `vertices_sum` and
                             `indices_sum` (checksum(): position-weighted, fp64) guard the regenerated input.  The hand-made degenerate mesh has normals only: the
                             reference's gradient is NaN there.
  vertex_normal_e2e.npz      e2e_scene(): a smooth closed mesh whose normals are compute_vertex_normal(vertices, indices), lit
                             by an area light, 32 x 32 x 4 samples, max_bounces 1, Sobol: image and d(vertices), which holds the
                             geometric part and the part through the normals; the same two checksums of its mesh.

Every cotangent fixture is checked here, in fp64 and for EVERY vertex (no exclusions): the length of the cotangent sum stays
0.02 away from the 0.05 threshold of the fallback; where the sum is kept, its angle to the 'max' normal stays away from 90
degrees (|n_cot . n_max| > 1e-3 |n_cot|: the flip is not decided by rounding); no fp32 length is exactly 0 and the reference's
gradients are finite.  An open boundary fails the second condition (the cotangent vector lies in the surface there), which is
why the open meshes are 'max' only.  If a seed trips an assertion, change the seed, not the bar.

The helpers at the top (meshes, upstream gradients, the scene) are also what tests/test_vertex_normal.py builds its inputs from;
they need neither the reference nor the oracle.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (HERE,) if p not in sys.path]
import make_deferred_golden as mk          # noqa: E402

E2E_SAMPLES, E2E_BOUNCES, E2E_SEED, E2E_RESOLUTION = (4, 4), 1, 13, (32, 32)          # 4 samples per pixel each way


# ---- meshes: (vertices [V, 3] float32, indices [T, 3] int32), numpy -----------------------------------------------------------
def box(divisions, seed):
    """A closed box, `divisions` x `divisions` quads per side, cut at sorted random places per axis, scaled 1 / 0.7 / 1.3.
    V = 6 n^2 + 2, T = 12 n^2.  The (n - 1)^2 inner vertices of every side are planar."""
    n = divisions
    rng = np.random.RandomState(seed)
    cuts = [np.concatenate([[-1.0], np.sort(rng.uniform(-0.8, 0.8, n - 1)), [1.0]]) * s for s in (1.0, 0.7, 1.3)]
    ids, verts = {}, []

    def vid(i, j, k):
        if (i, j, k) not in ids:
            ids[(i, j, k)] = len(verts)
            verts.append([cuts[0][i], cuts[1][j], cuts[2][k]])
        return ids[(i, j, k)]

    tris = []
    for axis in range(3):
        for side in (0, n):
            for a in range(n):
                for b in range(n):
                    def at(da, db):
                        c = [0, 0, 0]
                        c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = side, a + da, b + db
                        return vid(*c)
                    q = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]              # counter-clockwise seen from + axis
                    if side == 0:
                        q = q[::-1]
                    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32)


def uv_sphere(rows, cols, seed, jitter=0.15):
    """rows + 1 rings of cols vertices between the colatitudes pi (i + 0.5) / (rows + 1), every vertex moved by up to `jitter` of
    its ring spacing: a sphere with a small opening at either pole.  V = (rows + 1) cols, T = 2 rows cols."""
    rng = np.random.RandomState(seed)
    verts = []
    for i in range(rows + 1):
        for j in range(cols):
            th = np.pi * (i + 0.5 + jitter * rng.uniform(-1, 1)) / (rows + 1)
            ph = 2 * np.pi * (j + jitter * rng.uniform(-1, 1)) / cols
            r = 1.0 + 0.3 * jitter * rng.uniform(-1, 1)
            verts.append([r * np.sin(th) * np.cos(ph), r * np.cos(th), r * np.sin(th) * np.sin(ph)])
    tris = []
    for i in range(rows):
        for j in range(cols):
            a, b = i * cols + j, i * cols + (j + 1) % cols
            c, d = a + cols, b + cols
            tris += [[a, b, c], [b, d, c]]
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32)


def grid(rows, cols, seed):
    """An open rows x cols grid of vertices over the plane, jittered in all three directions.  T = 2 (rows - 1)(cols - 1)."""
    rng = np.random.RandomState(seed)
    verts = [[j + 0.25 * rng.uniform(-1, 1), i + 0.25 * rng.uniform(-1, 1), 0.4 * rng.uniform(-1, 1)]
             for i in range(rows) for j in range(cols)]
    tris = []
    for i in range(rows - 1):
        for j in range(cols - 1):
            a, b, c, d = i * cols + j, i * cols + j + 1, (i + 1) * cols + j, (i + 1) * cols + j + 1
            tris += [[a, b, c], [b, d, c]]
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32)


def fan(spokes, seed):
    """`spokes` triangles around one hub (vertex 0), closed: the hub's row has `spokes` corners.  V = spokes + 1."""
    rng = np.random.RandomState(seed)
    verts = [[0.02 * rng.uniform(-1, 1), 0.02 * rng.uniform(-1, 1), 0.5]]
    for j in range(spokes):
        ph, r = 2 * np.pi * (j + 0.2 * rng.uniform(-1, 1)) / spokes, 1.0 + 0.2 * rng.uniform(-1, 1)
        verts.append([r * np.cos(ph), r * np.sin(ph), 0.1 * rng.uniform(-1, 1)])
    tris = [[0, 1 + j, 1 + (j + 1) % spokes] for j in range(spokes)]
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32)


# vertex 4 is isolated; face 1 repeats face 0; face 3 has no area (0, 1, 5 lie on one line, exactly also in fp32: vertex 5
# belongs to it alone); face 4 lists vertex 6 twice (6 and 7 belong to it alone)
DEGENERATE_VERTICES = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [5, 5, 5], [2, 0, 0], [3, 1, 2], [-1, 2, 1]]
DEGENERATE_FACES = [[0, 1, 2], [0, 1, 2], [1, 3, 2], [0, 1, 5], [6, 6, 7]]
DEGENERATE_DEFAULT_NORMAL = [4, 5, 6, 7]            # vertices that take (0, 0, 1) and a zero gradient


def degenerate(_seed=None):
    return np.asarray(DEGENERATE_VERTICES, np.float32), np.asarray(DEGENERATE_FACES, np.int32)


# name -> (generator, arguments, schemes, has a reference gradient).  'cotangent' is left out where its conditions (module
# docstring) cannot hold: the open meshes, the degenerate mesh (the reference's cotangent sum is NaN there; collapsed_box() below
# covers the rule against the fp64 definition), and sphere40x64, where 363 of the 2624 cotangent sums (about 4 x the vertex area on a
# unit sphere) lie within 0.02 of the 0.05 threshold.  box9 is the many-workgroup cotangent case.
MESHES = {
    'box4': (box, (4, 11), ('max', 'cotangent'), True),
    'box9': (box, (9, 12), ('max', 'cotangent'), True),
    'sphere6x8': (uv_sphere, (6, 8, 21), ('max', 'cotangent'), True),
    'sphere40x64': (uv_sphere, (40, 64, 22), ('max',), True),
    'grid7x9': (grid, (7, 9, 31), ('max',), True),
    'fan300': (fan, (300, 41), ('max',), True),
    'fan5': (fan, (5, 42), ('max',), True),
    'degenerate': (degenerate, (), ('max',), False),
}
SIZES = {'box4': (98, 192), 'box9': (488, 972), 'sphere6x8': (56, 96), 'sphere40x64': (2624, 5120), 'grid7x9': (63, 96),
         'fan300': (301, 300), 'fan5': (6, 5), 'degenerate': (8, 5)}


# vertices that take the 'max' fallback under 'cotangent' (the planar inner vertices of a box's sides), asserted by the tests: both
# branches of the choice stay covered whatever the seeds
COTANGENT_FALLBACKS = {'box4': 54, 'box9': 384, 'sphere6x8': 0}


def checksum(t):
    """A sum that moves when elements move: element i weighs i + 1 (fp64)."""
    flat = t.double().reshape(-1)
    return float((flat * torch.arange(1, flat.numel() + 1, dtype=torch.float64)).sum())


def collapsed_box():
    """box4 with one edge collapsed (a vertex moved onto its neighbour: two faces with a zero-length side, every corner kind of
    the degenerate rule on a closed mesh) -- checked under both schemes against the fp64 definition; the reference's 'cotangent'
    is NaN here.  -> (vertices, indices, the two coincident vertices)"""
    v, f = (torch.from_numpy(a) for a in box(4, 11))
    a, b = int(f[0, 0]), int(f[0, 1])
    v[b] = v[a]
    return v, f, (a, b)


def mesh(name):
    """(vertices, indices) of a named mesh as CPU torch tensors."""
    gen, args, _, _ = MESHES[name]
    v, f = gen(*args)
    assert (v.shape[0], f.shape[0]) == SIZES[name], (name, v.shape, f.shape)
    return torch.from_numpy(v), torch.from_numpy(f)


def upstream(num_vertices, which):
    """The fixed seeded weight tensors W of loss = sum(normals * W): which = 0 the fixtures' own, 1 another dense one, 2 nonzero
    on one vertex only."""
    gen = torch.Generator().manual_seed(500 + which)
    w = torch.rand(num_vertices, 3, generator=gen) * 2.0 - 1.0
    if which == 2:
        keep = torch.zeros(num_vertices, 1)
        keep[num_vertices // 3] = 1.0
        w = w * keep
    return w


def e2e_mesh():
    """A smooth closed mesh: the vertices of box(4) pushed most of the way onto an ellipsoid.  98 vertices, 192 faces."""
    v, f = box(4, 51)
    v = v.astype(np.float64)
    on = v / np.linalg.norm(v / np.asarray([1.0, 0.7, 1.3]), axis=1, keepdims=True)
    return (1.1 * (0.2 * v + 0.8 * on)).astype(np.float32), f


def e2e_scene(device, vertices, indices, normals):
    """The mesh in front of the camera under one area light.  `vertices` is the leaf whose gradient is compared; `normals` is
    what a compute_vertex_normal made of it."""
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests')) if p not in sys.path]
    from redner_amd.render_pytorch import AreaLight, Camera, Material, Scene, Shape
    t = lambda x, dev=device, dtype=torch.float32: torch.tensor(x, dtype=dtype, device=dev)          # noqa: E731
    cam = Camera(position=t([0.4, 0.6, -5.0], 'cpu'), look_at=t([0.0, 0.0, 0.0], 'cpu'), up=t([0.0, 1.0, 0.0], 'cpu'),
                 fov=t([35.0], 'cpu'), clip_near=1e-2, resolution=E2E_RESOLUTION)
    mats = [Material(diffuse_reflectance=t([0.6, 0.5, 0.4])), Material(diffuse_reflectance=t([0.0, 0.0, 0.0]))]
    blob = Shape(vertices, indices, 0, normals=normals)
    light = Shape(t([[-1.5, 0.5, -7.0], [0.5, 0.5, -7.0], [-1.5, 2.5, -7.0], [0.5, 2.5, -7.0]]),
                  t([[0, 1, 2], [1, 3, 2]], dtype=torch.int32), 1)
    return Scene(cam, [blob, light], mats, [AreaLight(1, t([30.0, 30.0, 30.0], 'cpu'))])


def render_e2e(sc, device, backend):
    from redner_amd.render_pytorch import RenderFunction
    args = RenderFunction.serialize_scene(sc, E2E_SAMPLES, E2E_BOUNCES, sampler_type=backend.SamplerType.sobol, device=device,
                                          backend=backend)
    img = RenderFunction.apply(E2E_SEED, *args)
    (img * mk.upstream(img.shape).to(device)).sum().backward()
    return img


# ---- everything below needs the reference -------------------------------------------------------------------------------------
def check_cotangent_conditions(pyredner, name, vertices, indices):
    """The conditions of the module docstring.  The reference does not return its cotangent sum, so it is formed here in fp64
    (cot = e1 . e2 / |e1 x e2| per corner, index_add); the 'max' normal is the reference's own."""
    v = vertices.double()
    idx = indices.long()
    n_max = pyredner.compute_vertex_normal(v.float(), indices, 'max').double()
    total = torch.zeros_like(v)
    for i in range(3):
        p0, p1, p2 = v[idx[:, i]], v[idx[:, (i + 1) % 3]], v[idx[:, (i + 2) % 3]]
        e1, e2 = p1 - p0, p2 - p0
        cot = (e1 * e2).sum(1) / torch.linalg.cross(e1, e2, dim=1).norm(dim=1)
        total.index_add_(0, idx[:, (i + 1) % 3], (p2 - p1) * cot[:, None])
        total.index_add_(0, idx[:, (i + 2) % 3], -(p2 - p1) * cot[:, None])
    length = total.norm(dim=1)
    assert bool(((length - 0.05).abs() > 0.02).all()), (name, 'a cotangent sum near the fallback threshold', length.min())
    kept = length > 0.05
    align = (total * n_max).sum(1).abs()
    assert bool((align[kept] > 1e-3 * length[kept]).all()), (name, 'a cotangent sum at right angles to the max normal')
    assert int((~kept).sum()) == COTANGENT_FALLBACKS[name], (name, int((~kept).sum()))
    print(name, 'cotangent: %d of %d vertices fall back; kept lengths >= %.3g, fallback lengths <= %.3g'
          % (int((~kept).sum()), len(kept), float(length[kept].min()) if kept.any() else float('nan'),
             float(length[~kept].max()) if (~kept).any() else float('nan')))


def make_kernel_fixtures(pyredner):
    for name, (_, _, schemes, has_gradient) in MESHES.items():
        vertices, indices = mesh(name)
        out = {'vertices_sum': np.asarray(checksum(vertices)), 'indices_sum': np.asarray(checksum(indices))}
        for scheme in schemes:
            if scheme == 'cotangent':
                check_cotangent_conditions(pyredner, name, vertices, indices)
            x = vertices.clone().requires_grad_(True)
            normals = pyredner.compute_vertex_normal(x, indices, scheme)
            assert normals.dtype == torch.float32 and bool((normals.detach().norm(dim=1) > 0).all())
            out['normals_' + scheme] = normals.detach().numpy()
            if has_gradient:
                (normals * upstream(len(vertices), 0)).sum().backward()
                assert bool(torch.isfinite(x.grad).all()), (name, scheme, 'the reference gradient is not finite')
                out['d_vertices_' + scheme] = x.grad.numpy()
        np.savez_compressed(os.path.join(HERE, 'vertex_normal_%s.npz' % name), **out)
        print(name, {k: getattr(v, 'shape', ()) for k, v in out.items()})


def make_e2e_fixture(ref, pyredner):
    cpu = torch.device('cpu')
    v, f = e2e_mesh()
    vertices, indices = torch.from_numpy(v).requires_grad_(True), torch.from_numpy(f)
    sc = e2e_scene(cpu, vertices, indices, pyredner.compute_vertex_normal(vertices, indices))
    img = render_e2e(sc, cpu, ref)
    out = {'image': img.detach().numpy(), 'grad_vertices': vertices.grad.numpy(),
           'vertices_sum': np.asarray(checksum(vertices.detach())), 'indices_sum': np.asarray(checksum(indices))}
    assert np.isfinite(out['image']).all() and out['image'].max() > 0 and np.abs(out['grad_vertices']).sum() > 0
    np.savez_compressed(os.path.join(HERE, 'vertex_normal_e2e.npz'), **out)
    print('e2e', {k: v.shape for k, v in out.items()}, 'lit pixels', int((out['image'].sum(2) > 0).sum()),
          'vertices that get a gradient', int((np.abs(out['grad_vertices']).sum(1) > 0).sum()))


def main():
    # like make_golden.main: fresh zero pages for the reference's scratch buffers
    if os.environ.get('MALLOC_MMAP_THRESHOLD_') != '65536' or os.environ.get('MALLOC_PERTURB_') != '255':
        import subprocess
        env = dict(os.environ, MALLOC_MMAP_THRESHOLD_='65536', MALLOC_PERTURB_='255')
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    ref, pyredner = mk.reference_package()
    make_kernel_fixtures(pyredner)
    make_e2e_fixture(ref, pyredner)


if __name__ == '__main__':
    main()
