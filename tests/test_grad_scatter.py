"""The gradient scatter on its own: rdr::accum / accum_texel / accum_plain / accum_triple / accum_texel_triple (csrc/hip/exec.h),
scatter_trigrad_wave / scatter_positions_wave (csrc/surface.h) and the fold of GradStore + FlushGrad (csrc/grad_store.h,
csrc/stages_bwd.h), driven through rdr_debug_grad_scatter: the real gradient store, ONE stage whose lanes call one of those
functions, the real flush into the caller's fp32 tensors.

The operation is a scatter-add.  The exact leg adds integers in [-8, 8] to tensors pre-filled with small non-zero integers; the
test asserts of its own reference that |pre-fill| + sum |addends| < 2^24 for every element, so every partial sum is an integer
that fp32 and fp64 hold exactly, in any order, and the comparison with np.add.at on int64 is bit for bit (np.array_equal) --
over every element of every gradient tensor and the guard floats on either side of each.  The rounding leg adds non-dyadic
doubles of magnitudes 2^-20 .. 2^20 to zeroed tensors and holds every element to
    |out - exact| <= 2^-24 |exact| + n 2^-53 sum |v|          (exact: math.fsum of the element's n addends)
i.e. one rounding to fp32 of a sum whose fp64 additions -- at most n - 1 that are not additions of zero, in whatever order the
lanes, rounds, replicas and the fold perform them -- each lose at most 2^-53 of a partial sum that sum |v| bounds.

Lanes map to waves as i // 64 and to workgroups as i // 256.  On the CPU harness the first layer is `*p += v` and there is one
replica, so the legs on `hostsim_backend` check the plumbing, this file's reference, the layout of GradStore and FlushGrad; the
legs on `gpu_backend` check the wave-cooperative code, the replicas and the tiers where they run.

What the GPU legs were seen to catch (each change built once into a scratch library, never committed; one run each):
    accum_rounds without its final `if (mine)` add          accum / accum_texel / trigrad_wave exact cases with a lone lane
                                                            (all layouts but n63, whose 63 lanes share one address), tiers
    wave_sum without the row_mirror step                    every op but accum_plain, layouts all / n65 / n513 / neg_shape
                                                            (the butterfly only runs in a full wave)
    scatter_trigrad_wave skipping groups of exactly 4       trigrad_wave all / neg_shape, plain and not (runs345, runs543)
      lanes that it still marks as handled
    replica_of treating every address as small-tier         all eight tiers cases, nothing else
    FlushGrad leaving out the last replica                  all eight tiers cases, nothing else (needs a wave id that selects it)"""
import ctypes
import math

import numpy as np
import pytest
import torch

from redner_amd import _capi

K_SMALL_TENSOR, K_SMALL_TIER_MAX = 16384, 65536          # GradStore::kSmallTensor / kSmallTierMax (doubles)
LARGE_TIER_BUDGET = 256 << 20                            # exec::replica_budget of a short job (bytes)
PAD = 8                                                  # guard floats on either side of every gradient tensor
OPS = {'accum': (_capi.SCATTER_ACCUM, 1), 'accum_texel': (_capi.SCATTER_ACCUM_TEXEL, 1), 'accum_plain': (_capi.SCATTER_ACCUM_PLAIN, 1),
       'accum_triple': (_capi.SCATTER_ACCUM_TRIPLE, 3), 'accum_texel_triple': (_capi.SCATTER_ACCUM_TEXEL_TRIPLE, 3),
       'trigrad_wave': (_capi.SCATTER_TRIGRAD_WAVE, 33), 'positions_wave': (_capi.SCATTER_POSITIONS_WAVE, 9)}
# (op, plain): the call-wide flag only means something to scatter_trigrad_wave
VARIANTS = [('accum', 0), ('accum_texel', 0), ('accum_plain', 0), ('accum_triple', 0), ('accum_texel_triple', 0),
            ('trigrad_wave', 0), ('trigrad_wave', 1), ('positions_wave', 0)]
VARIANT_IDS = ['%s%s' % (o, '-plain' if p else '') for o, p in VARIANTS]
TEX_SLOTS = ('diffuse', 'specular', 'roughness', 'generic', 'normal_map')


# ---- address groups of one wave: group id of each of the 64 lanes ---------------------------------------------------------------
def _runs(lengths):
    out, g = [], 0
    while len(out) < 64:
        out += [g] * lengths[g % len(lengths)]
        g += 1
    return np.asarray(out[:64])


_L = np.arange(64)
PATTERNS = {
    'same': np.zeros(64, int),                             # all 64 lanes on one address
    'mod2': _L % 2, 'mod3': _L % 3,                        # within the 3 rounds of accum
    'mod4': _L % 4,                                        # one more than the rounds; four groups >= 4 lanes: the fourth falls back
    'mod9': _L % 9, 'mod10': _L % 10,                      # around the 8 texel rounds
    'distinct': _L.copy(),
    'loner_first': (_L == 0).astype(int),                  # the loner is the first leader, then a group of 63
    'loner_last': (_L == 63).astype(int),
    'ones_twos': (_L // 3) * 2 + (_L % 3 != 0),            # groups of 1 and 2 lanes: the `< 2` rule of accum
    'runs345': _runs([3, 4, 5]), 'runs543': _runs([5, 4, 3]),        # the `< 4` rule of the two *_wave ops
    'three_big_rest_alone': np.where(_L < 48, _L % 3, _L),           # three handled groups, sixteen lanes left to the fallback
    'big_pair_big': np.where(_L < 30, 0, np.where(_L < 32, 1, 2)),
}


def _waves_of_patterns():
    """Two waves per pattern; the second shifts the groups onto other addresses that overlap the first wave's."""
    return [(name, shift) for name in PATTERNS for shift in (0, 5)]


def _activity(kind, num_waves, rng):
    act = np.ones((num_waves, 64), np.uint8)
    if kind == 'even':
        act[:, 1::2] = 0
    elif kind == 'low32':
        act[:, 32:] = 0
    elif kind == 'lane63':
        act[:, :63] = 0
    elif kind == 'random':
        act = (rng.random((num_waves, 64)) < 0.6).astype(np.uint8)
    elif kind == 'empty_waves':                            # whole waves with nothing to do among busy ones
        act = (rng.random((num_waves, 64)) < 0.8).astype(np.uint8)
        act[1::3] = 0
    else:
        assert kind in ('all', 'neg_shape')
    return act.reshape(-1)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def _grid(nx, ny, rng, drop=0):
    """(nx x ny quads) * 2 triangles on shared vertices."""
    v = rng.uniform(-1.0, 1.0, ((nx + 1) * (ny + 1), 3)).astype(np.float32)
    idx = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            idx += [[a, a + nx + 1, a + 1], [a + 1, a + nx + 1, a + nx + 2]]
    idx = np.asarray(idx, np.int32)
    return v, idx[:len(idx) - drop]


def _shape(rng, nx, ny, drop=0, uvs=False, normals=False, colors=False, own_uv_idx=False, own_n_idx=False, material=0, light=-1,
           d=('v', 'uv', 'n', 'c'), extra_vertices=0):
    v, idx = _grid(nx, ny, rng, drop)
    if extra_vertices:                                     # vertices no triangle uses: a large gradient tensor on a small mesh
        v = np.concatenate([v, rng.uniform(-1.0, 1.0, (extra_vertices, 3)).astype(np.float32)])
    s = dict(v=v, idx=idx, uv=None, n=None, c=None, uv_idx=None, n_idx=None, material=material, light=light, d=d)
    if uvs:
        count = len(v) + 3 if own_uv_idx else len(v)
        s['uv'] = rng.uniform(0.0, 1.0, (count, 2)).astype(np.float32)
        if own_uv_idx:
            s['uv_idx'] = rng.integers(0, count, idx.shape).astype(np.int32)
    if normals:
        count = len(v) - 2 if own_n_idx else len(v)
        s['n'] = rng.uniform(-1.0, 1.0, (count, 3)).astype(np.float32)
        if own_n_idx:
            s['n_idx'] = rng.integers(0, count, idx.shape).astype(np.int32)
    if colors:
        s['c'] = rng.uniform(0.0, 1.0, (len(v), 3)).astype(np.float32)
    return s


def _spec_mixed():
    """Small tensors of every kind: shapes with and without normals / uvs / colours, own uv and normal indices, DShapes that
    leave a gradient out, 512 and 511 triangles (the plain-atomics branch of scatter_trigrad), a mip-mapped and a constant
    texture, two lights, a look-at camera, an environment map; shapes 1 and 6 share ONE vertex-gradient tensor."""
    rng = np.random.default_rng(11)
    shapes = [
        _shape(rng, 4, 4, uvs=True, normals=True, colors=True, own_uv_idx=True, own_n_idx=True, material=1),
        _shape(rng, 2, 2, light=1),
        _shape(rng, 3, 2, uvs=True, normals=True, colors=True, d=('v', 'n')),              # no uv / colour gradient asked for
        _shape(rng, 2, 3, uvs=True, normals=True, colors=True, d=('v', 'uv', 'c')),        # no normal gradient asked for
        _shape(rng, 16, 16, uvs=True, normals=True),                                       # exactly 512 triangles
        _shape(rng, 16, 16, drop=1, uvs=True, normals=True, colors=True),                  # 511
        _shape(rng, 2, 2, light=0),
    ]
    return dict(shapes=shapes, lights=[6, 1], envmap=[(4, 8), (2, 4)], alias={('v', 6): ('v', 1)},
                materials=[dict(diffuse=[]), dict(diffuse=[(8, 8), (4, 4)], roughness=[(16, 16)])])


def _spec_tiers():
    """One tensor of the small tier, one above kSmallTensor, four that fill the small tier, one that is small by size but comes
    after the tier is full, a 512 x 512 x 3 texel gradient, and the camera (small again: 3 doubles still fit)."""
    rng = np.random.default_rng(12)
    shapes = [_shape(rng, 2, 2), _shape(rng, 4, 4, extra_vertices=5500, normals=True)]
    shapes += [_shape(rng, 2, 2, extra_vertices=5391) for _ in range(4)]
    shapes += [_shape(rng, 4, 4, extra_vertices=275), _shape(rng, 1, 1, light=0, material=1)]
    return dict(shapes=shapes, lights=[7], envmap=None, alias={}, materials=[dict(diffuse=[(512, 512)]), dict(diffuse=[])])


def _spec_apart():
    """`mixed` with a tensor of its own for every entry: an fp32 tensor that two accumulators fold into is rounded twice."""
    return dict(_spec_mixed(), alias={})


SPECS = {'mixed': _spec_mixed, 'apart': _spec_apart, 'tiers': _spec_tiers}


def _tensor_counts(spec):
    """(name, elements) of every gradient tensor, in the order GradStore::layout places them."""
    out = []
    for i, s in enumerate(spec['shapes']):
        for key, width in (('v', 3), ('uv', 2), ('n', 3), ('c', 3)):
            if s[key] is not None and key in s['d']:
                out.append(((key, i), width * len(s[key])))
    for i, m in enumerate(spec['materials']):
        for slot, name in enumerate(TEX_SLOTS):
            if name in ('generic', 'normal_map'):          # absent in these scenes
                continue
            ch, levels = (1 if name == 'roughness' else 3), m.get(name, [])        # []: a constant
            if not levels:
                out.append((('tex', i, slot, 0), ch))
            for k, (h, w) in enumerate(levels):
                out.append((('tex', i, slot, k), h * w * ch))
    if spec['lights']:
        out.append((('lights',), 3 * len(spec['lights'])))
    out += [(('cam', 0), 3), (('cam', 1), 3), (('cam', 2), 3), (('cam', 5), 9), (('cam', 6), 9)]
    for k, (h, w) in enumerate(spec['envmap'] or []):
        out.append((('env', k), h * w * 3))
    return out


def _tiers(spec):
    """Tier of every accumulator and the replicas of the large tier, from the sizes and the constants above (GradStore::place)."""
    cursor, tier = [0, 0], {}
    for name, count in _tensor_counts(spec):
        padded = (count + 3) & ~3
        t = 0 if count <= K_SMALL_TENSOR and cursor[0] + padded <= K_SMALL_TIER_MAX else 1
        cursor[t] += padded
        tier[name] = t
    stride = (cursor[1] + 31) & ~31
    replicas = 256
    while replicas > 1 and stride * 8 * replicas > LARGE_TIER_BUDGET:
        replicas >>= 1
    return tier, replicas


class Built:
    """A Scene, a DScene whose gradient tensors are pre-filled and guarded, and what the reference needs to know about both."""

    def __init__(self, backend, device, spec):
        rd, self.spec, self.device, self.keep = backend, spec, device, []
        on_gpu = device.type == 'cuda'

        def dev(a):
            t = torch.tensor(np.ascontiguousarray(a), device=device)          # a copy, also on the CPU
            self.keep.append(t)
            return t

        def fp(t):
            return rd.float_ptr(t.data_ptr() if t is not None else 0)

        def ip(t):
            return rd.int_ptr(t.data_ptr() if t is not None else 0)

        def host(vals):
            a = np.asarray(vals, np.float32)
            self.keep.append(a)
            return rd.float_ptr(a.ctypes.data)

        eye3 = host(np.eye(3).reshape(-1))
        camera = rd.Camera(32, 32, host([0, 0, -5]), host([0, 0, 0]), host([0, 1, 0]), rd.float_ptr(0), rd.float_ptr(0), eye3, eye3,
                           rd.float_ptr(0), 1e-2, rd.CameraType.perspective, rd.Vector2i(0, 0), rd.Vector2i(32, 32))
        shapes = []
        for s in spec['shapes']:
            t = {k: (dev(s[k]) if s[k] is not None else None) for k in ('v', 'idx', 'uv', 'n', 'uv_idx', 'n_idx', 'c')}
            shapes.append(rd.Shape(fp(t['v']), ip(t['idx']), fp(t['uv']), fp(t['n']), ip(t['uv_idx']), ip(t['n_idx']), fp(t['c']),
                                   len(s['v']), len(s['uv']) if s['uv'] is not None else 0,
                                   len(s['n']) if s['n'] is not None else 0, len(s['idx']), s['material'], s['light']))
        rng = np.random.default_rng(5)
        uv_scale = dev(np.ones(2, np.float32))

        def texture(cls, levels, ch):
            if levels is None:
                return cls([], [], [], 0, rd.float_ptr(0))
            if not levels:
                return cls([fp(dev(rng.uniform(0.1, 0.9, ch).astype(np.float32)))], [0], [0], ch, fp(uv_scale))
            return cls([fp(dev(rng.uniform(0.1, 0.9, (h, w, ch)).astype(np.float32))) for h, w in levels],
                       [w for h, w in levels], [h for h, w in levels], ch, fp(uv_scale))

        materials = [rd.Material(texture(rd.Texture3, m['diffuse'], 3), texture(rd.Texture3, m.get('specular', []), 3),
                                 texture(rd.Texture1, m.get('roughness', []), 1), texture(rd.TextureN, None, 0),
                                 texture(rd.Texture3, None, 3), False, False, False) for m in spec['materials']]
        lights = [rd.AreaLight(sid, host([2.0, 3.0, 4.0]), False, True) for sid in spec['lights']]
        envmap = None
        if spec['envmap']:
            h, w = spec['envmap'][0]
            eye4 = host(np.eye(4).reshape(-1))
            envmap = rd.EnvironmentMap(texture(rd.Texture3, spec['envmap'], 3), eye4, eye4, fp(dev(np.linspace(0, 1, h, dtype=np.float32))),
                                       fp(dev(np.linspace(0, 1, h * w, dtype=np.float32))), 1.0, True)
        # both edge-sampling flags off: no edge structures are built
        self.scene = rd.Scene(camera, shapes, materials, lights, envmap, on_gpu, 0, False, False)

        # ---- gradient tensors: [PAD guards | the tensor | PAD guards], every float a small non-zero integer -----------------------
        self.counts = dict(_tensor_counts(spec))
        self.alias = dict(spec['alias'])
        for a, b in self.alias.items():
            assert self.counts[a] == self.counts[b]
        self.buffers = [n for n in self.counts if n not in self.alias]
        fill = np.random.default_rng(6)
        self.prefill = {n: fill.choice([-3, -2, -1, 1, 2, 3], self.counts[n] + 2 * PAD).astype(np.float32) for n in self.buffers}
        self.grads = {n: dev(self.prefill[n]) for n in self.buffers}

        def g(name):
            name = self.alias.get(name, name)
            return rd.float_ptr(self.grads[name].data_ptr() + 4 * PAD) if name in self.grads else rd.float_ptr(0)

        d_camera = rd.DCamera(g(('cam', 0)), g(('cam', 1)), g(('cam', 2)), rd.float_ptr(0), rd.float_ptr(0), g(('cam', 5)), g(('cam', 6)),
                              rd.float_ptr(0))
        d_shapes = [rd.DShape(g(('v', i)), g(('uv', i)), g(('n', i)), g(('c', i))) for i in range(len(shapes))]

        def d_texture(cls, i, slot):
            names = sorted(n for n in self.counts if n[:3] == ('tex', i, slot))
            return cls([g(n) for n in names], [0] * len(names), [0] * len(names), 0, rd.float_ptr(0))

        d_materials = [rd.DMaterial(d_texture(rd.Texture3, i, 0), d_texture(rd.Texture3, i, 1), d_texture(rd.Texture1, i, 2),
                                    d_texture(rd.TextureN, i, 3), d_texture(rd.Texture3, i, 4)) for i in range(len(materials))]
        # the intensities are one accumulator block in the store and one fp32[3] per light in the DScene
        light_base = self.grads[('lights',)].data_ptr() + 4 * PAD if lights else 0
        d_lights = [rd.DAreaLight(rd.float_ptr(light_base + 12 * k)) for k in range(len(lights))]
        d_envmap = None
        if envmap is not None:
            names = sorted(n for n in self.counts if n[0] == 'env')
            d_envmap = rd.DEnvironmentMap(rd.Texture3([g(n) for n in names], [0] * len(names), [0] * len(names), 3, rd.float_ptr(0)),
                                          rd.float_ptr(0))
        self.d_scene = rd.DScene(d_camera, d_shapes, d_materials, d_lights, d_envmap, on_gpu, 0)
        self.backend = rd

    def target(self, name):
        """(kind, a, b) of rdr_debug_grad_scatter for a tensor of the DScene."""
        kind = {'v': _capi.TARGET_VERTICES, 'uv': _capi.TARGET_UVS, 'n': _capi.TARGET_NORMALS, 'c': _capi.TARGET_COLORS,
                'tex': _capi.TARGET_TEXTURE, 'lights': _capi.TARGET_LIGHTS, 'cam': _capi.TARGET_CAMERA, 'env': _capi.TARGET_ENVMAP}[name[0]]
        if name[0] == 'tex':
            return kind, name[1], name[2] * _capi.MAX_MIP + name[3]
        if name[0] == 'env':
            return kind, 0, name[1]
        return kind, (name[1] if len(name) > 1 else 0), 0

    def reset(self, zero=False):
        for n in self.buffers:
            self.grads[n].copy_(torch.from_numpy(self.prefill[n]))
            if zero:
                self.grads[n][PAD:PAD + self.counts[n]] = 0

    def call(self, op, plain, active, target, index, values, expect=0):
        lib = self.scene._lib
        self.backend._use_torch_stream(lib, self.device.type == 'cuda', 0)
        active, target = np.ascontiguousarray(active, np.uint8), np.ascontiguousarray(target, np.int32)
        index, values = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(values, np.float64)
        n = len(active)
        assert target.shape == (n, 3) and index.shape == (n,) and values.shape == (n, OPS[op][1])
        rc = lib.rdr_debug_grad_scatter(self.scene._handle, ctypes.byref(self.d_scene._desc), 1024, OPS[op][0], plain, n,
                                        active.ctypes.data, target.ctypes.data, index.ctypes.data, values.ctypes.data)
        assert rc == expect, lib.rdr_last_error()
        return {b: self.grads[b].cpu().numpy() for b in self.buffers}


_BUILT = {}


def _built(backend, name):
    """One Scene per library and spec for the whole session (the gradient tensors are reset by every case)."""
    lib = _capi.lib()
    key = (_capi.library_path(), name)
    if key not in _BUILT or _BUILT[key].scene._lib is not lib:
        device = torch.device('cuda:0' if _capi.is_product_library() else 'cpu')
        _BUILT[key] = Built(backend, device, SPECS[name]())
    return _BUILT[key]


# ---- what a launch asks for, and the addends that follow from it ---------------------------------------------------------------
def _address_pool(built, width):
    """(tensor, element) addresses, neighbours in the list on different tensors: every kind of target, each tier."""
    per_tensor = []
    for name, count in built.counts.items():
        if width == 3 and count % 3:
            continue
        slots = count // width
        take = sorted(set(np.linspace(0, slots - 1, min(slots, 12)).astype(int).tolist()))
        per_tensor.append([(name, width * k) for k in take])
    pool, k = [], 0
    while any(k < len(p) for p in per_tensor):
        pool += [p[k] for p in per_tensor if k < len(p)]
        k += 1
    assert len(pool) >= 64
    return pool


def _triangle_pool(built, shapes=None):
    """(shape, triangle) keys, neighbours in the list on different shapes and, within a shape, on triangles that share vertices."""
    per_shape = [[(s, t) for t in range(min(len(sp['idx']), 32))] for s, sp in enumerate(built.spec['shapes'])
                 if shapes is None or s in shapes]
    pool, k = [], 0
    while any(k < len(p) for p in per_shape):
        pool += [p[k] for p in per_shape if k < len(p)]
        k += 1
    assert len(pool) >= 64
    return pool


def _launch(built, op, waves, activity, seed, num_lanes=None, integers=True, pool=None):
    """Per-lane arrays of one call.  `waves`: (pattern, shift) per wave; lane l of wave w is in group PATTERNS[pattern][l] and
    group g of the wave works on entry (g + shift + 3 w) of the pool, so waves overlap on some addresses and not on others."""
    rng = np.random.default_rng(seed)
    width = OPS[op][1]
    tri_op = op.endswith('_wave')
    if pool is None:
        pool = _triangle_pool(built) if tri_op else _address_pool(built, width)
    assert len(pool) >= 64                                 # 64 distinct groups stay 64 distinct addresses
    gid = np.concatenate([(PATTERNS[p] + shift + 3 * w) % len(pool) for w, (p, shift) in enumerate(waves)])
    n = len(gid)
    active = _activity(activity, len(waves), rng)
    target, index = np.zeros((n, 3), np.int32), np.zeros(n, np.int32)
    if tri_op:
        keys = np.asarray(pool, np.int32)[gid]
        target[:, :2] = keys
        if activity in ('neg_shape', 'random', 'empty_waves'):          # shape < 0 in full waves and in partly active ones
            target[rng.random(n) < (0.3 if activity == 'neg_shape' else 0.1), 0] = -1
    else:
        for i, (name, at) in enumerate(pool[k] for k in gid):
            target[i] = built.target(name)
            index[i] = at
    if integers:
        values = rng.integers(-8, 9, (n, width)).astype(np.float64)
    else:                                                  # non-dyadic, magnitudes 2^-20 .. 2^20, both signs
        values = rng.choice([-1.0, 1.0], (n, width)) * np.exp2(rng.uniform(-20.0, 20.0, (n, width))) * (1.0 + rng.random((n, width)) / 3.0)
    if num_lanes is not None:
        active, target, index, values = active[:num_lanes], target[:num_lanes], index[:num_lanes], values[:num_lanes]
    names = None if tri_op else [pool[k][0] for k in gid[:len(active)]]
    return dict(op=op, active=active, target=target, index=index, values=values, names=names)


def _addends(built, L, plain):
    """Every single add the call must perform: (buffer, element, value) arrays.  Add ops: the lane's value(s) at index, index + 1,
    index + 2.  Triangle ops, the rules of scatter_trigrad: vertices always receive p; normals receive n when the shape and
    the DShape have them, through normal_indices when given; uvs and colours receive uv and c only when `plain` is false."""
    buf_of = {n: built.buffers.index(built.alias.get(n, n)) for n in built.counts}
    live = L['active'] != 0
    bufs, elems, vals = [], [], []

    def add(b, e, v):
        bufs.append(np.full(len(e), b)), elems.append(np.asarray(e, np.int64)), vals.append(np.asarray(v, np.float64))

    if L['names'] is not None:
        lane_buf = np.asarray([buf_of[n] for n in L['names']])
        for j in range(L['values'].shape[1]):
            for b in np.unique(lane_buf[live]):
                sel = live & (lane_buf == b)
                add(b, L['index'][sel] + j, L['values'][sel, j])
    else:
        v = L['values']
        for s, sp in enumerate(built.spec['shapes']):
            sel = live & (L['target'][:, 0] == s)
            if not sel.any():
                continue
            tri = L['target'][sel, 1]
            for k in range(3):
                vi = sp['idx'][tri, k].astype(np.int64)
                ni = sp['n_idx'][tri, k].astype(np.int64) if sp['n_idx'] is not None else vi
                ui = sp['uv_idx'][tri, k].astype(np.int64) if sp['uv_idx'] is not None else vi
                for c in range(3):
                    add(buf_of[('v', s)], 3 * vi + c, v[sel, 3 * k + c])
                if L['op'] == 'positions_wave':
                    continue
                if ('n', s) in buf_of:
                    for c in range(3):
                        add(buf_of[('n', s)], 3 * ni + c, v[sel, 9 + 3 * k + c])
                if not plain and ('uv', s) in buf_of:
                    for c in range(2):
                        add(buf_of[('uv', s)], 2 * ui + c, v[sel, 18 + 2 * k + c])
                if not plain and ('c', s) in buf_of:
                    for c in range(3):
                        add(buf_of[('c', s)], 3 * vi + c, v[sel, 24 + 3 * k + c])
    if not bufs:
        return np.zeros(0, int), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(bufs), np.concatenate(elems), np.concatenate(vals)


def _check_exact(built, L, plain):
    built.reset()
    got = built.call(L['op'], plain, L['active'], L['target'], L['index'], L['values'])
    bufs, elems, vals = _addends(built, L, plain)
    touched = 0
    for b, name in enumerate(built.buffers):
        sel = bufs == b
        want = built.prefill[name].astype(np.int64)
        bound = np.abs(want)
        assert (elems[sel] >= 0).all() and (elems[sel] < built.counts[name]).all()
        np.add.at(want, PAD + elems[sel], vals[sel].astype(np.int64))
        np.add.at(bound, PAD + elems[sel], np.abs(vals[sel]).astype(np.int64))
        assert bound.max() < 2 ** 24                       # of the reference: every partial sum is exact in fp32 and fp64
        touched += int(sel.sum())
        # bit for bit: the targeted elements, the ones no lane targeted, the guards on both sides
        assert np.array_equal(got[name], want.astype(np.float32)), \
            (name, np.flatnonzero(got[name] != want.astype(np.float32))[:8] - PAD)
    assert touched == len(vals)
    return got


# ---- the exact leg ------------------------------------------------------------------------------------------------------------------
LAYOUTS = ['all', 'even', 'low32', 'lane63', 'random', 'empty_waves', 'neg_shape', 'n1', 'n63', 'n65', 'n513']
# (shape < 0 on a seeded subset: only the triangle ops take a shape)
EXACT_CASES = [(v, l) for v in VARIANTS for l in LAYOUTS if l != 'neg_shape' or v[0].endswith('_wave')]
EXACT_IDS = ['%s-%s' % (VARIANT_IDS[VARIANTS.index(v)], l) for v, l in EXACT_CASES]


def _exact_case(backend, variant, layout):
    op, plain = variant
    built = _built(backend, 'mixed')
    seed = 1000 + 37 * VARIANTS.index(variant) + LAYOUTS.index(layout)
    if layout[1:].isdigit():
        L = _launch(built, op, _waves_of_patterns(), 'all', seed, num_lanes=int(layout[1:]))      # the ragged last wave
    else:
        L = _launch(built, op, _waves_of_patterns(), layout, seed)
    _check_exact(built, L, plain)


@pytest.mark.parametrize('case', EXACT_CASES, ids=EXACT_IDS)
def test_scatter_exact_hostsim(hostsim_backend, case):
    _exact_case(hostsim_backend, *case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', EXACT_CASES, ids=EXACT_IDS)
def test_scatter_exact_gpu(gpu_backend, case):
    _exact_case(gpu_backend, *case)


# ---- tiers and replicas ---------------------------------------------------------------------------------------------------------------
def _tiers_case(backend, variant):
    """Lanes of one wave split between the tiers, 1101 waves (256 * 275 + 1 lanes) so that `wave & mask` wraps the 256 replicas of
    the small tier and the fewer ones of the large tier several times."""
    op, plain = variant
    built = _built(backend, 'tiers')
    tier, large_replicas = _tiers(built.spec)
    small, big, late, texels = ('v', 0), ('v', 1), ('v', 6), ('tex', 0, 0, 0)
    assert built.counts[small] <= K_SMALL_TENSOR and tier[small] == 0
    assert built.counts[big] > K_SMALL_TENSOR and tier[big] == 1
    assert built.counts[late] <= K_SMALL_TENSOR and tier[late] == 1          # small by size, placed after the tier was full
    assert all(tier[('v', s)] == 0 and built.counts[('v', s)] <= K_SMALL_TENSOR for s in (2, 3, 4, 5))
    assert built.counts[texels] == 512 * 512 * 3 and tier[texels] == 1
    assert tier[('cam', 0)] == 0 and tier[('n', 1)] == 1
    assert 1 < large_replicas < 256
    num_waves = 1101
    waves = [(('mod4', 'mod2', 'same', 'distinct', 'mod9', 'ones_twos')[w % 6], w % 11) for w in range(num_waves)]
    if op.endswith('_wave'):
        pool = _triangle_pool(built, shapes=(0, 1, 6, 7))
    else:
        width = OPS[op][1]
        per = [[(name, width * k) for k in np.linspace(0, built.counts[name] // width - 1, 24).astype(int)]
               for name in (small, big, late, texels, ('cam', 0), ('n', 1))]
        pool = [p[k % len(p)] for k in range(24) for p in per]
        pool = list(dict.fromkeys(pool))
    L = _launch(built, op, waves, 'random', 77 + VARIANTS.index(variant), num_lanes=256 * 275 + 1, pool=pool)
    _check_exact(built, L, plain)


@pytest.mark.parametrize('variant', VARIANTS, ids=VARIANT_IDS)
def test_scatter_tiers_hostsim(hostsim_backend, variant):
    _tiers_case(hostsim_backend, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS, ids=VARIANT_IDS)
def test_scatter_tiers_gpu(gpu_backend, variant):
    _tiers_case(gpu_backend, variant)


# ---- the rounding leg -----------------------------------------------------------------------------------------------------------------
def _rounding_case(backend, variant):
    op, plain = variant
    built = _built(backend, 'apart')
    L = _launch(built, op, _waves_of_patterns(), 'random', 500 + VARIANTS.index(variant), integers=False)
    built.reset(zero=True)                                 # 0 + (float)sum is exact: ONE rounding to fp32, as the bound says
    got = built.call(op, plain, L['active'], L['target'], L['index'], L['values'])
    bufs, elems, vals = _addends(built, L, plain)
    assert len(vals) > 1000
    per_element = {}
    for b, e, v in zip(bufs.tolist(), elems.tolist(), vals.tolist()):
        per_element.setdefault((b, e), []).append(v)
    assert max(len(v) for v in per_element.values()) >= 16
    for b, name in enumerate(built.buffers):
        out = got[name].astype(np.float64)
        want = built.prefill[name].astype(np.float64)
        want[PAD:PAD + built.counts[name]] = 0
        for (bb, e), v in per_element.items():
            if bb != b:
                continue
            exact = math.fsum(v)
            bound = 2.0 ** -24 * abs(exact) + len(v) * 2.0 ** -53 * math.fsum(abs(x) for x in v)
            assert abs(out[PAD + e] - exact) <= bound, (name, e, out[PAD + e], exact, bound, len(v))
            want[PAD + e] = out[PAD + e]
        assert np.array_equal(out, want), name               # everything else: untouched


@pytest.mark.parametrize('variant', VARIANTS, ids=VARIANT_IDS)
def test_scatter_rounding_hostsim(hostsim_backend, variant):
    _rounding_case(hostsim_backend, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS, ids=VARIANT_IDS)
def test_scatter_rounding_gpu(gpu_backend, variant):
    _rounding_case(gpu_backend, variant)


# ---- the hook refuses what could leave the accumulators ---------------------------------------------------------------------------------
def _refusal_case(backend):
    built = _built(backend, 'mixed')
    built.reset()
    one = np.ones(1, np.uint8)

    def refused(op, target, index, active=one):
        got = built.call(op, 0, active, np.asarray([target], np.int32), np.asarray([index], np.int32), np.ones((1, OPS[op][1])), expect=1)
        assert 'rdr_debug_grad_scatter' in built.scene._lib.rdr_last_error().decode()
        for name in built.buffers:                         # nothing was launched, nothing was folded
            assert np.array_equal(got[name], built.prefill[name]), name

    count = built.counts[('v', 0)]
    refused('accum', built.target(('v', 0)), count)
    refused('accum', built.target(('v', 0)), -1)
    refused('accum', built.target(('v', 0)), count, active=np.zeros(1, np.uint8))       # inactive lanes are checked too
    refused('accum_triple', built.target(('v', 0)), count - 2)                          # index + 2 is past the end
    refused('accum_texel_triple', built.target(('tex', 0, 0, 0)), 1)                    # a constant colour has 3 elements
    refused('accum', (_capi.TARGET_UVS, 2, 0), 0)                                       # the DShape asks for no uv gradient
    refused('accum', (_capi.TARGET_NORMALS, 1, 0), 0)                                   # the shape has no normals
    refused('accum', (_capi.TARGET_VERTICES, len(built.spec['shapes']), 0), 0)
    refused('accum', (_capi.TARGET_TEXTURE, 1, 0 * _capi.MAX_MIP + 2, ), 0)             # level 2 of a two-level texture
    refused('accum', (_capi.TARGET_TEXTURE, 0, 3 * _capi.MAX_MIP), 0)                   # no generic texture
    refused('accum', (_capi.TARGET_CAMERA, 3, 0), 0)                                    # look-at camera: no cam_to_world gradient
    refused('accum', (_capi.TARGET_CAMERA, 8, 0), 0)
    refused('accum', (_capi.TARGET_LIGHTS, 0, 0), 3 * len(built.spec['lights']))
    refused('accum', (_capi.TARGET_ENVMAP, 0, 2), 0)
    refused('accum', (99, 0, 0), 0)
    refused('trigrad_wave', (len(built.spec['shapes']), 0, 0), 0)
    refused('trigrad_wave', (5, 511, 0), 0)                                             # the shape with 511 triangles
    refused('positions_wave', (0, -1, 0), 0)
    # and the last element of a tensor is in range
    L = dict(op='accum_triple', active=one, target=np.asarray([built.target(('v', 0))], np.int32), index=np.asarray([count - 3], np.int32),
             values=np.asarray([[1.0, 2.0, 3.0]]), names=[('v', 0)])
    _check_exact(built, L, 0)


def test_scatter_hook_refuses_out_of_range_hostsim(hostsim_backend):
    _refusal_case(hostsim_backend)


@pytest.mark.gpu
def test_scatter_hook_refuses_out_of_range_gpu(gpu_backend):
    _refusal_case(gpu_backend)


def test_patterns_are_what_they_claim():
    """Of this file's own generators: group sizes, and that the mixed launch really covers what its docstrings say."""
    sizes = {n: np.bincount(p) for n, p in PATTERNS.items()}
    assert sizes['same'].tolist() == [64] and len(sizes['distinct']) == 64 and sizes['distinct'].max() == 1
    for g in (2, 3, 4, 9, 10):
        assert len(sizes['mod%d' % g]) == g
    assert sizes['loner_first'].tolist() == [63, 1] and PATTERNS['loner_first'][0] == 1
    assert sizes['loner_last'].tolist() == [63, 1] and PATTERNS['loner_last'][63] == 1
    assert set(sizes['ones_twos'].tolist()) == {1, 2}
    assert {3, 4, 5} <= set(sizes['runs345'].tolist()) and PATTERNS['runs345'][:12].tolist() == [0] * 3 + [1] * 4 + [2] * 5
    assert (sizes['mod4'] >= 4).all() and len(sizes['mod4']) == 4
    assert sizes['big_pair_big'].tolist() == [30, 2, 32]
    spec = _spec_mixed()
    assert [len(s['idx']) for s in spec['shapes']][4:6] == [512, 511]
