"""Deferred shading and the render_* family on the MI355X-native renderer.

The names, arguments and meaning are those of the reference's `pyredner/render_utils.py`, so a pyredner deferred-shading script
needs only its import line changed:

    from redner_amd import render_deferred, PointLight, AmbientLight

    img = render_deferred(scene, [AmbientLight(ia), PointLight(pos, ip)], aa_samples=2, seed=1)
    img.sum().backward()          # gradients reach the scene AND ia, pos, ip

The G-buffer (position, shading normal, diffuse reflectance[, alpha]) comes from `RenderFunction` at `aa_samples` times the
resolution; the lights, their sum and the anti-aliasing resolve are ONE native kernel (`rdr_deferred_shade`,
csrc/deferred.h), its adjoint another -- where the reference composes ~15 whole-image torch operations per light.  There is
no fall-back to torch operations: without the native library the call raises.

Per G-buffer texel with position p, normal n, albedo a, summed over the lights (I: the light's rgb intensity):

    AmbientLight      I * a
    PointLight        d = pos - p, l = d / |d|:       I * max(l.n, 0) * (a / pi) / d.d
    DirectionalLight  l = -dir / |dir|:               I * max(l.n, 0) * (a / pi)
    SpotLight         l = (pos - p) / |pos - p|, s = -sdir / |sdir|:
                                                      I * pow(max(l.s, 0), e) * max(l.n, 0) * (a / pi)
    SHLight           x = -n.z, y = n.x, z = n.y;  per colour channel c, with coeffs[c] = k:
                      E = sum_i A_i k_i Y_i(x, y, z), A = pi, 2 pi / 3, pi / 4 for l = 0, 1, 2:
                                                      max(E, 0) * a / pi

then alpha appended unshaded and the mean over each aa x aa block.

SHLight (not in the reference): an environment given by spherical-harmonic coefficients `coeffs` [3, n], n in {1, 4, 9} (rows
r, g, b; columns in SH_reconstruct's order i = l * l + l + m; missing columns are zeros), turned into diffuse irradiance at the
shading normal.  The basis and the directions are those of `SH_reconstruct` and of an `EnvironmentMap` with identity
env_to_world -- the texel of the reconstructed map at (theta, phi) lies in world direction
(sin phi sin theta, cos theta, -cos phi sin theta) -- so the same coefficients light the deferred pass and the path tracer alike:

    Y0 =  0.2820948         Y1 = -0.4886025 y        Y2 =  0.4886025 z               Y3 = -0.4886025 x
    Y4 =  1.0925484 x y     Y5 = -1.0925484 y z      Y6 =  0.3153916 (3 z z - 1)     Y7 = -1.0925484 x z
    Y8 =  0.5462742 (x x - y y)

The normal is used as stored; the position takes no part.  The clamp at 0 (an order-2 expansion rings negative) passes half the
gradient at E == 0 exactly, so all-zero coefficients receive a gradient.  There is no rotation of the SH frame: rotate the
coefficients or the normals.  In the light table an SHLight is three rows, one per colour channel.

Shadows (`render_deferred(..., shadows=True)`, `deferred_shade(..., occluders=...)`; not in the reference): every texel casts one
any-hit shadow ray per point, spot and directional light over the scene's triangles, on the path tracer's traversal kernels and
with its 1e-3 offsets; a blocked light adds nothing to the texel.  Shadows are hard, and visibility is a constant of the gradient.
Ambient lights and SHLights cast no shadow ray: occluders dim them through ambient occlusion only (below).  A shadowed image may have at most 32 rows in the
light table: one per light, three per SHLight.

Ambient occlusion (`render_deferred(..., ambient_occlusion=K, ao_radius=r)`, `deferred_shade(..., ambient_occlusion=K)`; not in
the reference): how occluders dim an AmbientLight and an SHLight.  Every texel casts K any-hit rays (1 .. 32),
cosine-distributed about its shading normal, that end after `ao_radius`; the fraction o that escapes multiplies what the ambient
lights and SHLights add to the texel.  Point, directional and spot lights are untouched -- shadows are their business -- and the
two features are independent.  The directions are a fixed table (a radical-inverse spiral, rotated by the texel's place in a
4 x 4 tile; include/redner_amd.h states the rule), so two calls give the same bits.  Occlusion, like visibility, is a constant of
the gradient: the backward call reads the saved words and traces nothing.  The limit of 32 rows does not apply to it.

Specular highlights (`render_deferred(..., specular=True)`, `deferred_specular(g_buffer, material, lights, eye)`; not in the
reference, whose deferred pass is Lambertian): the specular half of the path tracer's own BSDF -- Blinn-Phong distribution, Smith
shadowing, Schlick Fresnel; one-sided -- under the point, spot and directional lights, as ONE native kernel and its adjoint
(`rdr_deferred_specular`, csrc/deferred_specular.h).  Per texel with specular reflectance ks, roughness rho and the eye of its image:

    nh = n / |n|,  v = (eye - p) / |eye - p|,  cv = nh.v              nothing unless n != 0 and cv > 0
    per light:  l and E = I / d.d (point),  I * pow(max(l.s, 0), e) (spot),  I (directional);   cl = nh.l, nothing unless cl > 1e-3
    m = (v + l) / |v + l|,  cm = nh.m                                 nothing unless cm > 0
    r = max(rho, 1e-3),  e = max(2 / r - 2, 0),  D = pow(cm, e) * (e + 2) / (2 pi)
    G = G1(cv) * G1(cl), Smith's rational fit at a = 1 / (sqrt(r) * tan)
    F = k + (1 - k) * pow(max(1 - |m.l|, 0), 5),  k = max(ks, 0)
    E * F * D * G / (4 cv)

so a PointLight gives the path tracer's direct specular term for a point source.  Ambient lights and SHLights cast no highlight.
Every clamp and the roughness floor pass half the gradient at the tie; the conditions and the visibility bits are constants.

Quad lights (`QuadLight(vertices, intensity)`, `quad_light(position, look_at, size, intensity)`, `deferred_quad(g_buffer, lights)`;
not in the reference, whose deferred lights have no area): a rectangular emitter of uniform radiance L, the deferred counterpart
of the path tracer's `AreaLight` on a quad, as ONE native kernel and its adjoint (`rdr_deferred_quad`, csrc/deferred_quad.h).  The
diffuse irradiance of a polygon has a closed form -- Lambert's contour integral, clipped to the texel's horizon -- so the light
is exact and free of noise.  Per texel, with the corners q0..q3 in perimeter order (the emitting side is that of
cross(q1 - q0, q3 - q0)):

    nh = n / |n|,  r_i = q_i - p,  h_i = nh.r_i                       nothing unless n != 0
    S = sum over the edges r_i -> r_i+1, each clipped to h > 0 (an end below is replaced by the crossing point x), of
        edge(A, B) = atan2(|c|, A.B) * (c.nh) / |c|,  c = B x A,      + edge(exit, entry) when the horizon cut the quad
    F = max(S, 0) / 2  (two_sided: |S| / 2)
    L * (a / pi) * F

F / pi is the view factor; a quad that fills the hemisphere gives L * a.  The normal is normalised (the point light uses it as
stored).  Gradients reach p, n, a, the four corners and L; max(S, 0) passes half the gradient at S == 0, |S| passes sign(S), the
conditions are constants.  A QuadLight never enters the ten-float light table: `render_deferred` shades the table lights as before
and adds `deferred_quad` of the quads.  NOT done: quad lights are not shadowed by `shadows=True` (and do
not count towards its 32 rows; soft shadows are below), are not dimmed by ambient occlusion and cast no specular highlight; the
emitter's own surface, where it is in the G-buffer, is shaded like any other surface.

Soft shadows of the quad lights (`render_deferred(..., quad_shadow_rays=K)`, `deferred_quad(..., occluders=..., shadow_rays=K)`;
`rdr_deferred_quad_shadowed`, csrc/deferred_quad_shadow.h): the ratio estimator of Heitz et al. 2018.  Per texel and quad, K points
(1 .. 32) of the quad from a fixed table -- stratified in u, a radical inverse in v, jittered by the texel's place in a 4 x 4 block
-- each with the weight of the unshadowed integrand and one any-hit ray over the occluder scene, with the shadow rays' offsets:

    s = q0 + u (q1 - q0) + v (q3 - q0) + u v ((q2 - q1) - (q3 - q0)),  J the patch's area element at (u, v),  d = s - p
    w = (d.nh) (-d.J) / (d.d)^2  (two_sided: |d.J|)                    the sample counts where d.nh > 0, the quad faces the texel
    V = sum of w over the counting samples whose ray is not blocked / sum of w over the counting samples;  1 without any
    L * (a / pi) * F * V

F stays exact, so a penumbra carries no noise from the form factor, and where nothing is in the way V == 1 and the bits are the
unshadowed call's.  V is a constant of the gradient: the backward call reads the saved factors and traces nothing.  The estimator
is biased, and its fixed point set has an error that does not average out over a frame (DESIGN.md section 7 has the measurement).
csrc/deferred_quad_shadow_abi.h states the rule in the order of the fp32 operations.
"""
import random
from typing import List, Optional, Union

import torch

from . import redner as _default_backend
from ._op import first_order_only, place, ptr, upstream
from .render_pytorch import RenderFunction, Scene

_LIGHT_PARAMS = 10          # csrc/deferred.h: intensity 3, position 3, direction 3, spot exponent 1


class DeferredLight:
    """A light of the deferred pass: a plain holder of tensors (any device; they may require grad)."""
    light_type = None

    def _pieces(self):
        """-> (intensity, position | None, direction | None, exponent | None)"""
        raise NotImplementedError

    def render(self, position: torch.Tensor, normal: torch.Tensor, albedo: torch.Tensor):
        """This light alone on explicit position / normal / albedo images ([..., 3] each, broadcast against each other),
        through the same native kernel as render_deferred."""
        position, normal, albedo = torch.broadcast_tensors(position, normal, albedo)
        shape = position.shape
        if len(shape) < 1 or shape[-1] != 3:
            raise RuntimeError('DeferredLight.render: position, normal and albedo must be [..., 3]')
        g = torch.cat([position, normal, albedo], dim=-1).to(torch.float32)
        g = g.reshape(1, 1, -1, 9) if g.dim() < 3 else g.reshape((-1,) + tuple(g.shape[-3:]))
        img = deferred_shade(g, [self], alpha=False, aa_samples=1)
        return img.reshape(shape)


class AmbientLight(DeferredLight):
    light_type = _default_backend.DeferredLightType.ambient

    def __init__(self, intensity: torch.Tensor):
        self.intensity = intensity

    def _pieces(self):
        return self.intensity, None, None, None


class PointLight(DeferredLight):
    """Point light with squared-distance falloff."""
    light_type = _default_backend.DeferredLightType.point

    def __init__(self, position: torch.Tensor, intensity: torch.Tensor):
        self.position, self.intensity = position, intensity

    def _pieces(self):
        return self.intensity, self.position, None, None


class DirectionalLight(DeferredLight):
    light_type = _default_backend.DeferredLightType.directional

    def __init__(self, direction: torch.Tensor, intensity: torch.Tensor):
        self.direction, self.intensity = direction, intensity

    def _pieces(self):
        return self.intensity, None, self.direction, None


class SpotLight(DeferredLight):
    """Spot light with cosine-power falloff and no distance falloff (no cutoff: it would not be differentiable)."""
    light_type = _default_backend.DeferredLightType.spot

    def __init__(self, position: torch.Tensor, spot_direction: torch.Tensor, spot_exponent: torch.Tensor,
                 intensity: torch.Tensor):
        self.position, self.spot_direction = position, spot_direction
        self.spot_exponent, self.intensity = spot_exponent, intensity

    def _pieces(self):
        return self.intensity, self.position, self.spot_direction, self.spot_exponent


class SHLight(DeferredLight):
    """A spherical-harmonic environment light (not in the reference): `coeffs` [3, n], n in {1, 4, 9} -- rows r, g, b, columns in
    SH_reconstruct's order, missing columns zeros -- lights every texel by the diffuse irradiance at its shading normal (the
    module docstring has the formula).  Three rows of the light table, one per colour channel; it casts no shadow."""
    light_type = _default_backend.DeferredLightType.sh_r          # the first of its rows; the others follow in r, g, b order
    num_rows = 3
    _ROW_TYPES = tuple(int(_default_backend.DeferredLightType[n]) for n in ('sh_r', 'sh_g', 'sh_b'))

    def __init__(self, coeffs: torch.Tensor):
        self.coeffs = coeffs
        self._checked()

    def _checked(self):
        c = torch.as_tensor(self.coeffs)
        if c.dim() != 2 or c.shape[0] != 3 or c.shape[1] not in (1, 4, 9):
            raise RuntimeError('SHLight: coeffs must be [3, n] with n in (1, 4, 9), got %s' % (tuple(c.shape),))
        return c


_QUAD_FLOATS = 16          # csrc/deferred_quad.h: corners 12, radiance 3, one unused


class QuadLight(DeferredLight):
    """A rectangular area light of uniform radiance (not in the reference's deferred pass): `vertices` [4, 3], the corners in
    perimeter order, `intensity` [3], the radiance.  It emits on the side of cross(v1 - v0, v3 - v0), or on both with
    `two_sided`; the quad is expected to be planar and convex.  Every texel gets the exact diffuse irradiance of the part above
    its horizon (the module docstring has the formula).  It is shaded by `deferred_quad` (`render_deferred` does so for the
    QuadLights in its list) and never enters the light table: it is not shadowed by `shadows=True` (softly by
    `quad_shadow_rays=K` / `deferred_quad(occluders=..., shadow_rays=K)`), is not dimmed by ambient occlusion and casts no
    specular highlight."""
    light_type = None

    def __init__(self, vertices: torch.Tensor, intensity: torch.Tensor, two_sided: bool = False):
        self.vertices, self.intensity, self.two_sided = vertices, intensity, bool(two_sided)
        self._checked()

    def _checked(self):
        v, i = torch.as_tensor(self.vertices), torch.as_tensor(self.intensity)
        if tuple(v.shape) != (4, 3):
            raise RuntimeError('QuadLight: vertices must be [4, 3] (the corners in perimeter order), got %s' % (tuple(v.shape),))
        if i.numel() != 3:
            raise RuntimeError('QuadLight: intensity must be [3] (the radiance), got %s' % (tuple(i.shape),))
        return v, i

    def render(self, position: torch.Tensor, normal: torch.Tensor, albedo: torch.Tensor):
        """This light alone on explicit position / normal / albedo images ([..., 3] each, broadcast against each other),
        through the same native kernel as render_deferred."""
        position, normal, albedo = torch.broadcast_tensors(position, normal, albedo)
        shape = position.shape
        if len(shape) < 1 or shape[-1] != 3:
            raise RuntimeError('QuadLight.render: position, normal and albedo must be [..., 3]')
        g = torch.cat([position, normal, albedo], dim=-1).to(torch.float32)
        g = g.reshape(1, 1, -1, 9) if g.dim() < 3 else g.reshape((-1,) + tuple(g.shape[-3:]))
        return deferred_quad(g, [self], alpha=False, aa_samples=1).reshape(shape)


def quad_light(position: torch.Tensor, look_at: torch.Tensor, size: torch.Tensor, intensity: torch.Tensor,
               two_sided: bool = False):
    """The QuadLight that coincides with the emitter of the reference's `generate_quad_light(position, look_at, size, intensity)`:
    a rectangle of `size` [2] centred at `position`, emitting towards `look_at`, in the same in-plane frame.  With
    d = normalize(look_at - position), a = 1 / (1 + d.z) and b = -d.x d.y a, the frame is x = (1 - d.x d.x a, b, -d.x),
    y = (b, 1 - d.y d.y a, -d.y) (at the pole d.z < -1 + 1e-6: x = (0, -1, 0), y = (-1, 0, 0)), so x cross y = d, and the
    corners are position -+ x size[0] / 2 -+ y size[1] / 2 in the order (-, -), (+, -), (+, +), (-, +): the same four points as
    the emitter's, whose triangles are (0, 1, 3) and (1, 2, 3) of these.  Torch operations: autograd carries the gradients of the
    corners to `position`, `look_at` and `size`."""
    position, look_at, size = (torch.as_tensor(t) for t in (position, look_at, size))
    d = look_at - position
    d = d / torch.norm(d)
    if float(d[2]) < -1 + 1e-6:                # (which branch is taken is a constant of the gradient)
        x, y = d.new_tensor([0.0, -1.0, 0.0]), d.new_tensor([-1.0, 0.0, 0.0])
    else:
        a = 1 / (1 + d[2])
        b = -d[0] * d[1] * a
        x, y = torch.stack([1 - d[0] * d[0] * a, b, -d[0]]), torch.stack([b, 1 - d[1] * d[1] * a, -d[1]])
    ex, ey = x * size[0] * 0.5, y * size[1] * 0.5
    vertices = torch.stack([position - ex - ey, position + ex - ey, position + ex + ey, position - ex + ey])
    return QuadLight(vertices, intensity, two_sided=two_sided)


def _split_quads(lights):
    """a list of lights, or one list per image -> (the same without its QuadLights, the QuadLights in the same shape or None when
    there is none)"""
    if len(lights) > 0 and isinstance(lights[0], (list, tuple)):
        quads = [[light for light in lgts if isinstance(light, QuadLight)] for lgts in lights]
        if not any(quads):
            return lights, None
        return [[light for light in lgts if not isinstance(light, QuadLight)] for lgts in lights], quads
    quads = [light for light in lights if isinstance(light, QuadLight)]
    if not quads:
        return lights, None
    return [light for light in lights if not isinstance(light, QuadLight)], quads


def pack_quads(lights, device):
    """[Q, 16] fp32 table on `device` (layout: csrc/deferred_quad.h) + the Q two_sided flags.  One cat over the lights' tensors:
    autograd routes the table's gradient back to them."""
    pieces, flags = [], []
    unused = torch.zeros(1, dtype=torch.float32, device=device)
    for light in lights:
        if not isinstance(light, QuadLight):
            raise RuntimeError('deferred_quad: %r is not a QuadLight (the other lights are shaded by deferred_shade)' % (light,))
        v, i = light._checked()
        pieces += [v.to(device=device, dtype=torch.float32).reshape(-1), i.to(device=device, dtype=torch.float32).reshape(-1), unused]
        flags.append(int(light.two_sided))
    if not pieces:
        return torch.zeros(0, _QUAD_FLOATS, dtype=torch.float32, device=device), flags
    return torch.cat(pieces).reshape(len(flags), _QUAD_FLOATS), flags


def _quad_table(lights, n, device):
    """one list of QuadLights shared by the n images, or n lists -> (quads [Q, 16], the Q flags, the n row ranges)"""
    if len(lights) > 0 and isinstance(lights[0], (list, tuple)):
        if len(lights) != n:
            raise RuntimeError('deferred_quad: %d light lists for %d images' % (len(lights), n))
        flat, ranges = [], []
        for lgts in lights:
            ranges.append((len(flat), len(flat) + len(lgts)))
            flat.extend(lgts)
    else:
        flat, ranges = list(lights), [(0, len(lights))] * n
    quads, flags = pack_quads(flat, device)
    return quads, flags, ranges


def _num_rows(lights):
    """rows of the light table that a list of lights takes: one per light, three per SHLight"""
    return sum(getattr(light, 'num_rows', 1) for light in lights)


def _check_lights(lights):
    """what can be refused about the lights before anything native runs"""
    for light in lights:
        if isinstance(light, (list, tuple)):
            _check_lights(light)
        elif isinstance(light, (SHLight, QuadLight)):
            light._checked()


def pack_lights(lights, device):
    """[L, 10] fp32 table on `device` (layout: csrc/deferred.h) + the L row types: one row per light, three (r, g, b) per
    SHLight.  One cat over the lights' tensors: autograd routes the table's gradient back to them."""
    sizes = (3, 3, 3, 1)
    pieces, types = [], []
    zeros = {n: torch.zeros(n, dtype=torch.float32, device=device) for n in (1, 3, 6, 9)}
    for light in lights:
        if isinstance(light, QuadLight):
            raise RuntimeError('render_deferred: a QuadLight has no row in the light table of deferred_shade and deferred_specular: '
                               'shade it with deferred_quad (render_deferred does so for the QuadLights in its list)')
        if not isinstance(light, DeferredLight) or light.light_type is None:
            raise RuntimeError('render_deferred: %r is not a deferred light' % (light,))
        if isinstance(light, SHLight):
            coeffs = light._checked().to(device=device, dtype=torch.float32)
            for channel, row_type in enumerate(SHLight._ROW_TYPES):       # nine coefficients (n < 9: zeros) + the unused column
                types.append(row_type)
                pieces.append(coeffs[channel])
                pieces.append(zeros[_LIGHT_PARAMS - coeffs.shape[1]])
            continue
        types.append(int(light.light_type))
        for t, n in zip(light._pieces(), sizes):
            if t is None:
                pieces.append(zeros[n])
                continue
            t = torch.as_tensor(t).to(device=device, dtype=torch.float32).reshape(-1)
            if t.numel() != n:
                raise RuntimeError('render_deferred: a parameter of %s has %d elements, expected %d'
                                   % (type(light).__name__, t.numel(), n))
            pieces.append(t)
    if not pieces:
        return torch.zeros(0, _LIGHT_PARAMS, dtype=torch.float32, device=device), types
    return torch.cat(pieces).reshape(len(types), _LIGHT_PARAMS), types


def _light_table(lights, n, device):
    """one list of lights shared by the n images, or n lists -> (params [L, 10], the L row types, the n row ranges)"""
    per_image = len(lights) > 0 and isinstance(lights[0], (list, tuple))
    if per_image:
        if len(lights) != n:
            raise RuntimeError('render_deferred: %d light lists for %d scenes' % (len(lights), n))
        flat, ranges, rows = [], [], 0
        for lgts in lights:                  # ranges are in ROWS of the table
            ranges.append((rows, rows + _num_rows(lgts)))
            rows += _num_rows(lgts)
            flat.extend(lgts)
    else:
        flat, ranges = list(lights), [(0, _num_rows(lights))] * n
    params, types = pack_lights(flat, device)
    return params, types, ranges


def _aligned(t, alpha):
    """contiguous fp32; with alpha the kernels use 8- / 16-byte accesses (a fresh tensor is aligned, an offset view may not be)"""
    t = t.contiguous()
    if alpha and t.data_ptr() % 16 != 0:
        t = t.clone()
    return t


class DeferredShade(torch.autograd.Function):
    """apply(g_buffer [N, H * aa, W * aa, 9 + alpha], light_params [L, 10], light_types, image_light_ranges, aa_samples, alpha,
    backend, occluders, ao_scenes, ao_rays, ao_radius) -> [N, H, W, 3 + alpha].  One native launch forward, one (+ the fold of the
    light gradients) backward.
    `occluders`: None, or N `backend.Scene` (None: that image is not shadowed) -- the shadow rays of the forward call are traced
    over them; the [N, H * aa, W * aa] visibility words are saved for the backward call, which needs no scene.
    `ao_scenes`: None, or N `backend.Scene` (None: that image is not occluded) -- `ao_rays` hemisphere rays per texel, ending after
    `ao_radius`, are traced over them; the [N, H * aa, W * aa] occlusion words follow the image (and the visibility words, when
    there are any) and are saved likewise.
    Gradients reach the G-buffer and the light table, once: under create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, g_buffer, light_params, light_types, image_light_ranges, aa_samples, alpha, backend=None, occluders=None,
                ao_scenes=None, ao_rays=0, ao_radius=float('inf')):
        rd = backend or _default_backend
        light_types = tuple(int(t) for t in light_types)
        image_light_ranges = tuple((int(b), int(e)) for b, e in image_light_ranges)
        aa_samples, alpha = int(aa_samples), bool(alpha)
        channels = 9 + int(alpha)
        if g_buffer.dim() != 4 or g_buffer.shape[3] != channels:
            raise RuntimeError('DeferredShade: the G-buffer must be [N, H * aa, W * aa, %d], got %s'
                               % (channels, tuple(g_buffer.shape)))
        n, hg, wg = int(g_buffer.shape[0]), int(g_buffer.shape[1]), int(g_buffer.shape[2])
        if aa_samples < 1 or hg % aa_samples != 0 or wg % aa_samples != 0 or n == 0 or hg == 0 or wg == 0:
            raise RuntimeError('DeferredShade: a G-buffer of %d x %d x %d does not divide into aa_samples = %d blocks'
                               % (n, hg, wg, aa_samples))
        if tuple(light_params.shape) != (len(light_types), _LIGHT_PARAMS):
            raise RuntimeError('DeferredShade: light_params must be [%d, %d], got %s'
                               % (len(light_types), _LIGHT_PARAMS, tuple(light_params.shape)))
        if len(image_light_ranges) != n:
            raise RuntimeError('DeferredShade: %d light ranges for %d images' % (len(image_light_ranges), n))
        if occluders is not None and len(occluders) != n:
            raise RuntimeError('DeferredShade: %d occluder scenes for %d images' % (len(occluders), n))
        if ao_scenes is not None and len(ao_scenes) != n:
            raise RuntimeError('DeferredShade: %d ao occluder scenes for %d images' % (len(ao_scenes), n))
        if g_buffer.dtype != torch.float32 or light_params.dtype != torch.float32:
            raise RuntimeError('DeferredShade: fp32 tensors only')
        device = g_buffer.device
        use_gpu, index = place(device)
        g = _aligned(g_buffer.detach(), alpha)
        params = light_params.detach().to(device).contiguous()
        h, w = hg // aa_samples, wg // aa_samples
        image = torch.empty(n, h, w, 3 + int(alpha), dtype=torch.float32, device=device)
        geometry = (n, h, w, aa_samples, alpha, light_types, image_light_ranges, use_gpu, index)
        ctx.rd, ctx.geometry, ctx.params_device = rd, geometry, light_params.device
        if occluders is None and ao_scenes is None:
            rd.deferred_shade(ptr(rd, g), ptr(rd, params), ptr(rd, image), *geometry)
            ctx.shadowed, ctx.ao_rays = False, 0
            ctx.save_for_backward(g, params)
            return image
        words, keywords = [], {}                   # the word tensors in the order they are returned and saved
        if occluders is not None:
            words.append(torch.empty(n, hg, wg, dtype=torch.int32, device=device))       # every word is written
            keywords.update(occluders=tuple(occluders), visibility=rd.int_ptr(words[-1].data_ptr()))
        if ao_scenes is not None:
            words.append(torch.empty(n, hg, wg, dtype=torch.int32, device=device))
            keywords.update(ao_occluders=tuple(ao_scenes), ao_words=rd.int_ptr(words[-1].data_ptr()), ao_rays=int(ao_rays),
                            ao_radius=float(ao_radius))
        rd.deferred_shade(ptr(rd, g), ptr(rd, params), ptr(rd, image), *geometry, **keywords)
        ctx.shadowed, ctx.ao_rays = occluders is not None, int(ao_rays) if ao_scenes is not None else 0
        ctx.save_for_backward(g, params, *words)
        ctx.mark_non_differentiable(*words)
        return (image, *words)

    @staticmethod
    def backward(ctx, grad_img, *grad_words):
        first_order_only('DeferredShade')
        rd, geometry = ctx.rd, ctx.geometry
        saved = ctx.saved_tensors
        g, params, words = saved[0], saved[1], list(saved[2:])
        alpha = geometry[4]
        grad_img = _aligned(upstream(grad_img, g.device), alpha)
        assert torch.isfinite(grad_img).all()
        d_g = torch.empty_like(g)
        d_params = torch.empty_like(params)
        keywords = {}
        if ctx.shadowed:
            keywords.update(visibility=rd.int_ptr(words.pop(0).data_ptr()))
        if ctx.ao_rays:
            keywords.update(ao_words=rd.int_ptr(words.pop(0).data_ptr()), ao_rays=ctx.ao_rays)
        rd.deferred_shade_backward(ptr(rd, g), ptr(rd, params), ptr(rd, grad_img), ptr(rd, d_g), ptr(rd, d_params), *geometry,
                                   **keywords)
        return d_g, d_params.to(ctx.params_device), None, None, None, None, None, None, None, None, None


class OccluderScene:
    """What `occluder_scene` returns: the `backend.Scene` whose triangle hierarchy the shadow rays are traced over, together with
    the tensors its handle points into."""

    def __init__(self, scene, keep):
        self.scene, self._keep = scene, keep


def occluder_scene(scene, device: Optional[torch.device] = None, backend=None):
    """The triangles of `scene` as `deferred_shade(occluders=...)` takes them, for users who shade their own G-buffers.  Built as
    a render would build it, without the edge-sampling structures (shadow boundaries are not differentiated); for geometry the
    library has seen before, the topology caches make this a refit or a share."""
    backend = backend or _default_backend
    device = _default_device(device)
    args = RenderFunction.serialize_scene(scene, (1, 1), 0, channels=[backend.channels.position],
                                          sampler_type=backend.SamplerType.sobol, use_primary_edge_sampling=False,
                                          use_secondary_edge_sampling=False, device=device, backend=backend)
    u = RenderFunction.unpack_args((0, 0), args[0], args[1:])
    return OccluderScene(u.scene, (u, args))


def _per_image_scenes(occluders, n, which='occluders'):
    """None, one occluder_scene for all images or a list of N of them (None entries allowed) -> N backend Scenes or None.
    `which`: the argument of deferred_shade they came in by, for the error"""
    if occluders is None or not isinstance(occluders, (list, tuple)):
        occluders = [occluders] * n
    elif len(occluders) != n:
        raise RuntimeError('deferred_shade: %s holds %d occluder scenes for %d images' % (which, len(occluders), n))
    return tuple(o.scene if isinstance(o, OccluderScene) else o for o in occluders)


def deferred_shade(g_buffer, lights, alpha=False, aa_samples=1, backend=None, occluders=None, return_visibility=False,
                   ambient_occlusion=0, ao_radius=float('inf'), ao_occluders=None, return_occlusion=False):
    """Shade a stack of G-buffers [N, H * aa, W * aa, 9 + alpha] in one launch.  `lights`: one list of DeferredLight shared by
    the N images, or N lists.  `occluders`: None (no shadows), one `occluder_scene(...)` for all images, or a list of N of them
    (None: that image is not shadowed); a shadowed image may have at most 32 lights, three per SHLight (they count by their rows
    in the table, although they cast no shadow).  Shadows are hard and are held constant by
    the gradient.  `return_visibility`: also the [N, H * aa, W * aa] int32 words, bit b = light b of the image's list reaches the
    texel (all lights, when there are no occluders).
    `ambient_occlusion`: K in 1 .. 32 hemisphere rays per texel, ending after `ao_radius` (> 0), dim the ambient lights and
    SHLights by the fraction that is blocked; 0: none.  They are traced over `ao_occluders` (given like `occluders`) or, when
    that is None, over `occluders`: pass `ao_occluders=` alone for occlusion without shadows.  `return_occlusion`: also the
    [N, H * aa, W * aa] int32 words, bit r = ray r of the texel escaped.  Results come in the order image, visibility,
    occlusion, each extra only when asked for.  Occlusion is held constant by the gradient."""
    n = int(g_buffer.shape[0])
    params, types, ranges = _light_table(lights, n, g_buffer.device)
    ambient_occlusion = int(ambient_occlusion)
    if ambient_occlusion == 0 and not return_occlusion:
        if occluders is None and not return_visibility:
            return DeferredShade.apply(g_buffer, params, tuple(types), tuple(ranges), aa_samples, alpha, backend)
        scenes = _per_image_scenes(occluders, n)                                          # (`occluders` lives through the call)
        image, visibility = DeferredShade.apply(g_buffer, params, tuple(types), tuple(ranges), aa_samples, alpha, backend, scenes)
        return (image, visibility) if return_visibility else image
    if ambient_occlusion < 0 or ambient_occlusion > 32:
        raise RuntimeError('deferred_shade: ambient_occlusion must be 0 (off) or 1 .. 32 rays per texel, got %d' % ambient_occlusion)
    if ambient_occlusion > 0 and ao_occluders is None and occluders is None:
        raise RuntimeError('deferred_shade: ambient_occlusion needs ao_occluders or occluders to trace its rays over')
    if ambient_occlusion > 0:
        ao_scenes = _per_image_scenes(occluders, n) if ao_occluders is None else _per_image_scenes(ao_occluders, n, 'ao_occluders')
        rays = ambient_occlusion
    else:                                      # only the words were asked for: nothing is occluded, one ray that escapes
        ao_scenes, rays = (None,) * n, 1
    scenes = _per_image_scenes(occluders, n) if occluders is not None or return_visibility else None
    out = DeferredShade.apply(g_buffer, params, tuple(types), tuple(ranges), aa_samples, alpha, backend, scenes, ao_scenes, rays,
                              float(ao_radius))
    results = [out[0]]
    if return_visibility:
        results.append(out[1])
    if return_occlusion:
        results.append(out[-1])
    return tuple(results) if len(results) > 1 else results[0]


class DeferredSpecular(torch.autograd.Function):
    """apply(g_buffer [N, H * aa, W * aa, 9 + alpha], material [N, H * aa, W * aa, 4], eye [N, 3], light_params [L, 10],
    light_types, image_light_ranges, aa_samples, alpha, backend, visibility) -> [N, H, W, 3]: the specular lobe (module
    docstring) of every texel under the lights of its image, averaged over each aa x aa block.  One native launch forward, one
    (+ the fold of the light and eye gradients) backward; gradients reach the position and normal channels of the G-buffer, the
    material, the eye and the lights.  `visibility`: None, or the [N, H * aa, W * aa] int32 words of deferred_shade -- a light
    whose bit is clear adds nothing; the words are held constant by the gradient.  The gradients cannot be differentiated
    again: under create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, g_buffer, material, eye, light_params, light_types, image_light_ranges, aa_samples, alpha, backend=None,
                visibility=None):
        rd = backend or _default_backend
        light_types = tuple(int(t) for t in light_types)
        image_light_ranges = tuple((int(b), int(e)) for b, e in image_light_ranges)
        aa_samples, alpha = int(aa_samples), bool(alpha)
        channels = 9 + int(alpha)
        if g_buffer.dim() != 4 or g_buffer.shape[3] != channels:
            raise RuntimeError('DeferredSpecular: the G-buffer must be [N, H * aa, W * aa, %d], got %s'
                               % (channels, tuple(g_buffer.shape)))
        n, hg, wg = int(g_buffer.shape[0]), int(g_buffer.shape[1]), int(g_buffer.shape[2])
        if aa_samples < 1 or hg % aa_samples != 0 or wg % aa_samples != 0 or n == 0 or hg == 0 or wg == 0:
            raise RuntimeError('DeferredSpecular: a G-buffer of %d x %d x %d does not divide into aa_samples = %d blocks'
                               % (n, hg, wg, aa_samples))
        if tuple(material.shape) != (n, hg, wg, 4):
            raise RuntimeError('DeferredSpecular: the material must be [%d, %d, %d, 4] (specular reflectance 3, roughness 1), got %s'
                               % (n, hg, wg, tuple(material.shape)))
        if tuple(eye.shape) != (n, 3):
            raise RuntimeError('DeferredSpecular: eye must be [%d, 3], got %s' % (n, tuple(eye.shape)))
        if tuple(light_params.shape) != (len(light_types), _LIGHT_PARAMS):
            raise RuntimeError('DeferredSpecular: light_params must be [%d, %d], got %s'
                               % (len(light_types), _LIGHT_PARAMS, tuple(light_params.shape)))
        if len(image_light_ranges) != n:
            raise RuntimeError('DeferredSpecular: %d light ranges for %d images' % (len(image_light_ranges), n))
        if any(t.dtype != torch.float32 for t in (g_buffer, material, eye, light_params)):
            raise RuntimeError('DeferredSpecular: fp32 tensors only')
        device = g_buffer.device
        if material.device != device:
            raise RuntimeError('DeferredSpecular: the material is on %s, the G-buffer on %s' % (material.device, device))
        if visibility is not None:
            if tuple(visibility.shape) != (n, hg, wg) or visibility.dtype != torch.int32 or visibility.device != device:
                raise RuntimeError('DeferredSpecular: visibility must be [%d, %d, %d] int32 on %s' % (n, hg, wg, device))
            visibility = visibility.detach().contiguous()
        use_gpu, index = place(device)
        g = _aligned(g_buffer.detach(), True)                  # (16 bytes serve both widths)
        mat = _aligned(material.detach(), True)
        eyes = eye.detach().to(device).contiguous()
        params = light_params.detach().to(device).contiguous()
        h, w = hg // aa_samples, wg // aa_samples
        image = torch.empty(n, h, w, 3, dtype=torch.float32, device=device)
        geometry = (n, h, w, aa_samples, alpha, light_types, image_light_ranges, use_gpu, index)
        ctx.rd, ctx.geometry, ctx.devices = rd, geometry, (eye.device, light_params.device)
        words = None if visibility is None else rd.int_ptr(visibility.data_ptr())
        rd.deferred_specular(ptr(rd, g), ptr(rd, mat), ptr(rd, eyes), ptr(rd, params), ptr(rd, image), *geometry, visibility=words)
        ctx.shadowed = visibility is not None
        ctx.save_for_backward(g, mat, eyes, params, *(() if visibility is None else (visibility,)))
        return image

    @staticmethod
    def backward(ctx, grad_img):
        first_order_only('DeferredSpecular')
        rd, geometry = ctx.rd, ctx.geometry
        saved = ctx.saved_tensors
        g, mat, eyes, params = saved[:4]
        grad_img = upstream(grad_img, g.device)
        assert torch.isfinite(grad_img).all()
        d_g, d_mat, d_eye, d_params = (torch.empty_like(t) for t in (g, mat, eyes, params))
        words = rd.int_ptr(saved[4].data_ptr()) if ctx.shadowed else None
        rd.deferred_specular_backward(ptr(rd, g), ptr(rd, mat), ptr(rd, eyes), ptr(rd, params), ptr(rd, grad_img), ptr(rd, d_g),
                                      ptr(rd, d_mat), ptr(rd, d_eye), ptr(rd, d_params), *geometry, visibility=words)
        return d_g, d_mat, d_eye.to(ctx.devices[0]), d_params.to(ctx.devices[1]), None, None, None, None, None, None


def deferred_specular(g_buffer, material, lights, eye, alpha=False, aa_samples=1, visibility=None, backend=None):
    """The specular highlights of a stack of G-buffers [N, H * aa, W * aa, 9 + alpha] -> [N, H, W, 3], to be added to the colour
    channels of `deferred_shade`'s image.  `material` [N, H * aa, W * aa, 4]: specular reflectance rgb, then roughness (the
    `specular_reflectance` and `roughness` channels of `render_g_buffer`); `eye` [N, 3] (or [3] for all images): where the camera
    stands; `lights` as for `deferred_shade` -- point, spot and directional lights cast a highlight, ambient lights and SHLights
    none.  `visibility`: the words `deferred_shade(..., return_visibility=True)` gave: a light that is blocked casts no highlight."""
    n = int(g_buffer.shape[0])
    params, types, ranges = _light_table(lights, n, g_buffer.device)
    eye = torch.as_tensor(eye)
    if eye.dim() == 1:
        eye = eye.reshape(1, -1).expand(n, -1)
    return DeferredSpecular.apply(g_buffer, material, eye, params, tuple(types), tuple(ranges), aa_samples, alpha, backend,
                                  visibility)


class DeferredQuad(torch.autograd.Function):
    """apply(g_buffer [N, H * aa, W * aa, 9 + alpha], quads [Q, 16], two_sided, image_quad_ranges, aa_samples, alpha, backend)
    -> [N, H, W, 3]: the light of the quads of its image (module docstring) on every texel, averaged over each aa x aa block.
    `quads`: a row is the corners q0..q3, the radiance and one unused float; `two_sided`: Q flags, 0 or 1;
    `image_quad_ranges`: N (begin, end) pairs into the rows.  One native launch forward, one (+ the fold of the quad gradients)
    backward; gradients reach the nine channels of the G-buffer and the table.  The gradients cannot be differentiated again:
    under create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, g_buffer, quads, two_sided, image_quad_ranges, aa_samples, alpha, backend=None):
        rd = backend or _default_backend
        two_sided = tuple(int(t) for t in two_sided)
        image_quad_ranges = tuple((int(b), int(e)) for b, e in image_quad_ranges)
        aa_samples, alpha = int(aa_samples), bool(alpha)
        channels = 9 + int(alpha)
        if g_buffer.dim() != 4 or g_buffer.shape[3] != channels:
            raise RuntimeError('DeferredQuad: the G-buffer must be [N, H * aa, W * aa, %d], got %s'
                               % (channels, tuple(g_buffer.shape)))
        n, hg, wg = int(g_buffer.shape[0]), int(g_buffer.shape[1]), int(g_buffer.shape[2])
        if aa_samples < 1 or hg % aa_samples != 0 or wg % aa_samples != 0 or n == 0 or hg == 0 or wg == 0:
            raise RuntimeError('DeferredQuad: a G-buffer of %d x %d x %d does not divide into aa_samples = %d blocks'
                               % (n, hg, wg, aa_samples))
        if tuple(quads.shape) != (len(two_sided), _QUAD_FLOATS):
            raise RuntimeError('DeferredQuad: quads must be [%d, %d], got %s' % (len(two_sided), _QUAD_FLOATS, tuple(quads.shape)))
        if len(image_quad_ranges) != n:
            raise RuntimeError('DeferredQuad: %d quad ranges for %d images' % (len(image_quad_ranges), n))
        if g_buffer.dtype != torch.float32 or quads.dtype != torch.float32:
            raise RuntimeError('DeferredQuad: fp32 tensors only')
        device = g_buffer.device
        use_gpu, index = place(device)
        g = _aligned(g_buffer.detach(), alpha)
        table = quads.detach().to(device).contiguous()
        h, w = hg // aa_samples, wg // aa_samples
        image = torch.empty(n, h, w, 3, dtype=torch.float32, device=device)
        geometry = (n, h, w, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu, index)
        ctx.rd, ctx.geometry, ctx.quads_device = rd, geometry, quads.device
        rd.deferred_quad(ptr(rd, g), ptr(rd, table), ptr(rd, image), *geometry)
        ctx.save_for_backward(g, table)
        return image

    @staticmethod
    def backward(ctx, grad_img):
        first_order_only('DeferredQuad')
        rd, geometry = ctx.rd, ctx.geometry
        g, table = ctx.saved_tensors
        grad_img = upstream(grad_img, g.device)
        assert torch.isfinite(grad_img).all()
        d_g, d_table = torch.empty_like(g), torch.empty_like(table)
        rd.deferred_quad_backward(ptr(rd, g), ptr(rd, table), ptr(rd, grad_img), ptr(rd, d_g), ptr(rd, d_table), *geometry)
        return d_g, d_table.to(ctx.quads_device), None, None, None, None, None


class DeferredQuadShadowed(torch.autograd.Function):
    """apply(g_buffer, quads, two_sided, image_quad_ranges, aa_samples, alpha, backend, occluders, shadow_rays[, factors])
    -> (image [N, H, W, 3], words [P, H * aa, W * aa] int32, factors [P, H * aa, W * aa] fp32): DeferredQuad with soft shadows.
    `occluders`: N `backend.Scene` (None: that image is not shadowed); `shadow_rays`: K in 1 .. 32 any-hit rays per texel and
    quad towards fixed stratified points of the quad.  Each (quad, texel) term is multiplied by the factor
    V = sum_k w_k vis_k / sum_k w_k (the module docstring; csrc/deferred_quad_shadow_abi.h has the rule); P is the sum of the
    images' range lengths, and the pair of quad l of image n is (the earlier images' lengths) + l - begin_n.  Bit k of a word:
    sample k does not count or its ray was not blocked.  `factors` (optional): the [P, H * aa, W * aa] fp32 tensor the factors
    are written into.  The factors are saved for the backward call, which traces nothing and holds them constant; words and
    factors carry no gradient.  Under create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, g_buffer, quads, two_sided, image_quad_ranges, aa_samples, alpha, backend=None, occluders=None,
                shadow_rays=0, factors=None):
        rd = backend or _default_backend
        two_sided = tuple(int(t) for t in two_sided)
        image_quad_ranges = tuple((int(b), int(e)) for b, e in image_quad_ranges)
        aa_samples, alpha, shadow_rays = int(aa_samples), bool(alpha), int(shadow_rays)
        channels = 9 + int(alpha)
        if g_buffer.dim() != 4 or g_buffer.shape[3] != channels:
            raise RuntimeError('DeferredQuadShadowed: the G-buffer must be [N, H * aa, W * aa, %d], got %s'
                               % (channels, tuple(g_buffer.shape)))
        n, hg, wg = int(g_buffer.shape[0]), int(g_buffer.shape[1]), int(g_buffer.shape[2])
        if aa_samples < 1 or hg % aa_samples != 0 or wg % aa_samples != 0 or n == 0 or hg == 0 or wg == 0:
            raise RuntimeError('DeferredQuadShadowed: a G-buffer of %d x %d x %d does not divide into aa_samples = %d blocks'
                               % (n, hg, wg, aa_samples))
        if tuple(quads.shape) != (len(two_sided), _QUAD_FLOATS):
            raise RuntimeError('DeferredQuadShadowed: quads must be [%d, %d], got %s'
                               % (len(two_sided), _QUAD_FLOATS, tuple(quads.shape)))
        if len(image_quad_ranges) != n:
            raise RuntimeError('DeferredQuadShadowed: %d quad ranges for %d images' % (len(image_quad_ranges), n))
        if g_buffer.dtype != torch.float32 or quads.dtype != torch.float32:
            raise RuntimeError('DeferredQuadShadowed: fp32 tensors only')
        if occluders is None or len(occluders) != n:
            raise RuntimeError('DeferredQuadShadowed: occluders must be %d scenes (None: that image is not shadowed), got %s'
                               % (n, 'None' if occluders is None else '%d' % len(occluders)))
        if shadow_rays < 1 or shadow_rays > 32:
            raise RuntimeError('DeferredQuadShadowed: shadow_rays must be 1 .. 32, got %d' % shadow_rays)
        device = g_buffer.device
        pairs = sum(max(e - b, 0) for b, e in image_quad_ranges)
        if factors is not None and (tuple(factors.shape) != (pairs, hg, wg) or factors.dtype != torch.float32 or
                                    factors.device != device or not factors.is_contiguous()):
            raise RuntimeError('DeferredQuadShadowed: factors must be a contiguous [%d, %d, %d] fp32 tensor on %s, got %s'
                               % (pairs, hg, wg, device, tuple(factors.shape)))
        use_gpu, index = place(device)
        g = _aligned(g_buffer.detach(), alpha)
        table = quads.detach().to(device).contiguous()
        h, w = hg // aa_samples, wg // aa_samples
        image = torch.empty(n, h, w, 3, dtype=torch.float32, device=device)
        words = torch.empty(pairs, hg, wg, dtype=torch.int32, device=device)           # every word and factor is written
        if factors is None:
            factors = torch.empty(pairs, hg, wg, dtype=torch.float32, device=device)
        # (a call without a pair still hands the library two buffers it can name: four bytes each, of which nothing is returned)
        spare = torch.empty(2, dtype=torch.int32, device=device) if pairs == 0 else None
        geometry = (n, h, w, aa_samples, alpha, two_sided, image_quad_ranges, use_gpu, index)
        ctx.rd, ctx.geometry, ctx.quads_device = rd, geometry, quads.device
        rd.deferred_quad_shadowed(ptr(rd, g), ptr(rd, table), rd.float_ptr((factors if spare is None else spare[1:]).data_ptr()),
                                  ptr(rd, image), *geometry, occluders=tuple(occluders),
                                  visibility=rd.int_ptr((words if spare is None else spare).data_ptr()), shadow_rays=shadow_rays)
        ctx.save_for_backward(g, table, factors)
        ctx.mark_non_differentiable(words, factors)
        return image, words, factors

    @staticmethod
    def backward(ctx, grad_img, grad_words, grad_factors):
        first_order_only('DeferredQuadShadowed')
        rd, geometry = ctx.rd, ctx.geometry
        g, table, factors = ctx.saved_tensors
        grad_img = upstream(grad_img, g.device)
        assert torch.isfinite(grad_img).all()
        d_g, d_table = torch.empty_like(g), torch.empty_like(table)
        if factors.shape[0] == 0:              # (no pair: as in forward)
            factors = torch.ones(1, dtype=torch.float32, device=g.device)
        rd.deferred_quad_shadowed_backward(ptr(rd, g), ptr(rd, table), ptr(rd, factors), ptr(rd, grad_img), ptr(rd, d_g),
                                           ptr(rd, d_table), *geometry)
        return d_g, d_table.to(ctx.quads_device), None, None, None, None, None, None, None, None


def deferred_quad(g_buffer, lights, alpha=False, aa_samples=1, backend=None, occluders=None, shadow_rays=0,
                  return_visibility=False):
    """The light of QuadLights on a stack of G-buffers [N, H * aa, W * aa, 9 + alpha] -> [N, H, W, 3], to be added to the colour
    channels of `deferred_shade`'s image.  `lights`: one list of QuadLight shared by the N images, or N lists (an empty one is
    fine).  The lights are exact area emitters (the module docstring has the formula and what is left out);
    gradients reach position, normal and albedo, and the corners and radiance of every QuadLight -- through `quad_light`, its
    position, look_at and size.
    Soft shadows: `occluders`, one `occluder_scene(...)` for all images or a list of N of them (None: that image is not
    shadowed), together with `shadow_rays`, K in 1 .. 32 any-hit rays per texel and quad; each quad's light on a texel is
    multiplied by the weighted fraction of K fixed points of the quad that the texel sees.  One without the other raises.  The
    factors are held constant by the gradient.  `return_visibility`: also (words, factors), [P, H * aa, W * aa] int32 and fp32,
    one plane per (image, quad) pair in the order of the images and of each image's list.  With the defaults: the launches and
    the bits of the call without these arguments."""
    n = int(g_buffer.shape[0])
    shadow_rays = int(shadow_rays)
    if occluders is None and shadow_rays == 0 and not return_visibility:
        quads, flags, ranges = _quad_table(lights, n, g_buffer.device)
        return DeferredQuad.apply(g_buffer, quads, tuple(flags), tuple(ranges), aa_samples, alpha, backend)
    if occluders is None:
        raise RuntimeError('deferred_quad: shadow_rays = %d (or return_visibility) needs occluders to trace the rays over'
                           % shadow_rays)
    if shadow_rays < 1 or shadow_rays > 32:
        raise RuntimeError('deferred_quad: with occluders, shadow_rays must be 1 .. 32 rays per texel and quad, got %d' % shadow_rays)
    quads, flags, ranges = _quad_table(lights, n, g_buffer.device)
    scenes = _per_image_scenes(occluders, n)                                              # (`occluders` lives through the call)
    image, words, factors = DeferredQuadShadowed.apply(g_buffer, quads, tuple(flags), tuple(ranges), aa_samples, alpha, backend,
                                                       scenes, shadow_rays)
    return (image, (words, factors)) if return_visibility else image


def _default_device(device):
    if device is not None:
        return device
    return torch.device('cuda:%d' % torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


def _random_seed():
    return random.randint(0, 16777216)


def _seeds_for(scenes, seed):
    if seed is None:
        return [_random_seed() for _ in scenes]
    if len(seed) != len(scenes):
        raise RuntimeError('a batch of %d scenes needs a list of %d seeds' % (len(scenes), len(seed)))
    return list(seed)


def _render_g_buffer_for_deferred(scene, seed, channels, aa_samples, sample_pixel_center, use_primary_edge_sampling, device,
                                  backend):
    """The scene at aa_samples times its resolution and viewport; both are restored whatever happens."""
    camera = scene.camera
    resolution, viewport = camera.resolution, camera.viewport
    try:
        camera.resolution = (resolution[0] * aa_samples, resolution[1] * aa_samples)
        if viewport is not None:
            camera.viewport = [v * aa_samples for v in viewport]
        args = RenderFunction.serialize_scene(scene, (1, 1), 0, channels=channels, sampler_type=backend.SamplerType.sobol,
                                              use_primary_edge_sampling=use_primary_edge_sampling,
                                              use_secondary_edge_sampling=False, sample_pixel_center=sample_pixel_center,
                                              device=device, backend=backend)
    finally:
        camera.resolution, camera.viewport = resolution, viewport
    return RenderFunction.apply(seed, *args)


def _eye_of(camera, backend):
    """where a camera stands, as a tensor a gradient can reach: its position or, for one given by cam_to_world, the translation
    column; an orthographic camera has no eye point"""
    if int(camera.camera_type) == int(backend.CameraType.orthographic):
        raise RuntimeError('render_deferred: specular=True needs an eye point, which an orthographic camera does not have')
    if camera.cam_to_world is not None:
        return camera.cam_to_world[:3, 3]
    return torch.as_tensor(camera.position).reshape(3)


def _add_quads(images, g_buffer, quad_lights, alpha, aa_samples, backend, occluders=None, shadow_rays=0):
    """images + deferred_quad of the QuadLights on the same G-buffer (softly shadowed by `occluders` when `shadow_rays` > 0); the
    alpha channel is left as it is"""
    if shadow_rays:
        light = deferred_quad(g_buffer, quad_lights, alpha=alpha, aa_samples=aa_samples, backend=backend, occluders=occluders,
                              shadow_rays=shadow_rays)
    else:
        light = deferred_quad(g_buffer, quad_lights, alpha=alpha, aa_samples=aa_samples, backend=backend)
    if alpha:
        light = torch.cat([light, torch.zeros_like(light[..., :1])], dim=-1)
    return images + light


def render_deferred(scene: Union[Scene, List[Scene]], lights, alpha: bool = False, aa_samples: int = 2, seed=None,
                    sample_pixel_center: bool = False, use_primary_edge_sampling: bool = True,
                    device: Optional[torch.device] = None, backend=None, shadows: bool = False, ambient_occlusion: int = 0,
                    ao_radius: float = float('inf'), specular: bool = False, quad_shadow_rays: int = 0):
    """Deferred rendering: Lambertian shading of the G-buffer by `lights` and, with `specular`, the specular lobe on top.

    scene: a Scene -> [H, W, 3 | 4]; a list of N scenes of one resolution -> [N, H, W, 3 | 4], shaded in one launch.
    lights: a list of DeferredLight (shared by all scenes of a batch) or, for a batch, one list per scene.
    seed: an int (a list of N ints for a batch); random when None.
    `backend` (redner_amd extension): the module providing the `redner` API, as for RenderFunction.serialize_scene.
    `shadows` (redner_amd extension; the reference's render_deferred has none): every texel casts one any-hit shadow ray per
    point, spot and directional light over the triangles of its scene, with the path tracer's offsets (the ray starts 1e-3 along
    its direction and, for a light with a position, ends at (1 - 1e-3) of the distance); a light that is blocked adds nothing.
    Shadows are HARD and are not differentiated across their boundary: the gradient holds visibility constant (DESIGN.md
    section 7).  At most 32 lights per scene, three per SHLight; ambient lights and SHLights are not shadowed.
    `ambient_occlusion` (redner_amd extension), independent of `shadows`: K in 1 .. 32 any-hit rays per texel, cosine-distributed
    about the shading normal and ending after `ao_radius`, over the triangles of its scene; the fraction that escapes multiplies
    what the AmbientLights and SHLights add (the other lights are untouched).  Held constant by the gradient, like visibility.
    WARNING: in a closed scene, such as a box around the objects, every unbounded ray is blocked and the ambient lights go
    black: give a finite `ao_radius` there, a fraction of the scene's size.
    `specular` (redner_amd extension): the G-buffer also carries the materials' specular reflectance and roughness, and the
    specular lobe of the path tracer's BSDF under the point, spot and directional lights (`deferred_specular`; the module
    docstring has the formula) is added to the colour channels; with `shadows`, a blocked light casts no highlight.  The eye is
    the camera's position (the translation column of a `cam_to_world`), so an orthographic camera raises.  Gradients reach
    `specular_reflectance`, `roughness`, the geometry, the lights and the camera position.  Ambient occlusion leaves the
    highlights alone.  False: the same launches and the same bits as without the argument.
    QuadLights (redner_amd extension) may stand in `lights` among the others, in a shared list or in per-scene lists: the others
    are shaded exactly as without them, the quads by `deferred_quad` on the same G-buffer, and the sum is returned (alpha is the
    diffuse pass's).  Quad lights are NOT shadowed by `shadows` and do not count towards its 32 rows, are NOT dimmed by
    `ambient_occlusion` and cast NO specular highlight; the emitter's own surface, where the scene holds it, is shaded like any
    other surface.  Without a QuadLight in `lights`: the same launches and the same bits as before there were any.
    `quad_shadow_rays` (redner_amd extension), independent of `shadows`: K in 1 .. 32 any-hit rays per texel and QuadLight over
    the triangles of its scene, towards K fixed stratified points of the quad; the quad's exact light on the texel is multiplied
    by the weighted fraction of the points the texel sees (`deferred_quad(..., occluders=..., shadow_rays=K)`): SOFT shadows
    with a penumbra, whose only error is in that fraction.  The rays end short of the quad, so the emitter's own mesh in the
    scene does not block them.  Held constant by the gradient, like visibility.  The occluder scene is the one `shadows` and
    `ambient_occlusion` use, built once.  0: the same launches and the same bits as without the argument."""
    backend = backend or _default_backend
    device = _default_device(device)
    aa_samples = int(aa_samples)
    if aa_samples < 1:
        raise RuntimeError('render_deferred: aa_samples must be at least 1')
    _check_lights(lights)
    lights, quad_lights = _split_quads(lights)
    channels = [backend.channels.position, backend.channels.shading_normal, backend.channels.diffuse_reflectance]
    if alpha:
        channels.append(backend.channels.alpha)
    single = isinstance(scene, Scene) or not isinstance(scene, (list, tuple))
    scenes = [scene] if single else list(scene)
    if specular:
        channels += [backend.channels.specular_reflectance, backend.channels.roughness]
        eyes = [_eye_of(sc.camera, backend) for sc in scenes]
    seeds = [_random_seed() if seed is None else seed] if single else _seeds_for(scenes, seed)
    g_buffers = [_render_g_buffer_for_deferred(sc, se, channels, aa_samples, sample_pixel_center, use_primary_edge_sampling,
                                               device, backend) for sc, se in zip(scenes, seeds)]
    g_buffer = g_buffers[0].unsqueeze(0) if single else torch.stack(g_buffers)
    # (the occluder scenes live until the shade call has returned)
    ambient_occlusion, quad_shadow_rays = int(ambient_occlusion), int(quad_shadow_rays)
    if quad_shadow_rays < 0 or quad_shadow_rays > 32:
        raise RuntimeError('render_deferred: quad_shadow_rays must be 0 (off) or 1 .. 32 rays per texel and QuadLight, got %d'
                           % quad_shadow_rays)
    quad_rays = quad_shadow_rays if quad_lights is not None else 0
    built = [occluder_scene(sc, device=device, backend=backend) for sc in scenes] if shadows or ambient_occlusion or quad_rays \
        else None
    if not specular:
        images = deferred_shade(g_buffer, lights, alpha=alpha, aa_samples=aa_samples, backend=backend,
                                occluders=built if shadows else None, ambient_occlusion=ambient_occlusion, ao_radius=ao_radius,
                                ao_occluders=built if ambient_occlusion else None)
        if quad_lights is not None:
            images = _add_quads(images, g_buffer, quad_lights, alpha, aa_samples, backend, built, quad_rays)
        return images[0] if single else images
    # the diffuse part exactly as above on its own channels (asking for the words when there are shadows), then the lobe
    diffuse_channels = 9 + int(bool(alpha))
    g, material = g_buffer[..., :diffuse_channels].contiguous(), g_buffer[..., diffuse_channels:].contiguous()      # one copy each
    out = deferred_shade(g, lights, alpha=alpha, aa_samples=aa_samples, backend=backend, occluders=built if shadows else None,
                         return_visibility=bool(shadows), ambient_occlusion=ambient_occlusion, ao_radius=ao_radius,
                         ao_occluders=built if ambient_occlusion else None)
    images, visibility = out if shadows else (out, None)
    eye = torch.stack([e.to(device=device, dtype=torch.float32) for e in eyes])
    highlights = deferred_specular(g, material, lights, eye, alpha=alpha, aa_samples=aa_samples, visibility=visibility,
                                   backend=backend)
    if alpha:
        highlights = torch.cat([highlights, torch.zeros_like(highlights[..., :1])], dim=-1)
    images = images + highlights
    if quad_lights is not None:
        images = _add_quads(images, g, quad_lights, alpha, aa_samples, backend, built, quad_rays)
    return images[0] if single else images


def render_generic(scene, channels: List, max_bounces: int = 1, sampler_type=None, num_samples=(4, 4), seed=None,
                   sample_pixel_center: bool = False, use_primary_edge_sampling: bool = True,
                   use_secondary_edge_sampling: bool = True, device: Optional[torch.device] = None, backend=None):
    """Path tracing, G-buffer channels or both: serialize_scene + RenderFunction.apply; a list of scenes is stacked."""
    backend = backend or _default_backend
    device = _default_device(device)
    if sampler_type is None:
        sampler_type = backend.SamplerType.sobol

    def one(sc, se):
        args = RenderFunction.serialize_scene(sc, num_samples, max_bounces, channels=channels, sampler_type=sampler_type,
                                              use_primary_edge_sampling=use_primary_edge_sampling,
                                              use_secondary_edge_sampling=use_secondary_edge_sampling,
                                              sample_pixel_center=sample_pixel_center, device=device, backend=backend)
        return RenderFunction.apply(se, *args)

    if isinstance(scene, Scene) or not isinstance(scene, (list, tuple)):
        return one(scene, _random_seed() if seed is None else seed)
    scenes = list(scene)
    return torch.stack([one(sc, se) for sc, se in zip(scenes, _seeds_for(scenes, seed))])


def render_g_buffer(scene, channels: List, num_samples=(1, 1), seed=None, sample_pixel_center: bool = False,
                    use_primary_edge_sampling: bool = True, use_secondary_edge_sampling: bool = True,
                    device: Optional[torch.device] = None, backend=None):
    """The given channels without light transport: max_bounces 0, Sobol sampler."""
    backend = backend or _default_backend
    return render_generic(scene, channels, max_bounces=0, sampler_type=backend.SamplerType.sobol, num_samples=num_samples,
                          seed=seed, sample_pixel_center=sample_pixel_center,
                          use_primary_edge_sampling=use_primary_edge_sampling,
                          use_secondary_edge_sampling=use_secondary_edge_sampling, device=device, backend=backend)


def render_pathtracing(scene, alpha: bool = False, max_bounces: int = 1, sampler_type=None, num_samples=(4, 4), seed=None,
                       sample_pixel_center: bool = False, use_primary_edge_sampling: bool = True,
                       use_secondary_edge_sampling: bool = True, device: Optional[torch.device] = None, backend=None):
    """Radiance (and alpha) by path tracing; max_bounces 1 = direct lighting only."""
    backend = backend or _default_backend
    channels = [backend.channels.radiance] + ([backend.channels.alpha] if alpha else [])
    return render_generic(scene, channels, max_bounces=max_bounces, sampler_type=sampler_type, num_samples=num_samples,
                          seed=seed, sample_pixel_center=sample_pixel_center,
                          use_primary_edge_sampling=use_primary_edge_sampling,
                          use_secondary_edge_sampling=use_secondary_edge_sampling, device=device, backend=backend)


def render_albedo(scene, alpha: bool = False, num_samples=(16, 4), seed=None, sample_pixel_center: bool = False,
                  use_primary_edge_sampling: bool = True, device: Optional[torch.device] = None, backend=None):
    """The diffuse reflectance (and alpha) of the first hit."""
    backend = backend or _default_backend
    channels = [backend.channels.diffuse_reflectance] + ([backend.channels.alpha] if alpha else [])
    return render_g_buffer(scene, channels, num_samples=num_samples, seed=seed, sample_pixel_center=sample_pixel_center,
                           use_primary_edge_sampling=use_primary_edge_sampling, device=device, backend=backend)
