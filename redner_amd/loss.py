"""The Gaussian image pyramid loss of the reference's optimisation scripts on the native kernels of csrc/pyramid_loss.h.

    loss = gaussian_pyramid_loss(render(scene), target)         # rdr_pyramid_loss: five levels, one 0-dim fp32 tensor
    loss.backward()                                             # rdr_pyramid_loss_backward, then the renderer's own backward

What the scripts write in torch at every iteration (tests/test_bunny_box.py, tutorials/05_coarse_to_fine_estimation.py, ...):

    D_0 = image - target                                        (clamped to [-clamp, clamp] when `clamp` is given)
    D_{l+1} = AvgPool2d(2)(conv2d(D_l, 7 x 7 Gaussian, padding=3))          zero padding; an odd side drops the last row / column
    loss = sum_l weights[l] * D_l.pow(2).sum() / ((H / 2 ** l) * (W / 2 ** l))

with the 7 x 7 table of scipy.ndimage.gaussian_filter(dirac, 1.0): a (x) a, a = [w3 + w4, w2, w1, w0, w1, w2, w3 + w4],
w_k = exp(-k^2 / 2) / sum_{-4..4}.  csrc/pyramid_loss.h pins the fp32 order of every sum; the sums of squares are fp64 in a fixed
order and rounded once, the gradient is a gather without atomics: loss and gradient are bitwise reproducible from run to run.

A handful of native launches each way instead of about forty torch ones.  There is no torch fall-back: the tensors' memory goes to
the loaded native library.  CPU tensors are accepted by the CPU debugging harness only (the test-suite loads it); the product
library raises for them.
"""
import torch

from . import redner as _default_backend
from ._op import first_order_only, named, place, ptr, scratch, upstream


def _geometry(image):
    shape = tuple(int(v) for v in image.shape)
    return shape if len(shape) == 4 else (1,) + shape


def _forward(rd, image, target, num_levels, clamp, weights):
    """image, target: detached contiguous fp32.  -> loss (0-dim fp32), terms (fp64 [L]), saved (fp64; the levels at its start)"""
    batch, height, width, channels = _geometry(image)
    use_gpu, index = place(image)
    fwd, _ = rd.pyramid_loss_scratch(batch, height, width, channels, num_levels)
    saved = scratch(fwd, image.device)
    loss = torch.empty((), dtype=torch.float32, device=image.device)
    terms = torch.empty(num_levels, dtype=torch.float64, device=image.device)
    rd.pyramid_loss(ptr(rd, image), ptr(rd, target), ptr(rd, loss), terms.data_ptr(), ptr(rd, saved), fwd, batch, height, width,
                    channels, num_levels, weights, clamp or 0.0, use_gpu, index)
    return loss, terms, saved


class GaussianPyramidLoss(torch.autograd.Function):
    """image, target [H, W, C] or [N, H, W, C] fp32 -> (loss, terms): a 0-dim fp32 tensor and the fp64 [num_levels] per-level
    terms (not differentiable), on the inputs' device.  The gradient goes to `image` and, if it asks for one, to `target`; it cannot be
    differentiated again: under create_graph=True the backward call raises."""

    @staticmethod
    def forward(ctx, image, target, num_levels, clamp, weights, backend=None):
        rd = backend or _default_backend
        a, b = image.detach().contiguous(), target.detach().contiguous()
        loss, terms, saved = _forward(rd, a, b, num_levels, clamp, weights)
        ctx.rd, ctx.options = rd, (num_levels, clamp, weights)
        # (for a contiguous input a / b is the caller's own memory: saved this way, an in-place edit before backward raises)
        ctx.save_for_backward(a, b, saved)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, d_loss, _d_terms):
        first_order_only('GaussianPyramidLoss')
        rd = ctx.rd
        a, b, saved = ctx.saved_tensors
        num_levels, clamp, weights = ctx.options
        batch, height, width, channels = _geometry(a)
        use_gpu, index = place(a)
        g = upstream(d_loss, a.device)
        d_image = torch.empty_like(a)
        d_target = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _, bwd = rd.pyramid_loss_scratch(batch, height, width, channels, num_levels)
        work = scratch(bwd, a.device)
        rd.pyramid_loss_backward(ptr(rd, a), ptr(rd, b), ptr(rd, saved), 2 * saved.numel(), ptr(rd, g), ptr(rd, d_image),
                                 ptr(rd, d_target), ptr(rd, work), bwd, batch, height, width, channels, num_levels, weights,
                                 clamp or 0.0, use_gpu, index)
        return (d_image if ctx.needs_input_grad[0] else None), d_target, None, None, None, None


def _checked(image, target, num_levels, clamp, weights):
    who = 'gaussian_pyramid_loss'
    if not isinstance(image, torch.Tensor) or not isinstance(target, torch.Tensor) or image.dim() not in (3, 4):
        raise ValueError('%s: image and target must be [H, W, C] or [N, H, W, C] tensors' % who)
    if tuple(image.shape) != tuple(target.shape):
        raise ValueError('%s: image is %s, target is %s' % (who, tuple(image.shape), tuple(target.shape)))
    if image.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError('%s: fp32 only, got %s and %s' % (who, image.dtype, target.dtype))
    if image.device != target.device:
        raise ValueError('%s: image is on %s, target on %s' % (who, image.device, target.device))
    if image.numel() == 0:
        raise ValueError('%s: an empty image' % who)
    num_levels = int(num_levels)
    _, height, width, _ = _geometry(image)
    if num_levels < 1 or num_levels > 16 or (min(height, width) >> (num_levels - 1)) < 1:
        raise ValueError('%s: %d levels for a %d x %d image: the smaller side must stay at least 1 texel' %
                         (who, num_levels, height, width))
    if clamp is not None:
        clamp = float(clamp)
        if not clamp > 0.0:
            raise ValueError('%s: clamp must be positive, got %r' % (who, clamp))
    if weights is not None:
        weights = tuple(float(w) for w in weights)
        if len(weights) != num_levels:
            raise ValueError('%s: %d weights for %d levels' % (who, len(weights), num_levels))
    return num_levels, clamp, weights


def gaussian_pyramid_loss(image, target, num_levels=5, clamp=None, weights=None, return_terms=False, backend=None):
    """The loss of the module's docstring as a 0-dim fp32 tensor on the inputs' device; differentiable with respect to `image`
    and `target`.  clamp: clamp image - target to [-clamp, clamp] first (tutorial 05's clamp(-1, 1)); weights: one factor per
    level (a coarse-to-fine schedule), rounded to fp32.  With return_terms=True also the detached fp64 [num_levels] per-level
    terms, summed over the batch."""
    num_levels, clamp, weights = _checked(image, target, num_levels, clamp, weights)
    with named('gaussian_pyramid_loss'):
        loss, terms = GaussianPyramidLoss.apply(image, target, num_levels, clamp, weights, backend)
    return (loss, terms) if return_terms else loss


def pyramid_levels(image, target, num_levels=5, clamp=None, backend=None):
    """For checks: the levels D_1 .. D_{num_levels - 1} the forward call keeps for its gradient, as [N, H_l, W_l, C] tensors."""
    num_levels, clamp, _ = _checked(image, target, num_levels, clamp, None)
    rd = backend or _default_backend
    a, b = image.detach().contiguous(), target.detach().contiguous()
    _, _, saved = _forward(rd, a, b, num_levels, clamp, None)
    flat = saved.view(torch.float32)
    batch, height, width, channels = _geometry(a)
    levels, at = [], 0
    for _ in range(1, num_levels):
        height, width = height // 2, width // 2
        count = batch * height * width * channels
        levels.append(flat[at:at + count].reshape(batch, height, width, channels).clone())
        at += (count + 63) // 64 * 64
    return levels
