"""What every native tensor op (texture, utils, loss, transform, shape, render_utils) does the same way between torch and the
`redner` module: where a tensor lives, its address, scratch memory, the upstream gradient, the name in front of an error."""
import torch


def place(t):
    """(use_gpu, index) of a tensor or a torch.device, as the `redner` module takes them; a device without an index is the
    current one."""
    device = getattr(t, 'device', t)
    use_gpu = device.type == 'cuda'
    index = device.index if device.index is not None else (torch.cuda.current_device() if use_gpu else 0)
    return use_gpu, index


def ptr(rd, t):
    """The float_ptr of a tensor's memory; None stays None (the C side's NULL)."""
    return None if t is None else rd.float_ptr(t.data_ptr())


def scratch(floats, device):
    """Uninitialised memory for at least `floats` floats, never empty.  Its storage is fp64, so it is 8-byte aligned whatever the
    allocator: the ops whose C side asks for that (csrc/arena.h: need_scratch) need no rule of their own.  2 * numel() floats."""
    return torch.empty(max((floats + 1) // 2, 1), dtype=torch.float64, device=device)


def upstream(g, device):
    """An upstream gradient as the kernels read it: fp32, contiguous, on `device`; None (no gradient) stays None."""
    return None if g is None else g.to(device=device, dtype=torch.float32).contiguous()


def first_order_only(name):
    """First line of every native `backward`: the adjoints are kernels, which autograd cannot differentiate again.  Autograd runs
    `backward` in grad mode exactly under create_graph=True (plain and retain_graph passes run it with grad mode off); without
    this the first gradient would come back with requires_grad == False and a second-order term would drop out silently."""
    if torch.is_grad_enabled():
        raise RuntimeError('%s: the native adjoint cannot be differentiated again (create_graph=True)' % name)


class named:
    """with named(who): a RuntimeError from inside leaves with the public function's name in front of its text (and itself as
    the cause); anything else passes."""

    def __init__(self, who):
        self.who = who

    def __enter__(self):
        return self

    def __exit__(self, kind, error, traceback):
        if isinstance(error, RuntimeError):
            raise RuntimeError('%s: %s' % (self.who, error)) from error
