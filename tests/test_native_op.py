"""redner_amd._op: the rules every native tensor op shares -- where a tensor lives, its address, scratch memory, the upstream
gradient, the name in front of an error.  No native call here; one case needs a GPU."""
import pytest
import torch

from redner_amd import _op

CPU = torch.device('cpu')


@pytest.mark.parametrize('floats', (0, 1, 2, 3, 7, 4096))
def test_scratch(floats):
    """fp64 storage of ceil(floats / 2) elements, never empty: room for `floats` floats, 8-byte aligned whatever the allocator."""
    s = _op.scratch(floats, CPU)
    assert s.dtype == torch.float64
    assert s.numel() == max((floats + 1) // 2, 1)
    assert s.data_ptr() % 8 == 0
    assert s.device == CPU


def test_upstream():
    assert _op.upstream(None, CPU) is None
    g = torch.arange(24, dtype=torch.float64).reshape(4, 6)[:, ::2]
    assert tuple(g.shape) == (4, 3) and not g.is_contiguous()
    out = _op.upstream(g, CPU)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.device == CPU
    assert torch.equal(out.double(), g)
    ready = torch.ones(4, 3)
    assert _op.upstream(ready, CPU).data_ptr() == ready.data_ptr()
    # what out.sum().backward() hands over: one element expanded with strides of 0
    expanded = torch.full((), 3.0).expand(4, 3)
    assert expanded.stride() == (0, 0) and not expanded.is_contiguous()
    out = _op.upstream(expanded, CPU)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (4, 3) and out.stride() == (3, 1)
    assert out.untyped_storage().nbytes() >= 4 * 12 and bool((out == 3.0).all())


def test_named():
    with pytest.raises(RuntimeError) as caught:
        with _op.named('x'):
            raise RuntimeError('m')
    assert str(caught.value) == 'x: m'
    assert isinstance(caught.value.__cause__, RuntimeError) and str(caught.value.__cause__) == 'm'
    error = ValueError('m')
    with pytest.raises(ValueError) as caught:
        with _op.named('x'):
            raise error
    assert caught.value is error and error.__cause__ is None and str(error) == 'm'
    with _op.named('x'):
        pass


def test_ptr():
    class Backend:
        float_ptr = staticmethod(lambda address: ('float_ptr', address))

    t = torch.zeros(3)
    assert _op.ptr(Backend, None) is None
    assert _op.ptr(Backend, t) == ('float_ptr', t.data_ptr())


def test_place():
    assert _op.place(torch.empty(1)) == (False, 0)
    assert _op.place(CPU) == (False, 0)


@pytest.mark.gpu
def test_place_gpu():
    assert _op.place(torch.empty(1, device='cuda')) == (True, torch.cuda.current_device())
