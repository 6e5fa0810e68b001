"""bench.py's plain run and `--dump-outputs DIR`: what the timed path computed in its last step, written as DIR/<name>.npy
(float32, at most 64 MiB in all; a larger array as a fixed, seeded sample), so that two builds can be compared output for
output.  The measurements beyond the headline figure run only under `--full` (tests/test_rccl_gpu.py)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('roofline', 'roofline_large', 'sharded_check', 'self_check', 'cpu_baseline', 'scene_build_warm_ms')


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_dump_outputs_caps_the_total_with_a_fixed_sample(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(3)
    prep = types.SimpleNamespace(img=torch.rand(64, 64, 3, generator=g),
                                 grads=[torch.rand(5, generator=g), torch.rand(300000, 3, generator=g).double(),
                                        torch.rand(200, 3, generator=g)],
                                 grad_names=['grad_light0_intensity', 'grad_shape0_vertices', 'grad_shape1_vertices'])
    cap = 1 << 20
    outs = []
    for run in ('a', 'b'):
        d = str(tmp_path / run)
        bench.dump_outputs(prep, d, cap_bytes=cap)
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= cap
        outs.append(_load_dir(d))
    a, b = outs
    assert sorted(a) == ['grad_light0_intensity', 'grad_shape0_vertices', 'grad_shape1_vertices', 'image']
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k
    # what fits is written whole; the one array that does not is a sample of its elements, in index order
    assert np.array_equal(a['image'], prep.img.numpy()) and np.array_equal(a['grad_light0_intensity'], prep.grads[0].numpy())
    assert np.array_equal(a['grad_shape1_vertices'], prep.grads[2].numpy())
    big = prep.grads[1].float().numpy().reshape(-1)
    s = a['grad_shape0_vertices']
    assert s.ndim == 1 and 0 < s.size < big.size
    assert np.isin(s, big).all()


def test_dump_outputs_of_a_prepared_step(hostsim_backend, tmp_path):
    """The names say which input a gradient belongs to; the files are what the step left in the buffers."""
    bench = _bench()
    import scenes
    cpu = torch.device('cpu')
    prep = bench.Prepared(hostsim_backend, scenes.bunny_box(cpu, resolution=(16, 16)), 2, 2, 0, 4, cpu)
    prep.step(0)
    assert len(set(prep.grad_names)) == len(prep.grad_names)
    assert 'grad_shape6_vertices' in prep.grad_names and 'grad_light0_intensity' in prep.grad_names
    assert not any(n.startswith('grad_arg') for n in prep.grad_names), prep.grad_names
    d = str(tmp_path / 'out')
    bench.dump_outputs(prep, d)
    z = _load_dir(d)
    assert sorted(z) == sorted(['image'] + prep.grad_names)
    assert np.array_equal(z['image'], prep.img.numpy()) and float(np.abs(z['image']).sum()) > 0
    for n, t in zip(prep.grad_names, prep.grads):
        assert np.array_equal(z[n], t.numpy()), n
    assert float(np.abs(z['grad_shape6_vertices']).sum()) > 0


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_outputs(tmp_path):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'MASTER_PORT', 'MASTER_ADDR', 'REDNER_AMD_LIBM', 'REDNER_AMD_LIB'):
        env.pop(k, None)
    d = str(tmp_path / 'out')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--res', '64', '--spp', '4', '--steps', '2',
                        '--warmup', '1', '--dump-outputs', d], env=env, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert all(k in j for k in HEADLINE), j
    assert j['steps'] == 2 and j['ms_per_step'] > 0 and j['value'] > 0 and j['full'] is False
    assert not any(k in j for k in FULL_ONLY), sorted(j)
    z = _load_dir(d)
    assert z['image'].shape == (64, 64, 3) and z['image'].dtype == np.float32 and np.isfinite(z['image']).all()
    assert float(z['image'].sum()) > 0 and float(np.abs(z['grad_shape6_vertices']).sum()) > 0
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 2 ** 20
