"""The C-ABI library loads and exports every symbol include/redner_amd.h declares; the product
refuses to run without a GPU (no CPU fallback).  No compute calls here (-m "not gpu")."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'redner_amd.h')
LIB = os.path.join(ROOT, 'redner_amd', 'lib', 'libredner_amd.so')


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(rdr_[a-z_0-9]+)\s*\(', src)))


def test_header_declares_the_boundary():
    syms = declared_symbols()
    for s in ('rdr_scene_create', 'rdr_scene_destroy', 'rdr_render', 'rdr_compute_num_channels', 'rdr_last_error'):
        assert s in syms


@pytest.mark.skipif(not os.path.exists(LIB), reason='libredner_amd.so not built (run __graft_entry__.build())')
def test_product_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(LIB)
    for s in declared_symbols():
        assert hasattr(lib, s), s


@pytest.mark.skipif(not os.path.exists(LIB), reason='libredner_amd.so not built')
def test_no_cpu_fallback():
    """Scene(use_gpu=False) must fail loudly; so must a machine without a HIP device."""
    import torch
    from redner_amd import _capi
    previous = _capi.library_path()
    _capi.load(LIB)
    try:
        from redner_amd import redner
        import scenes
        from redner_amd.render_pytorch import RenderFunction
        sc = scenes.single_triangle(torch.device('cpu'), resolution=(8, 8))
        args = RenderFunction.serialize_scene(sc, 1, 1, sampler_type=redner.SamplerType.sobol, device=torch.device('cpu'))
        with pytest.raises(RuntimeError, match='no CPU fallback|HIP device'):
            RenderFunction.apply(1, *args)
    finally:
        if previous:
            _capi.load(previous)        # other tests in this session use the host harness


def test_compute_num_channels(hostsim_backend):
    rd = hostsim_backend
    assert rd.compute_num_channels([rd.channels.radiance], 0) == 3
    assert rd.compute_num_channels([rd.channels.radiance, rd.channels.alpha, rd.channels.uv, rd.channels.generic_texture], 5) == 11


def test_missing_library_is_an_error(tmp_path):
    from redner_amd import _capi
    with pytest.raises(RuntimeError, match='not found'):
        _capi.load(str(tmp_path / 'nope.so'))


def declared_signatures(header):
    """name -> number of parameters, for every rdr_* function the header of include/ declares"""
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    found = {}
    for name, params in re.findall(r'\b(rdr_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', src):
        params = params.strip()
        found[name] = 0 if params in ('', 'void') else len(params.split(','))
    return found


# header -> what pins its set of functions: how many there are (redner_amd.h, which is fixed) or their sorted names
DECLARED = {
    'redner_amd.h': 43,
    'redner_amd_mesh.h': ['rdr_mesh_boundary', 'rdr_mesh_laplacian', 'rdr_mesh_laplacian_backward', 'rdr_mesh_smooth',
                          'rdr_mesh_smooth_scratch'],
    'redner_amd_image.h': ['rdr_pyramid_loss', 'rdr_pyramid_loss_backward', 'rdr_pyramid_loss_plan', 'rdr_pyramid_loss_scratch'],
    'redner_amd_pose.h': ['rdr_pose_plan', 'rdr_pose_scratch', 'rdr_pose_vertices', 'rdr_pose_vertices_backward',
                          'rdr_rotate_matrix', 'rdr_rotate_matrix_backward'],
    'redner_amd_debug.h': ['rdr_debug_lane_park', 'rdr_debug_scene_trace', 'rdr_debug_trace_occupancy'],
}


@pytest.mark.parametrize('header', list(DECLARED))
def test_signature_table_matches_the_header(hostsim_backend, header):
    """Every function a header declares has a (restype, argtypes) entry of the right length under that header in _capi.HEADERS and
    there is no entry without a declaration: a forgotten signature would send 64-bit handles through ctypes' default int
    conversion.  No name stands under two headers, and the harness library and, where they are built, both product libraries
    export every one."""
    from conftest import HOSTSIM_LIB
    from redner_amd import _capi
    declared, table, pinned = declared_signatures(header), _capi.HEADERS[header], DECLARED[header]
    assert sorted(_capi.HEADERS) == sorted(DECLARED) == sorted(os.listdir(os.path.join(ROOT, 'include')))
    assert (len(declared) if isinstance(pinned, int) else sorted(declared)) == pinned
    assert set(declared) == set(table)
    for name, count in declared.items():
        assert len(table[name][1]) == count, name
    for other, others in _capi.HEADERS.items():
        assert other == header or not set(declared) & set(others), other
    for path in (HOSTSIM_LIB, _capi.DEFAULT_LIBRARY, _capi.EXACT_LIBRARY):
        if path == HOSTSIM_LIB or os.path.exists(path):
            lib = ctypes.CDLL(path)
            for name in declared:
                assert hasattr(lib, name), (path, name)


def _null_handles_are_errors(lib, tmp_path):
    """The entry points that used to dereference a null Scene report it; a call that succeeds clears the text.  No kernel runs."""
    def error():
        return lib.rdr_last_error().decode()

    assert lib.rdr_scene_trace(None, None, None, 0, 0) == 1 and 'rdr_scene_trace' in error()
    assert lib.rdr_debug_bvh_check(None) == -2 and 'rdr_debug_bvh_check' in error()
    path = tmp_path / 'edges.txt'
    assert lib.rdr_debug_dump_edges(None, str(path).encode()) == 1 and 'rdr_debug_dump_edges' in error()
    assert not path.exists()
    assert lib.rdr_render(None, None, None, None, None, None, None) == 1
    assert error() == 'rdr_render: scene and options are required'
    out = (ctypes.c_int32 * 10)()
    assert lib.rdr_debug_trace_plan(1000, 24, 1, 20, 1000, 0, 0, 0, None, out) == 0       # host arithmetic only
    assert error() == ''


def test_null_handles_are_errors_harness(hostsim_backend, tmp_path):
    from redner_amd import _capi
    _null_handles_are_errors(_capi.lib(), tmp_path)


@pytest.mark.gpu
def test_null_handles_are_errors_product(gpu_backend, tmp_path):
    from redner_amd import _capi
    _null_handles_are_errors(_capi.lib(), tmp_path)


def test_arena_rule(tmp_path):
    """csrc/arena.h over a counting stand-in for exec.h (tests/arena), as a program of its own under ASan + UBSan: blocks go
    back when the owner dies, and only an owner that dies during stack unwinding waits for the device first."""
    import subprocess
    exe = str(tmp_path / 'arena_rule')
    subprocess.check_call(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-I' + os.path.join(ROOT, 'tests', 'arena'), '-I' + os.path.join(ROOT, 'redner_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'arena', 'arena_rule.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'arena rule ok' in r.stdout


def _device_index_beyond_the_table_is_an_error(lib):
    """A device index the per-device tables (csrc/per_device.h) have no slot for is refused where it enters, with a text that names
    the index and the limit -- it used to share device 0's lock, caches and pool lists; a call that succeeds clears the text.  No
    kernel runs."""
    assert not lib.rdr_mesh_topology_create(None, 0, 1, 1, 16)
    text = lib.rdr_last_error().decode()
    assert re.search(r'device index 16\b', text) and re.search(r'\b16 devices\b', text), text
    out = (ctypes.c_int32 * 10)()
    assert lib.rdr_debug_trace_plan(1000, 24, 1, 20, 1000, 0, 0, 0, None, out) == 0       # host arithmetic only
    assert lib.rdr_last_error().decode() == ''


def test_device_index_beyond_the_table_is_an_error_harness(hostsim_backend):
    from redner_amd import _capi
    _device_index_beyond_the_table_is_an_error(_capi.lib())


@pytest.mark.gpu
def test_device_index_beyond_the_table_is_an_error_product(gpu_backend):
    from redner_amd import _capi
    _device_index_beyond_the_table_is_an_error(_capi.lib())


def test_per_device_rule(tmp_path):
    """csrc/per_device.h (tests/per_device), as a program of its own under ASan + UBSan: sixteen distinct slots, host memory on
    slot 0, an index beyond them is an error that names it, iteration in index order, slots of a type that is not copied."""
    import subprocess
    exe = str(tmp_path / 'per_device_rule')
    subprocess.check_call(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-I' + os.path.join(ROOT, 'redner_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'per_device', 'per_device_rule.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'per-device rule ok' in r.stdout
