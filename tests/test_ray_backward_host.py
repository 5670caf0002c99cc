"""CPU tests of the ray-gradient C ABI (include/nerf_hip.h: nerf_hip_render_backward_rays): the ctypes mirror of the
new argument block, the exports, and argument errors caught on the host before any HIP call."""
import ctypes
import os
import re

import pytest

from test_abi_host import ROOT, declared_symbols, header_fields


@pytest.fixture(scope="module")
def handle():
    from nerf_amd import build as nerf_build
    nerf_build.build()
    from nerf_amd import _lib
    return _lib.lib()


def test_ray_backward_struct_matches_the_header():
    from nerf_amd import _lib
    text = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    for c_name, mirror in (("NerfHipRayBackwardArgs", _lib.RayBackwardArgs), ("NerfHipBackwardArgs", _lib.BackwardArgs)):
        assert header_fields(text, c_name) == [f[0] for f in mirror._fields_], c_name
    defines = dict(re.findall(r"#define (NERF_HIP_\w+) (\d+)", text))
    assert int(defines["NERF_HIP_TIMING_RAY_GRADIENT"]) == 9
    assert int(defines["NERF_HIP_TIMING_TAGS"]) == _lib.TIMING_TAGS == 10


def test_ray_backward_symbols_are_exported(handle):
    from nerf_amd import _lib
    for name in ("nerf_hip_render_backward_rays", "nerf_hip_ray_backward_scratch_bytes"):
        assert name in declared_symbols() and name in _lib.EXPORTS
        assert hasattr(handle, name)
    assert handle.nerf_hip_timing_tag_name(9) == b"ray_gradient"
    assert handle.nerf_hip_timing_tag_name(10) is None


def test_ray_backward_scratch_bytes(handle):
    assert handle.nerf_hip_ray_backward_scratch_bytes(0, 64) == 0
    assert handle.nerf_hip_ray_backward_scratch_bytes(5, 1) == 0
    # one partial of 8 floats per (padded ray, 16-sample chunk)
    assert handle.nerf_hip_ray_backward_scratch_bytes(4096, 64) == 4096 * 4 * 8 * 4
    assert handle.nerf_hip_ray_backward_scratch_bytes(5, 9) == 8 * 1 * 8 * 4


def test_ray_backward_argument_errors_do_not_touch_the_gpu(handle):
    from nerf_amd import _lib
    assert handle.nerf_hip_render_backward_rays(None, None) == -1
    assert b"null args" in handle.nerf_hip_last_error()
    args = _lib.RayBackwardArgs()                        # empty: no output asked for
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -1
    dummy = ctypes.c_void_p(16)
    args.d_rays_o = dummy
    fwd = args.bwd.fwd
    fwd.n_rays, fwd.num_samples, fwd.num_outputs = 8, 1, 54
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -1       # num_samples < 2
    fwd.num_samples = 16
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -1       # rays are not explicit
    assert b"explicit" in handle.nerf_hip_last_error()
    fwd.rays_o = fwd.rays_d = dummy
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -1       # w0 / ray_scratch null
    args.w0 = args.ray_scratch = dummy
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -1       # no scratch, no d_rgb / d_raw
    args.bwd.scratch = args.bwd.d_rgb = dummy
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -1       # not a training forward
    assert b"training forward" in handle.nerf_hip_last_error()
    fwd.num_outputs = 65
    assert handle.nerf_hip_render_backward_rays(ctypes.byref(args), None) == -2       # shape out of range
