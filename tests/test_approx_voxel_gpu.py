"""GPU: gorio_prep_approx_voxel_downsample (csrc/apd_approx_voxel.hip) against tests/approx_voxel_restatement.py -- output, order and
n_out bit for bit."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import approx_voxel_restatement as R
import approx_voxel_scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
CLOUDS, same = S.CLOUDS, S.same
prep = importlib.import_module("go-rio_amd.prep")
GorioError = importlib.import_module("go-rio_amd.apd").GorioError


@functools.lru_cache(maxsize=None)
def scene(name):
    """(cloud, leaf, the restatement's output): computed once, never modified."""
    p, leaf = CLOUDS[name]()
    want = R.sequential(p, leaf)
    p.setflags(write=False)
    want.setflags(write=False)
    return p, leaf, want


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_matches_restatement(gpu, name):
    p, leaf, want = scene(name)
    got = prep.approx_voxel_downsample(p, leaf)
    assert got.shape == want.shape  # n_out
    assert same(got, want)
    if name in ("ring_scan", "real_target"):
        assert len(got) <= len(p) / 2  # the case is not the identity
    if name == "one_cell":
        assert len(got) == 1
    if name == "alternating":
        assert len(got) == len(p)
    if name == "buckets_512":
        assert len(got) == 512


def raw_call(pts, n, stride_bytes, offsets, leaf, out, out_stride_bytes, capacity, device=0):
    lib = importlib.import_module("go-rio_amd").load_library()
    offs = np.ascontiguousarray(offsets, np.int32)
    lf = np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, np.float64).reshape(-1), (3,)), np.float64)
    m = C.c_int(-5)
    rc = lib.gorio_prep_approx_voxel_downsample(device, C.c_void_p(pts.ctypes.data), n, stride_bytes, C.c_void_p(offs.ctypes.data), len(offs), C.c_void_p(lf.ctypes.data),
                                                C.c_void_p(out.ctypes.data) if out is not None else None, out_stride_bytes, capacity, C.byref(m))
    return rc, m.value


def test_strided_xyzinormal_offsets(gpu):
    """F = 8 through the field offsets of pcl::PointXYZINormal: the padding floats are neither read into the averages nor written."""
    p = S.xyzinormal(3000, 30)
    want = R.sequential(p[:, S.XYZINORMAL_OFFSETS], 0.5)
    out = np.full((3000, 12), f32(-5.0), f32)
    rc, m = raw_call(p, 3000, 48, S.XYZINORMAL_OFFSETS, 0.5, out, 48, 3000)
    assert rc == 0 and m == len(want) and m < 3000
    assert same(np.ascontiguousarray(out[:m][:, S.XYZINORMAL_OFFSETS]), want)
    assert (out[:, [3, 7, 10, 11]] == f32(-5.0)).all() and (out[m:] == f32(-5.0)).all()
    # F = 3 of the same strided cloud: downsample_all_data_ = false
    want3 = R.sequential(p[:, :3], 0.5)
    out3 = np.full((3000, 12), f32(-5.0), f32)
    rc, m3 = raw_call(p, 3000, 48, [0, 1, 2], 0.5, out3, 48, 3000)
    assert rc == 0 and m3 == len(want3)
    assert same(np.ascontiguousarray(out3[:m3, :3]), want3) and (out3[:, 3:] == f32(-5.0)).all()


def test_capacity_too_small(gpu):
    p, leaf, want = scene("gauss_3000")
    out = np.full((len(p), 4), f32(-5.0), f32)
    rc, m = raw_call(p, len(p), 16, [0, 1, 2, 3], leaf, out, 16, len(want) - 1)
    assert rc == -1 and m == len(want)
    assert (out == f32(-5.0)).all()
    rc, m = raw_call(p, len(p), 16, [0, 1, 2, 3], leaf, out, 16, len(want))  # exactly enough
    assert rc == 0 and m == len(want) and same(np.ascontiguousarray(out[:m]), want)


@pytest.mark.parametrize("bad", [np.nan, np.inf, 1e12])
def test_refused_clouds(gpu, bad):
    p = S.gaussian(1000, 31).copy()
    p[617, 2] = bad
    out = np.full((1000, 4), f32(-5.0), f32)
    rc, m = raw_call(p, 1000, 16, [0, 1, 2, 3], 0.1, out, 16, 1000)
    assert rc == -1 and m == 0
    assert (out == f32(-5.0)).all()
    with pytest.raises(GorioError) as e:
        prep.approx_voxel_downsample(p, 0.1)
    assert e.value.code == -1
    # the next call of the same thread is served as usual
    q, leaf, want = scene("n257")
    assert same(prep.approx_voxel_downsample(q, leaf), want)


def test_nan_in_a_non_coordinate_field_is_averaged(gpu):
    p = S.gaussian(2000, 32, span=2.0).copy()
    p[::97, 3] = np.nan
    want = R.sequential(p, 0.5)
    got = prep.approx_voxel_downsample(p, 0.5)
    assert np.isnan(want[:, 3]).any() and same(got, want)


class Hip:
    """device arrays through the HIP runtime the library links against"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.ptrs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        self.ptrs.append(p)
        return p.value

    def dev(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(C.c_void_p(p), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p

    def host(self, p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipDeviceSynchronize() == 0
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.mark.parametrize("name", ["gauss_3000", "fields_8", "fields_3", "one_cell"])
def test_device_form_equals_host_form(gpu, name):
    p, leaf, want = scene(name)
    n, nf = p.shape
    lib = importlib.import_module("go-rio_amd").load_library()
    hip = Hip()
    try:
        cols = (C.c_void_p * nf)(*[hip.dev(p[:, f]) for f in range(nf)])
        sentinel = np.full(n, f32(-5.0), f32)
        outs = (C.c_void_p * nf)(*[hip.dev(sentinel) for _ in range(nf)])
        lf = np.ascontiguousarray(R.leaf3(leaf), np.float64)
        m = C.c_int(-5)
        rc = lib.gorio_prep_approx_voxel_downsample_device(0, cols, nf, n, C.c_void_p(lf.ctypes.data), outs, n, C.byref(m), None)
        assert rc == 0 and m.value == len(want)
        got = np.stack([hip.host(outs[f], n, f32) for f in range(nf)], axis=1)
        assert same(np.ascontiguousarray(got[:m.value]), want)
        assert (got[m.value:] == f32(-5.0)).all()
        rc = lib.gorio_prep_approx_voxel_downsample_device(0, cols, nf, n, C.c_void_p(lf.ctypes.data), outs, max(len(want) - 1, 0), C.byref(m), None)
        assert rc == -1 and m.value == len(want)
    finally:
        hip.free()

