"""ABI checks of the method selection (gorio_apd_set_method and the FastVGICP parity hooks): symbols, the untouched parameter struct, refusals."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

apd = importlib.import_module("go-rio_amd.apd")
NEW = ["gorio_apd_set_method", "gorio_apd_get_method", "gorio_apd_get_voxelmap", "gorio_apd_get_voxel_correspondences"]


def test_new_symbols_exported_and_bound(gorio):
    lib = gorio.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in apd.APD_SYMBOLS


def test_params_struct_and_defaults_unchanged(gorio):
    """gorio_apd_params keeps its layout (the method lives behind a call of its own): 15 fields, 96 bytes, the reference's defaults."""
    assert C.sizeof(gorio.ApdParams) == 96 and len(gorio.ApdParams._fields_) == 15
    assert gorio.ApdParams.keep_knn_indices.offset == 88 and gorio.ApdParams.corr_dist_threshold.offset == 32
    p = gorio.ApdParams()
    gorio.load_library().gorio_apd_default_params(C.byref(p))
    assert (p.k_correspondences, p.regularization, p.max_iterations, p.optimizer, p.lm_max_iterations, p.search) == (20, 3, 64, 1, 10, 0)
    assert (p.dist_var, p.azimuth_var, p.elevation_var, p.rotation_epsilon, p.transformation_epsilon) == (0.86, 0.5, 1.0, 2e-3, 5e-4)


def test_enum_values_follow_gicp_settings(gorio):
    assert (apd.METHOD_APDGICP, apd.METHOD_GICP, apd.METHOD_VGICP) == (0, 1, 2)
    assert (apd.VOXEL_DIRECT27, apd.VOXEL_DIRECT7, apd.VOXEL_DIRECT1, apd.VOXEL_DIRECT_RADIUS) == (0, 1, 2, 3)
    assert (apd.VOXEL_ADDITIVE, apd.VOXEL_ADDITIVE_WEIGHTED, apd.VOXEL_MULTIPLICATIVE) == (0, 1, 2)


def test_no_handle_without_device(gorio):
    """A null handle is an invalid argument; without a GPU there is no handle to select a method on (gorio_apd_create refuses, no CPU path)."""
    lib = gorio.load_library()
    assert lib.gorio_apd_set_method(None, 1, C.c_double(1.0), 2, 0) == -1
    assert lib.gorio_apd_get_method(None, None, None, None, None) == -1
    h = C.c_void_p()
    rc = lib.gorio_apd_create(C.byref(h), 0)
    assert rc in (0, -2)  # GORIO_OK on a GPU box, GORIO_ERR_NO_DEVICE everywhere else
    if rc == 0:
        lib.gorio_apd_destroy(h)


def test_variants_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    """host/test/gicp_variants_sequence (FastGICP, FastAPDGICP, FastVGICP through a pcl::Registration pointer) builds next to the existing
    drivers; where gorio_apd_create finds no device the drop-ins refuse (exit status 3), there is no CPU path."""
    from test_host_cpp import HOST, _frames

    gorio.build()
    subprocess.check_call(["make", "-C", HOST])
    driver = os.path.join(HOST, "test", "gicp_variants_sequence")
    assert os.path.exists(driver)
    h = C.c_void_p()
    rc = gorio.load_library().gorio_apd_create(C.byref(h), 0)
    if rc == 0:
        gorio.load_library().gorio_apd_destroy(h)
    path, _ = _frames(str(tmp_path), n_frames=3, n=300)
    r = subprocess.run([driver, path], capture_output=True, text=True, timeout=300)
    if rc == -2:
        assert r.returncode == 3 and "no usable HIP device" in r.stderr
    else:
        assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_method_defaults_and_refusals(gpu, gorio):
    g = gorio.ApdGicp()
    assert g.get_method() == dict(method=apd.METHOD_APDGICP, voxel_resolution=1.0, voxel_search=apd.VOXEL_DIRECT1, voxel_mode=apd.VOXEL_ADDITIVE)
    for args in ((apd.METHOD_VGICP, 1.0, apd.VOXEL_DIRECT_RADIUS, 0), (apd.METHOD_VGICP, 0.0, apd.VOXEL_DIRECT1, 0), (apd.METHOD_VGICP, -1.0, apd.VOXEL_DIRECT1, 0),
                 (7, 1.0, apd.VOXEL_DIRECT1, 0), (apd.METHOD_VGICP, 1.0, 9, 0), (apd.METHOD_VGICP, 1.0, apd.VOXEL_DIRECT1, 5)):
        with pytest.raises(gorio.GorioError) as e:
            g.set_method(*args)
        assert e.value.code == -5  # GORIO_ERR_UNSUPPORTED
    assert g.get_method()["method"] == apd.METHOD_APDGICP  # a refused call changes nothing
    g.set_method(apd.METHOD_VGICP, 0.5, apd.VOXEL_DIRECT27, apd.VOXEL_MULTIPLICATIVE)
    assert g.get_method() == dict(method=apd.METHOD_VGICP, voxel_resolution=0.5, voxel_search=apd.VOXEL_DIRECT27, voxel_mode=apd.VOXEL_MULTIPLICATIVE)
    with pytest.raises(gorio.GorioError) as e:
        g.getVoxelMap()
    assert e.value.code == -3  # no clouds yet: GORIO_ERR_STATE
