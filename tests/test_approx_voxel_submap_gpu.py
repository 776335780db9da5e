"""GPU: gorio_apd_set_submap_downsample -- the scan-to-submap calls with downsample_method APPROX_VOXELGRID
(scan_matching_odometry_nodelet.cpp:150-154) against tests/approx_voxel_restatement.py applied to the oracle's unthinned assembly."""
import importlib

import numpy as np
import pytest

import approx_voxel_restatement as R
from approx_voxel_scenes import same

pytestmark = pytest.mark.gpu
synth = importlib.import_module("go-rio_amd.synth")
apd = importlib.import_module("go-rio_amd.apd")
F = np.float32
KW = dict(corr_dist_threshold=2.0, search=1, transformation_epsilon=0.01)


def _keyframes(n_frames=5, n=3000, noise=True):
    frames, odoms = [], []
    for k in range(n_frames):
        odom = synth.gt_transform([0.6 * k, 0.05 * k, 0.01 * k], [0.1 * k, -0.05 * k, 1.2 * k])
        xyz, lab = synth.radar_scan(n + 37 * k, seed=500 + k, sensor_pose=odom, noise=noise)
        frames.append((xyz, lab))
        odoms.append(odom)
    rel = [np.linalg.inv(odoms[-1]) @ odoms[i] for i in range(n_frames - 1)]
    return frames[:-1], rel, frames[-1]


@pytest.fixture(scope="module")
def case(oracle_apd):
    """Frames (one non-finite point among them), poses, the newest scan, the oracle's unthinned assembly as [m, 4] rows."""
    frames, rel, newest = _keyframes()
    frames[2][0][11, 1] = np.inf  # dropped before the filter, as the submap path does today
    xo, lo = oracle_apd.submap_assemble(frames, rel, 0.0)
    return frames, rel, newest, np.concatenate([xo, lo[:, None]], axis=1).astype(F)


def _target(g):
    x, l = g.getTargetPoints()
    return np.concatenate([x, l[:, None]], axis=1)


def test_enum_values_and_persistence(gpu, gorio, case):
    frames, rel, _, full = case
    assert (apd.DOWNSAMPLE_VOXELGRID, apd.DOWNSAMPLE_APPROX_VOXELGRID) == (0, 1)
    g = gorio.ApdGicp(**KW)
    assert g.getSubmapDownsample() == apd.DOWNSAMPLE_VOXELGRID
    with pytest.raises(gorio.GorioError) as e:
        g.setSubmapDownsample(2)
    assert e.value.code == -1 and g.getSubmapDownsample() == 0
    g.setSubmapDownsample(apd.DOWNSAMPLE_APPROX_VOXELGRID)
    want = R.sequential(full, 0.5)
    for _ in range(2):  # the method persists across calls
        assert g.setInputTargetSubmap(frames, rel, voxel_leaf=0.5) == len(want)
        assert g.getSubmapDownsample() == 1 and same(_target(g), want)
    assert g.setInputTargetSubmap(frames, rel, voxel_leaf=0.0) == len(full) and same(_target(g), full)  # voxel_leaf <= 0 is unchanged
    g.setSubmapDownsample(apd.DOWNSAMPLE_VOXELGRID)  # and back
    h = gorio.ApdGicp(**KW)
    assert g.setInputTargetSubmap(frames, rel, voxel_leaf=0.5) == h.setInputTargetSubmap(frames, rel, voxel_leaf=0.5)
    assert same(_target(g), _target(h))


@pytest.mark.parametrize("leaf", [0.1, 0.5])
def test_approx_submap_equals_restatement(gpu, gorio, case, leaf):
    frames, rel, _, full = case
    want = R.sequential(full, F(leaf))
    assert 0 < len(want) < len(full)
    g = gorio.ApdGicp(**KW)
    g.setSubmapDownsample(apd.DOWNSAMPLE_APPROX_VOXELGRID)
    assert g.setInputTargetSubmap(frames, rel, voxel_leaf=leaf) == len(want)
    assert same(_target(g), want)
    # the label is the plain float mean of the run, not VoxelGrid's normalised sign
    assert np.abs(want[:, 3]).max() > 1.0
    store = gorio.KeyframeStore()
    try:
        ids = [store.add(x, label=l) for x, l in frames]
        k = gorio.ApdGicp(**KW)
        k.setSubmapDownsample(apd.DOWNSAMPLE_APPROX_VOXELGRID)
        assert k.setInputTargetSubmapKeyframes(store, ids, rel, voxel_leaf=leaf) == len(want)
        assert same(_target(k), want)
    finally:
        store.close()


def test_default_method_is_unchanged(gpu, gorio, oracle_apd, case):
    frames, rel, _, _ = case
    for leaf in (0.1, 0.5):
        xo, lo = oracle_apd.submap_assemble(frames, rel, leaf)
        g = gorio.ApdGicp(**KW)
        assert g.setInputTargetSubmap(frames, rel, voxel_leaf=leaf) == len(xo)
        x, l = g.getTargetPoints()
        assert same(x, xo) and same(l, lo)


def test_align_against_approx_submap(gpu, gorio, pose_err):
    """The newest scan against the approx-thinned submap converges to the pose of the align against the unthinned one within 50 times the
    project's 1e-4 m / 1e-4 rad gate (the targets differ, hence the factor).

    The scene is the synthetic one WITHOUT the radar noise model.  With it a point at 50 m scatters by 0.4 m in azimuth and 0.9 m in
    elevation (synth.radar_scan), the optimum of an align moves by centimetres with the sample (tests/test_submap_gpu.py accepts 0.05 m
    from the truth on that scene), and a 5e-3 m gate would measure that scatter: observed there 3.3e-2 m / 3.1e-3 rad between the two
    targets at leaf 0.1 with both aligns run to a 1e-6 step, 1.2e-2 m with the shipped 0.01 step.  On the noise-free scans every point
    lies on a plane of the scene, a run's centroid lies on the same plane unless the run straddles an edge, so the thinned target
    describes the same surfaces.  Both aligns stop on a step far below the gate (1e-6): the two optima are compared, not the places
    where a loose termination test happened to stop."""
    frames, rel, newest = _keyframes(noise=False)
    kw = dict(KW, transformation_epsilon=1e-6, rotation_epsilon=1e-6, max_iterations=256)
    a, b = gorio.ApdGicp(**kw), gorio.ApdGicp(**kw)
    na = a.setInputTargetSubmap(frames, rel, voxel_leaf=0.0)
    b.setSubmapDownsample(apd.DOWNSAMPLE_APPROX_VOXELGRID)
    nb = b.setInputTargetSubmap(frames, rel, voxel_leaf=0.1)
    assert nb < na
    for g in (a, b):
        g.setInputSource(*newest)
    ra, rb = a.align(), b.align()
    te, re = pose_err(ra["T"], rb["T"])
    print(f"approx-thinned (leaf 0.1, {nb} of {na} points) vs unthinned submap: {te:.3e} m, {re:.3e} rad; iterations {ra['nr_iterations']} / {rb['nr_iterations']}")
    assert ra["converged"] and rb["converged"]
    assert te < 50 * 1e-4 and re < 50 * 1e-4, (te, re)


def test_refused_cloud_keeps_the_old_target(gpu, gorio, case):
    frames, rel, _, full = case
    g = gorio.ApdGicp(**KW)
    g.setSubmapDownsample(apd.DOWNSAMPLE_APPROX_VOXELGRID)
    n0 = g.setInputTargetSubmap(frames, rel, voxel_leaf=0.5)
    before = _target(g)
    far = (frames[0][0].copy(), frames[0][1].copy())
    far[0][100, 0] = F(1e12)  # finite, but its cell coordinate at leaf 0.1 leaves (-2^30, 2^30)
    with pytest.raises(gorio.GorioError) as e:
        g.setInputTargetSubmap([far] + list(frames[1:]), rel, voxel_leaf=0.1)
    assert e.value.code == -1
    assert g._n_tgt == n0 and same(_target(g), before)
    store = gorio.KeyframeStore()
    try:
        ids = [store.add(x, label=l) for x, l in [far] + list(frames[1:])]
        with pytest.raises(gorio.GorioError) as e:
            g.setInputTargetSubmapKeyframes(store, ids, rel, voxel_leaf=0.1)
        assert e.value.code == -1 and same(_target(g), before)
    finally:
        store.close()
