"""tests/map_cloud_restatement.py against itself (CPU): the lattice include/gorio_map.h defines equals the one PCL's growing bounding box
arrives at -- same voxel count, every centre within one float ulp per coordinate -- and the closed forms of the gate, the anchor and the
dedup hold.  The one-ulp bound is derived, not measured: both forms round the same real number (key + 0.5) * resolution + corner from
doubles that differ by the rounding of the moved corner, about 1e-13 at these coordinates, far below half a float ulp (4e-6 at 50 m), so
the two float results are equal or neighbours.  The derivation is about the lattice, so it holds for every point that is inside a
cell; a point that lies exactly ON a cell face (map_cloud_restatement.face_ties says how float coordinates bring that about) falls to
one side or the other by the rounding of a double quotient, in PCL as here.  Such points are counted, required to be few, and set aside
before the two lattices are compared."""
import numpy as np
import pytest

import map_cloud_restatement as mr

F = np.float32


@pytest.fixture(scope="module")
def curve_map():
    """8 keyframes of 4000 radar-like points, snapped to 0.5 m plus 0.05 m of noise, on a curving trajectory: stage A once for all."""
    frames, poses = mr.scene([4000] * 8, seed=100)
    q, inten = mr.stage_a(frames, poses)
    assert 8 * 4000 * 0.6 < len(q) < 8 * 4000  # the gate dropped some (ranges reach 60 m) and kept most
    return q


@pytest.mark.parametrize("resolution", [0.05, 0.1, 0.3, 0.7])
def test_direct_lattice_equals_the_emulated_pcl_growth(curve_map, resolution):
    ties = mr.face_ties(curve_map, resolution)
    assert not ties[0] and ties.sum() <= 8, ties.sum()  # the anchor sits in the middle of its cell; ties are a handful in 25 000 points
    print("points on a cell face at %g: %d of %d" % (resolution, ties.sum(), len(ties)))
    curve_map = curve_map[~ties]
    c, info = mr.voxel_centres(curve_map, resolution)
    p = mr.pcl_voxel_centres(curve_map, resolution)
    assert len(c) == len(p) == info["n_voxels"]
    assert info["n_voxels"] < info["n_finite"] == len(curve_map)  # voxels are shared
    assert min(info["min_k"]) < 0 < max(info["max_k"])  # the anchor lies inside the map: PCL's corner did move
    d = mr.ulp_distance(c, p)
    assert d.max() <= 1, d.max()


def test_one_point_gives_its_own_float():
    for res in (0.05, 0.3, 1.0):
        for pt in ([1.25, -3.5, 0.75], [10.1, 20.2, -0.3], [0.0, 0.0, 0.0]):
            xyz, inten, info = mr.generate([(np.array([pt], F), np.array([7.0], F))], [np.eye(4)], res)
            # a = q0 - res / 2, k = 0, centre = 0.5 * res + a: q0 again up to one double rounding, far below a float ulp
            assert xyz.shape == (1, 3) and np.array_equal(xyz.view(np.uint32), np.array([pt], F).view(np.uint32))
            assert inten.tolist() == [0.0] and info["n_voxels"] == 1 and info["min_k"] == info["max_k"] == [0, 0, 0]


def test_a_keyframe_listed_twice_gives_the_map_of_one():
    frames, poses = mr.scene([700], seed=5)
    one = mr.generate(frames, poses, 0.3)
    two = mr.generate(frames * 2, poses * 2, 0.3)
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)) and two[2]["n_kept"] == 2 * one[2]["n_kept"] and two[2]["n_voxels"] == one[2]["n_voxels"]
    raw = mr.generate(frames * 2, poses * 2, 0.0)
    assert len(raw[0]) == 2 * one[2]["n_kept"]  # no dedup without a resolution


def test_gate_edges():
    above = np.nextafter(F(40.0), F(np.inf))
    xyz = np.array([[30, 40, 0], [30, above, 0], [0, 0, 50], [np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, 0], [0, 0, np.nextafter(F(50.0), F(np.inf))]], F)
    assert mr.gate(xyz).tolist() == [True, False, True, True, False, False, False]


def test_nan_survives_without_a_resolution_and_vanishes_with_one():
    xyz = np.array([[1, 2, 3], [np.nan, 1, 1], [4, 5, 6]], F)
    frames = [(xyz, np.array([1, 2, 3], F))]
    q, inten, info = mr.generate(frames, [np.eye(4)], 0.0)
    assert len(q) == 3 and np.isnan(q[1, 0]) and inten.tolist() == [1.0, 2.0, 3.0] and info["n_kept"] == 3
    c, inten, info = mr.generate(frames, [np.eye(4)], 0.5)
    assert len(c) == 2 and np.isfinite(c).all() and not inten.any() and (info["n_kept"], info["n_finite"], info["n_voxels"]) == (3, 2, 2)


def test_anchor_falls_to_the_first_finite_kept_point():
    xyz = np.array([[np.inf, 0, 0], [np.nan, 1, 1], [2.5, 1.5, 0.5], [2.6, 1.5, 0.5]], F)  # dropped; kept but not finite; the anchor
    c, _, info = mr.generate([(xyz, None)], [np.eye(4)], 1.0)
    assert info["anchor"] == [2.0, 1.0, 0.0] and info["n_kept"] == 3 and info["n_finite"] == 2
    assert c.tolist() == [[2.5, 1.5, 0.5]] and info["n_voxels"] == 1


def test_float_pose_differs_from_the_double_transform():
    frames, poses = mr.scene([500, 500], seed=9)
    qf, _ = mr.stage_a(frames, poses)
    qd, _ = mr.stage_a(frames, poses, mr.transform_double)
    assert qf.shape == qd.shape and not np.array_equal(qf.view(np.uint32), qd.view(np.uint32))
    assert mr.ulp_distance(qf, qd).max() < 64  # the same transform, rounded differently


def test_limits_raise():
    far = [(np.array([[1, 1, 1]], F), None), (np.array([[1, 1, 1]], F), None)]
    poses = [np.eye(4), np.eye(4)]
    poses[1] = poses[1].copy()
    poses[1][0, 3] = 300.0
    with pytest.raises(OverflowError):
        mr.generate(far, poses, 1e-4)  # 3e6 cells apart: more than 2^21
    with pytest.raises(OverflowError):
        mr.generate(far, poses, 1e-8)  # 3e10: past 2^30
