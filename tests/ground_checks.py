"""What the Patchwork++ GPU tests compare between a GroundSegmenter and the NumPy restatement (tests/patchwork_restatement.py)."""
import numpy as np
import pytest


def _compare_frame(seg, ref_out, xyz, id, exact_lm=True):
    """Device (last estimate of seg) against one restatement output."""
    dg = seg.diagnostics()
    np.testing.assert_array_equal(dg["point_label"], ref_out["labels"])  # RNR mask and patch ids
    np.testing.assert_array_equal(dg["patch_order"], ref_out["patch_order"])  # per-patch sorted order
    for pd, pr_ in zip(dg["patches"], ref_out["patches"]):
        assert pd["n_points"] == pr_["n_points"] and pd["segment_offset"] == pr_["segment_offset"]
        assert pd["decision"] == pr_["decision"], (pd, pr_["decision"])
        if "fits" not in pr_:
            assert pd["n_fits"] == 0
            continue
        f = pr_["fits"][-1]
        np.testing.assert_array_equal(pd["mean"], f["mean"])
        np.testing.assert_array_equal(pd["cov"], f["cov"].reshape(-1))
        np.testing.assert_allclose(pd["singular_values"], f["sv"], rtol=1e-5, atol=1e-12)
        assert list(pd["fit_points"][:len(pr_["fits"])]) == [q["m"] for q in pr_["fits"]]
        assert list(pd["lm_iterations"][:len(pr_["fits"])]) == [q["iters"] for q in pr_["fits"]]
        assert pd["n_ground"] == pr_["n_ground"]
        if id == 0:
            np.testing.assert_array_equal(pd["normal"], f["normal"])
        else:
            np.testing.assert_allclose(pd["normal"], f["normal"], atol=1e-6)
    fin, fr = dg["frame"], ref_out["final"]
    np.testing.assert_array_equal(fin["final_mean"], fr["mean"])
    np.testing.assert_array_equal(fin["final_cov"], fr["cov"].reshape(-1))
    assert fin["final_lm_iterations"] == fr["iters"] and fin["final_fit_points"] == fr["m"]
    np.testing.assert_allclose(fin["final_normal"], fr["normal"], atol=1e-6)
    np.testing.assert_allclose(fin["final_d"], fr["d"], atol=1e-6)


def _state_equal(seg, ref):
    s, r = seg.get_state(), ref.state()
    np.testing.assert_allclose(s["elevation_thr"], r["elevation_thr"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(s["flatness_thr"], r["flatness_thr"], rtol=1e-9, atol=1e-12)
    assert s["sensor_height"] == pytest.approx(r["sensor_height"], rel=1e-9, abs=1e-12)
    for a, b in zip(s["update_elevation"] + s["update_flatness"], r["update_elevation"] + r["update_flatness"]):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
