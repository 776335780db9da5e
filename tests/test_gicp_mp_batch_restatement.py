"""CPU check of the records in tests/gicp_mp_batch_scenes.py: the restatement alone decides every pass count of the batch with a margin, the
batch holds at least three distinct pass counts, and dense_64_4200 has long neighbour segments at its first and at its last pose."""
import numpy as np

import gicp_mp_batch_scenes as B
import gicp_mp_restatement as R
import search_restatement as sr


def test_pass_counts_are_the_recorded_ones_and_decided_with_a_margin():
    for name in B.BATCH:
        r = B.reference(name)
        assert r["passes"] == B.PASSES[name], name
        for q in r["ratios"]:
            assert q < 0.5 or q > 2.0, (name, r["ratios"])  # float noise cannot flip the pass count
        assert r["clamp_margin"] > 1e-6, name
    assert len(set(B.PASSES.values())) >= 3
    assert B.reference("all_empty")["passes"] == 1 and not B.reference("all_empty")["converged"]


def test_dense_scene_runs_passes_over_long_segments():
    sc, r, rec = B.scenes()[B.DENSE], B.reference(B.DENSE), B.DENSE_RECORD
    assert (r["passes"], r["iterations"], r["converged"]) == (rec["passes"], rec["iterations"], rec["converged"]) and r["passes"] >= 2
    assert sc["source"].shape == (64, 3) and sc["target"].shape == (4500, 3)
    for T in (sc["guess"], r["T"]):
        lens = np.diff(sr.radius(sc["target"], R.transform_points_f32(T, sc["source"]), 0.5)[0])
        assert int((lens > 4096).sum()) == rec["long_segments"]
