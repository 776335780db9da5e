"""Deterministic scenes of the FastGICPMultiPoints tests, built from icp_scenes.room / source / target.  Sources of 255, 256, 257 and 513
points (below, at and above one 256-point block, more than two blocks) against targets of 300 and 2 000 points, identity and offset
guesses, the class defaults of fast_gicp_mp_impl.hpp:20-36 unless a scene names another value.  Every align scene is admitted only if the restatement alone decides each
floating-point criterion with a margin (tests/test_gicp_mp_restatement.py checks all of them on the CPU; the GPU tests run every scene,
none is skipped).  Reference runs are computed once per process."""
import functools

import numpy as np

import gicp_mp_restatement as R
import icp_scenes as S

f32 = np.float32
G1 = S.pose([0.02, 0.01, -0.01], [0.0, 0.1, -0.3])
FAR = f32(100.0)


def with_far_points(n, m):
    """source(n, m) with 20 points 100 m away put in the MIDDLE of its first block (positions 100 .. 119): their neighbourhoods are empty."""
    src = S.source(n, m)
    far = S.room(20, 12) + FAR
    return np.concatenate([src[:100], far, src[100:]]).astype(f32)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(source, target, guess, params): params are keyword arguments of gicp_mp_restatement.align."""
    I = np.eye(4, dtype=f32)
    return {
        "id_257_2000": dict(source=S.source(257, 2000), target=S.target(2000), guess=I, params={}),
        "guess_513_2000": dict(source=S.source(513, 2000), target=S.target(2000), guess=G1, params=dict(rotation_epsilon=1e-4, transformation_epsilon=1e-4)),
        "id_256_300": dict(source=S.source(256, 300), target=S.target(300), guess=I, params={}),
        "guess_256_300": dict(source=S.source(256, 300), target=S.target(300), guess=G1, params={}),
        "id_64_300": dict(source=S.source(64, 300), target=S.target(300), guess=I, params={}),
        "guess_255_300_r025": dict(source=S.source(255, 300), target=S.target(300), guess=G1,
                                   params=dict(neighbor_search_radius=0.25, regularization=R.MIN_EIG, rotation_epsilon=1e-4, transformation_epsilon=1e-4)),
        "id_513_300_frob": dict(source=S.source(513, 300), target=S.target(300), guess=I, params=dict(regularization=R.FROBENIUS, k_correspondences=12)),
        # 20 of the source points have no neighbour: they are skipped, the rest align
        "far_points_257": dict(source=with_far_points(257, 2000), target=S.target(2000), guess=I, params={}),
        # the whole source is 100 m away: no neighbourhood at all, the align ends unconverged at the guess with iterations 0
        "all_empty": dict(source=(S.source(64, 300) + FAR).astype(f32), target=S.target(300), guess=G1, params={}),
    }


ALIGN_SCENES = ["id_257_2000", "guess_513_2000", "id_256_300", "guess_256_300", "id_64_300", "guess_255_300_r025", "id_513_300_frob", "far_points_257"]


@functools.lru_cache(maxsize=None)
def reference(name):
    sc = scenes()[name]
    return R.align(sc["source"], sc["target"], sc["guess"], **sc["params"])


def params_of(name):
    p = dict(R.DEFAULTS)
    p.update(scenes()[name]["params"])
    return p


# ------------------------------------------------------------------------------------------------ the cases of the parity checks

def cov_clouds():
    """name -> cloud of the covariance checks: n = k = 20 (the smallest legal cloud) and 255 / 256 / 257 points."""
    return {"room_20": S.room(20, 31), "room_255": S.room(255, 32), "room_256": S.room(256, 33), "room_257": S.room(257, 34)}


def pass_cases():
    """(name, source, target, T, params) of the one-pass checks: every scene at its guess (a pose well away from the optimum, so that g is no
    cancellation)."""
    return [(name, sc["source"], sc["target"], sc["guess"], params_of(name)) for name, sc in scenes().items()]


@functools.lru_cache(maxsize=None)
def pass_reference(name, dtype_name="f32"):
    """The restatement's pass of a case: the float32 form, or its float64 twin on the float32 form's neighbourhoods."""
    sc, p = scenes()[name], params_of(name)
    dt = f32 if dtype_name == "f32" else np.float64
    cs = R.covariances(sc["source"], p["k_correspondences"], p["regularization"], dt)
    ct = R.covariances(sc["target"], p["k_correspondences"], p["regularization"], dt)
    csr = None
    if dtype_name != "f32":
        P = pass_reference(name)
        csr = (P.offsets, P.idx, P.sqd)
    return R.one_pass(sc["source"], cs, sc["target"], ct, sc["guess"], p["neighbor_search_radius"], dt, csr)


def rel(a, b):
    """largest deviation of a from b relative to the scale (largest magnitude) of b"""
    b = np.asarray(b, np.float64)
    s = float(np.max(np.abs(b))) if b.size else 0.0
    return float(np.max(np.abs(np.asarray(a, np.float64) - b))) / s if s > 0 else 0.0


@functools.lru_cache(maxsize=None)
def measured_spreads():
    """Per quantity the largest deviation between the restatement's float32 form and its float64 twin, relative to the quantity's scale:
    covariances over cov_clouds() x the four regularisations, mean_B / cov_B / H / g over pass_cases()."""
    out = dict(cov=0.0, mean_B=0.0, cov_B=0.0, H=0.0, g=0.0)
    for cloud in cov_clouds().values():
        for reg in (R.MIN_EIG, R.NORMALIZED_MIN_EIG, R.PLANE, R.FROBENIUS):
            out["cov"] = max(out["cov"], rel(R.covariances(cloud, 20, reg), R.covariances(cloud, 20, reg, np.float64)))
    for name, *_ in pass_cases():
        a, b = pass_reference(name), pass_reference(name, "f64")
        for q in ("mean_B", "cov_B", "H", "g"):
            out[q] = max(out[q], rel(getattr(a, q), getattr(b, q)))
    return out
