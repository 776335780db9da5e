"""NumPy restatement of GORIO_METHOD_ICP, written from the specification in include/gorio_apd.h (not from the kernels):

  search     the exact float32 1-NN of tests/search_restatement.py (un-fused L2_Simple, ties to the lowest index)
  move       ((m0 x + m1 y) + m2 z) + m3 in float32, the working copy moved incrementally
  estimate   Umeyama without scale in float64 from the 17 sums (count, sum d^2, sum q, sum t, sum t q^T), rounded once to float32
  criteria   pcl::registration::DefaultConvergenceCriteria with max_similar = 0 and abs_mse_thr = 1e-12

align() also reports `margin`: the smallest relative margin |a - b| / max(|a|, |b|) by which any floating-point comparison of step 9 was
decided over the whole align (a conjunction that holds counts its weakest member, one that fails its strongest failing member).  A scene
whose margin is tiny could be decided the other way by an implementation that sums in another order."""
import numpy as np

import search_restatement as SR

f32 = np.float32
DBL_MAX = np.finfo(np.float64).max
STATE_NOT_CONVERGED, STATE_ITERATIONS, STATE_TRANSFORM, STATE_ABS_MSE, STATE_REL_MSE, STATE_NO_CORRESPONDENCES = 0, 1, 2, 3, 4, 5
CHUNK = 512


def transform_f(T, P):
    """T [4, 4] float32, P [n, 3] float32 -> [n, 3] float32, every operation rounded to float32."""
    T = np.asarray(T, f32)
    P = np.asarray(P, f32)
    out = np.empty_like(P)
    for r in range(3):
        a = T[r, 0] * P[:, 0]
        a = a + T[r, 1] * P[:, 1]
        a = a + T[r, 2] * P[:, 2]
        out[:, r] = a + T[r, 3]
    return out


def nearest(queries, cloud):
    """(index int32, squared distance float32) of the exact 1-NN of every query; -1 / +inf for a query with a non-finite coordinate."""
    q = np.asarray(queries, f32).reshape(-1, 3)
    idx = np.full(q.shape[0], -1, np.int32)
    sqd = np.full(q.shape[0], np.inf, f32)
    for b in range(0, q.shape[0], CHUNK):
        d = SR.sqdist(q[b:b + CHUNK], cloud)
        j = np.argmin(np.where(np.isnan(d), np.inf, d), axis=1)  # the first minimum: the lowest index
        live = np.isfinite(q[b:b + CHUNK]).all(axis=1)
        rows = np.arange(d.shape[0])
        ok = live & np.isfinite(d[rows, j])
        idx[b:b + CHUNK][ok] = j[ok]
        sqd[b:b + CHUNK][ok] = d[rows, j][ok]
    return idx, sqd


def correspondences(W, target, max_dist, reciprocal):
    """(corr int32 [-1: none], sqd float32 [+inf: none]) of one pass on the moved copy W."""
    idx, sqd = nearest(W, target)
    thr2 = np.float64(max_dist) * np.float64(max_dist)
    with np.errstate(over="ignore"):
        keep = (idx >= 0) & ~(sqd.astype(np.float64) > thr2)
    if reciprocal and keep.any():
        back, _ = nearest(np.asarray(target, f32)[np.where(idx >= 0, idx, 0)], W)
        keep &= back == np.arange(W.shape[0])
    return np.where(keep, idx, -1).astype(np.int32), np.where(keep, sqd, f32(np.inf)).astype(f32)


def sums17(W, target, corr, sqd):
    """count, sum d^2, sum q (3), sum t (3), sum t q^T (9, t along the rows) over the pairs, in float64 (math.fsum-free: plain sums; the
    GPU adds in another order, hence the 1e-9 relative gate of the tests)."""
    m = corr >= 0
    q = np.asarray(W, f32)[m].astype(np.float64)
    t = np.asarray(target, f32)[corr[m]].astype(np.float64)
    s = np.zeros(17, np.float64)
    s[0] = m.sum()
    s[1] = sqd[m].astype(np.float64).sum()
    s[2:5] = q.sum(0)
    s[5:8] = t.sum(0)
    s[8:17] = (t[:, :, None] * q[:, None, :]).sum(0).reshape(9)
    return s


def umeyama(s):
    """The rigid transform of the sums: float64 Umeyama without scale, in the branches of Eigen::umeyama; float32 4x4, rounded once.
    Also returns which branch decided: 'full', 'reflection' (det Sigma < 0), 'rank2' or 'rank2_reflection'."""
    n = s[0]
    qm, tm = s[2:5] / n, s[5:8] / n
    sig = s[8:17].reshape(3, 3) / n - np.outer(tm, qm)
    U, d, Vt = np.linalg.svd(sig)
    S = np.ones(3)
    branch = "full"
    if np.linalg.det(sig) < 0:
        S[2] = -1.0
        branch = "reflection"
    rank = int((d > d[0] * 3 * np.finfo(np.float64).eps).sum()) if d[0] > 0 else 0
    if rank == 2:
        if np.linalg.det(U) * np.linalg.det(Vt) > 0:
            R = U @ Vt
            branch = "rank2"
        else:
            R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
            branch = "rank2_reflection"
    else:
        R = U @ np.diag(S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = tm - R @ qm
    return T.astype(f32), branch


def mul4f(A, B):
    """float32 4x4 product, every sum left to right."""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    C = np.empty((4, 4), f32)
    for r in range(4):
        for c in range(4):
            s = A[r, 0] * B[0, c]
            for k in range(1, 4):
                s = s + A[r, k] * B[k, c]
            C[r, c] = s
    return C


def _rel(a, b):
    m = max(abs(a), abs(b))
    return 1.0 if m == 0.0 and a == b else (abs(a - b) / m if m > 0 else 0.0)


def step(source, target, T, max_dist, reciprocal=False):
    """gorio_apd_icp_step: one pass on T * source."""
    W = transform_f(T, source)
    corr, sqd = correspondences(W, target, max_dist, reciprocal)
    s = sums17(W, target, corr, sqd)
    est = umeyama(s)[0] if s[0] >= 3 else np.eye(4, dtype=f32)
    return dict(W=W, corr=corr, sqd=sqd, sums=s, pairs=int(s[0]), T_est=est)


def align(source, target, guess=None, max_iterations=10, transformation_epsilon=0.0, max_correspondence_distance=np.sqrt(DBL_MAX), use_reciprocal=False,
          euclidean_fitness_epsilon=-DBL_MAX, transformation_rotation_epsilon=0.0):
    """computeTransformation of the specification.  Defaults are pcl::IterativeClosestPoint's constructor values."""
    source, target = np.asarray(source, f32), np.asarray(target, f32)
    final = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32).copy()
    W = transform_f(final, source)
    nr, similar, prev_mse = 0, 0, DBL_MAX
    trans_thr = float(transformation_epsilon)
    rot_thr = float(transformation_rotation_epsilon) if transformation_rotation_epsilon > 0 else 1.0 - float(transformation_epsilon)
    rel_thr, abs_thr, max_similar = float(euclidean_fitness_epsilon), 1e-12, 0
    margin = np.inf
    state, converged = STATE_NOT_CONVERGED, False
    mse, pairs, passes = 0.0, -1, 0
    corr = sqd = None
    while True:
        corr, sqd = correspondences(W, target, max_correspondence_distance, use_reciprocal)
        s = sums17(W, target, corr, sqd)
        pairs = int(s[0])
        passes += 1
        if pairs < 3:
            state = STATE_NO_CORRESPONDENCES
            break
        T, _ = umeyama(s)
        W = transform_f(T, W)
        final = mul4f(T, final)
        nr += 1
        mse = s[1] / s[0]
        if nr >= max_iterations:
            state, converged = STATE_ITERATIONS, True
            break
        is_similar = False
        Td = T.astype(np.float64)
        cos = 0.5 * (((Td[0, 0] + Td[1, 1]) + Td[2, 2]) - 1.0)
        t2 = (Td[0, 3] * Td[0, 3] + Td[1, 3] * Td[1, 3]) + Td[2, 3] * Td[2, 3]
        m_cos, m_t = _rel(cos, rot_thr), _rel(t2, trans_thr)
        both = cos >= rot_thr and t2 <= trans_thr
        margin = min(margin, min(m_cos, m_t) if both else max(m_cos if cos < rot_thr else 0.0, m_t if t2 > trans_thr else 0.0))
        if both:
            if similar >= max_similar:
                state, converged = STATE_TRANSFORM, True
                break
            is_similar = True
        with np.errstate(over="ignore"):
            diff = abs(mse - prev_mse)
            ratio = diff / prev_mse
        margin = min(margin, _rel(diff, abs_thr))
        if diff < abs_thr:
            if similar >= max_similar:
                state, converged = STATE_ABS_MSE, True
                break
            is_similar = True
        margin = min(margin, _rel(ratio, rel_thr))
        if ratio < rel_thr:
            if similar >= max_similar:
                state, converged = STATE_REL_MSE, True
                break
            is_similar = True
        similar = similar + 1 if is_similar else 0
        prev_mse = mse
    return dict(T=final, converged=converged, nr_iterations=nr, state=state, pairs=pairs, mse=float(mse), margin=float(margin), passes=passes, corr=corr, sqd=sqd)
