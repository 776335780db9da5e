"""NumPy restatement of GORIO_METHOD_GICP_MP (include/gorio_apd.h): fast_gicp::FastGICPMultiPoints as this library defines it, written from the
header's text, not from the kernels.

Reference lines (paths relative to the reference's fast_apdgicp/): MPH / MPI = include/fast_gicp/gicp/experimental/fast_gicp_mp.hpp and
fast_gicp_mp_impl.hpp.

Every float32 operation is written out element-wise in ONE order (NumPy rounds every float32 product and sum on its own, nothing is fused).
The k-NN lists and the neighbourhoods are search_restatement.knn / radius.  Functions that take `dtype` run their float stages in that type:
float32 is the definition, float64 the TWIN that only measures how far rounding can move a quantity (the neighbourhoods, the weights and
the fp64 sums are the same in both).  Covariances travel as six numbers (00 01 02 11 12 22).
"""
import math

import numpy as np

import search_restatement as sr

F = np.float32
D = np.float64
NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS = 0, 1, 2, 3, 4  # gorio_regularization
UP = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
DEFAULTS = dict(k_correspondences=20, regularization=PLANE, max_iterations=64, rotation_epsilon=1e-5, transformation_epsilon=1e-5, neighbor_search_radius=0.5)  # MPI:20-36


def full3(c6):
    """[n, 6] -> [n, 3, 3]"""
    out = np.empty(c6.shape[:-1] + (3, 3), c6.dtype)
    for t, (a, b) in enumerate(UP):
        out[..., a, b] = c6[..., t]
        out[..., b, a] = c6[..., t]
    return out


# ------------------------------------------------------------------------------------------------ covariances (MPI:225-276)

def raw_covariances(cloud, k, dtype=F):
    """[n, 6] of the k-NN lists (self included), NOT divided by k: s += p; mean = s / k; cov_ab += d_a d_b in list order."""
    p = np.ascontiguousarray(cloud, F)
    lists = sr.knn(p, None, k)[0]
    p = p.astype(dtype)
    n = p.shape[0]
    s = np.zeros((n, 3), dtype)
    for t in range(k):
        s = s + p[lists[:, t]]
    mean = s / dtype(k)
    cov = np.zeros((n, 6), dtype)
    for t in range(k):
        d = p[lists[:, t]] - mean
        for c, (a, b) in enumerate(UP):
            cov[:, c] = cov[:, c] + d[:, a] * d[:, b]
    return cov


def regularize(raw6, reg, dtype=F):
    """[n, 6] regularised covariances of the raw ones, rounded to dtype once."""
    if reg == NONE:
        raise ValueError("NONE is refused (the reference aborts, MPI:255-257)")
    c = full3(raw6.astype(D))
    if reg == FROBENIUS:
        X = np.linalg.inv(c + 1e-3 * np.eye(3))
        f = np.sqrt((X * X).sum(axis=(1, 2)))
        out = np.linalg.inv(X / f[:, None, None])
    else:
        w, v = np.linalg.eigh(c)  # ascending
        w, v = w[:, ::-1], v[:, :, ::-1]
        s = np.abs(w.astype(dtype))
        if reg == PLANE:
            val = np.broadcast_to(np.array([1.0, 1.0, 1e-3], F).astype(dtype), s.shape)
        elif reg == MIN_EIG:
            val = np.maximum(s, dtype(F(1e-3)))
        else:
            val = np.maximum(s / s.max(axis=1, keepdims=True), dtype(F(1e-3)))
        out = np.einsum("nk,nak,nbk->nab", val.astype(D), v, v)
    return np.stack([out[:, a, b] for a, b in UP], axis=1).astype(dtype)


def covariances(cloud, k=20, reg=PLANE, dtype=F):
    return regularize(raw_covariances(cloud, k, dtype), reg, dtype)


# ------------------------------------------------------------------------------------------------ exp / log, the float transform

def so3_exp(w):
    """Rodrigues in double: I + A K + B K^2, K^2 = w w^T - t2 I."""
    w = [float(x) for x in w]
    t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if t2 < 1e-12:
        A, B = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        t = math.sqrt(t2)
        sh = math.sin(0.5 * t)
        A, B = math.sin(t) / t, 2.0 * sh * sh / t2
    K = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    R = np.empty((3, 3), D)
    for r in range(3):
        for c in range(3):
            R[r, c] = ((1.0 if r == c else 0.0) + A * K[r][c]) + B * (w[r] * w[c] - (t2 if r == c else 0.0))
    return R


def so3_log(R):
    R = np.asarray(R, D)
    v = [0.5 * (R[2, 1] - R[1, 2]), 0.5 * (R[0, 2] - R[2, 0]), 0.5 * (R[1, 0] - R[0, 1])]
    c = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    s = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    t = math.atan2(s, c)
    f = 1.0 + t * t / 6.0 if s < 1e-6 else t / s
    return np.array([f * v[0], f * v[1], f * v[2]], D)


def trans_of(x):
    """[float(exp(x.head)) | x.tail] as a float32 4 x 4 (MPI:131-133)."""
    T = np.eye(4, dtype=F)
    T[:3, :3] = so3_exp(x[:3]).astype(F)
    T[:3, 3] = x[3:]
    return T


def transform_points_f32(T, pts, dtype=F):
    """((m0 x + m1 y) + m2 z) + m3, the float transform of the GICP family."""
    T = np.asarray(T, F).astype(dtype)
    p = np.asarray(pts, F).astype(dtype)
    out = np.empty_like(p)
    for r in range(3):
        out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    return out


# ------------------------------------------------------------------------------------------------ one pass (MPI:130-221)

def block_sums(vals):
    """[n, m] per-point float64 values -> [m]: the halving tree of a 64-lane wave, (w0 + w1) + (w2 + w3) per 256-point block, blocks in order."""
    n, m = vals.shape
    nb = (n + 255) // 256
    v = np.zeros((nb * 256, m), D)
    v[:n] = vals
    v = v.reshape(nb, 4, 64, m)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[:, :, :off] + v[:, :, off:2 * off]
    w = v[:, :, 0]
    blk = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    out = np.zeros(m, D)
    for b in range(nb):
        out = out + blk[b]
    return out


class Pass:
    """Everything one pass leaves: q, the CSR, weights' margin, mean_B / cov_B, used, H, g."""


def one_pass(source, src_cov6, target, tgt_cov6, T, radius=0.5, dtype=F, csr=None):
    """A pass at the float pose T.  csr: the neighbourhoods to use (the float64 twin takes the float32 form's)."""
    src = np.ascontiguousarray(source, F)
    tgt = np.ascontiguousarray(target, F)
    T = np.asarray(T, F)
    n = src.shape[0]
    P = Pass()
    P.q = transform_points_f32(T, src)
    P.offsets, P.idx, P.sqd = sr.radius(tgt, P.q, radius) if csr is None else csr
    lens = np.diff(P.offsets)
    P.used = lens > 0
    # the merge: double sums in the neighbours' order
    sw = np.zeros(n, D)
    sm = np.zeros((n, 3), D)
    sc = np.zeros((n, 6), D)
    wraw = 1.0 - np.sqrt(P.sqd).astype(D) / D(radius)  # the square root is the float32 one (MPI:184)
    P.clamp_margin = float(np.min(np.abs(wraw - 1e-3) / 1e-3)) if wraw.size else np.inf
    wj = np.maximum(1e-3, np.minimum(1.0, wraw))
    tp = tgt.astype(D)
    tc = np.asarray(tgt_cov6).astype(dtype).astype(D)
    for t in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > t)[0]
        j = P.offsets[rows] + t
        w = wj[j]
        sw[rows] = sw[rows] + w
        sm[rows] = sm[rows] + w[:, None] * tp[P.idx[j]]
        sc[rows] = sc[rows] + w[:, None] * tc[P.idx[j]]
    u = np.nonzero(P.used)[0]
    P.mean_B = np.zeros((n, 3), dtype)
    P.cov_B = np.zeros((n, 6), dtype)
    P.mean_B[u] = (sm[u] / sw[u, None]).astype(dtype)
    P.cov_B[u] = (sc[u] / sw[u, None]).astype(dtype)
    # the term, in dtype
    a = (P.q if dtype is F else transform_points_f32(T, src, dtype))[u]
    d = P.mean_B[u] - a
    A = full3(np.asarray(src_cov6).astype(dtype)[u])
    B = full3(P.cov_B[u])
    R = T[:3, :3].astype(dtype)
    m = a.shape[0]
    M = np.empty((m, 3, 3), dtype)
    Q = np.empty((m, 3, 3), dtype)
    for r in range(3):
        for c in range(3):
            M[:, r, c] = (R[r, 0] * A[:, 0, c] + R[r, 1] * A[:, 1, c]) + R[r, 2] * A[:, 2, c]
    for r in range(3):
        for c in range(3):
            Q[:, r, c] = B[:, r, c] + ((M[:, r, 0] * R[c, 0] + M[:, r, 1] * R[c, 1]) + M[:, r, 2] * R[c, 2])
    C = np.empty((m, 3, 3), dtype)
    C[:, 0, 0] = Q[:, 1, 1] * Q[:, 2, 2] - Q[:, 1, 2] * Q[:, 2, 1]
    C[:, 0, 1] = Q[:, 0, 2] * Q[:, 2, 1] - Q[:, 0, 1] * Q[:, 2, 2]
    C[:, 0, 2] = Q[:, 0, 1] * Q[:, 1, 2] - Q[:, 0, 2] * Q[:, 1, 1]
    C[:, 1, 0] = Q[:, 1, 2] * Q[:, 2, 0] - Q[:, 1, 0] * Q[:, 2, 2]
    C[:, 1, 1] = Q[:, 0, 0] * Q[:, 2, 2] - Q[:, 0, 2] * Q[:, 2, 0]
    C[:, 1, 2] = Q[:, 0, 2] * Q[:, 1, 0] - Q[:, 0, 0] * Q[:, 1, 2]
    C[:, 2, 0] = Q[:, 1, 0] * Q[:, 2, 1] - Q[:, 1, 1] * Q[:, 2, 0]
    C[:, 2, 1] = Q[:, 0, 1] * Q[:, 2, 0] - Q[:, 0, 0] * Q[:, 2, 1]
    C[:, 2, 2] = Q[:, 0, 0] * Q[:, 1, 1] - Q[:, 0, 1] * Q[:, 1, 0]
    det = (Q[:, 0, 0] * C[:, 0, 0] + Q[:, 0, 1] * C[:, 1, 0]) + Q[:, 0, 2] * C[:, 2, 0]
    C = C / det[:, None, None]
    z = np.zeros(m, dtype)
    S = np.empty((m, 3, 3), dtype)  # skew(trans a)
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2] = z, -a[:, 2], a[:, 1]
    S[:, 1, 0], S[:, 1, 1], S[:, 1, 2] = a[:, 2], z, -a[:, 0]
    S[:, 2, 0], S[:, 2, 1], S[:, 2, 2] = -a[:, 1], a[:, 0], z
    res = np.empty((m, 3), dtype)
    J = np.empty((m, 3, 6), dtype)
    for r in range(3):
        res[:, r] = (C[:, r, 0] * d[:, 0] + C[:, r, 1] * d[:, 1]) + C[:, r, 2] * d[:, 2]
        for c in range(3):
            J[:, r, c] = (C[:, r, 0] * S[:, 0, c] + C[:, r, 1] * S[:, 1, c]) + C[:, r, 2] * S[:, 2, c]
            J[:, r, 3 + c] = -C[:, r, c]
    Jd, rd = J.astype(D), res.astype(D)
    vals = np.zeros((n, 28), D)
    t = 0
    for r in range(6):
        for c in range(r, 6):
            vals[u, t] = (Jd[:, 0, r] * Jd[:, 0, c] + Jd[:, 1, r] * Jd[:, 1, c]) + Jd[:, 2, r] * Jd[:, 2, c]
            t += 1
    for r in range(6):
        vals[u, 21 + r] = (Jd[:, 0, r] * rd[:, 0] + Jd[:, 1, r] * rd[:, 1]) + Jd[:, 2, r] * rd[:, 2]
    vals[u, 27] = 1.0
    sums = block_sums(vals)
    P.H = np.zeros((6, 6), D)
    t = 0
    for r in range(6):
        for c in range(r, 6):
            P.H[r, c] = P.H[c, r] = sums[t]
            t += 1
    P.g = sums[21:27].copy()
    P.n_used = int(sums[27])
    return P


# ------------------------------------------------------------------------------------------------ the shell (MPI:80-127)

def ldlt6_solve(A_in, rhs):
    """Eigen::LDLT<6x6>(A).solve(rhs) as this library's kernels and host code run it: symmetric diagonal pivoting, zero pivots skipped."""
    A = np.array(A_in, D).reshape(6, 6).copy()
    perm = list(range(6))
    for k in range(6):
        piv = k
        best = abs(A[k, k])
        for i in range(k + 1, 6):
            if abs(A[i, i]) > best:
                best, piv = abs(A[i, i]), i
        if piv != k:
            A[[k, piv], :] = A[[piv, k], :]
            A[:, [k, piv]] = A[:, [piv, k]]
            perm[k], perm[piv] = perm[piv], perm[k]
        d = A[k, k]
        if d == 0.0:
            continue
        col = A[:, k].copy()
        for i in range(k + 1, 6):
            l = col[i] / d
            for j in range(k + 1, i + 1):
                A[i, j] -= l * col[j]
            A[i, k] = l
        for i in range(k + 1, 6):
            for j in range(i + 1, 6):
                A[i, j] = A[j, i]
    y = np.array([rhs[perm[i]] for i in range(6)], D)
    for i in range(6):
        for j in range(i):
            y[i] -= A[i, j] * y[j]
    for i in range(6):
        y[i] = y[i] / A[i, i] if A[i, i] != 0.0 else 0.0
    for i in range(5, -1, -1):
        for j in range(i + 1, 6):
            y[i] -= A[j, i] * y[j]
    x = np.zeros(6, D)
    for i in range(6):
        x[perm[i]] = y[i]
    return x


def convergence_ratio(delta, rotation_epsilon, transformation_epsilon):
    """max(|float(exp(delta.head)) - I| (float)(1 / rotation_epsilon), |delta.tail| (float)(1 / transformation_epsilon)), in float32."""
    Rm = np.abs(so3_exp(delta[:3]).astype(F) - np.eye(3, dtype=F))
    r = F(1.0 / rotation_epsilon) * Rm
    t = F(1.0 / transformation_epsilon) * np.abs(np.asarray(delta[3:], F))
    return float(max(r.max(), t.max()))


def align(source, target, guess=None, k_correspondences=20, regularization=PLANE, max_iterations=64, rotation_epsilon=1e-5, transformation_epsilon=1e-5,
          neighbor_search_radius=0.5):
    """computeTransformation (MPI:80-115) -> dict(T, converged, iterations, passes, ratios, clamp_margin, used, H)."""
    src = np.ascontiguousarray(source, F)
    tgt = np.ascontiguousarray(target, F)
    g = np.eye(4, dtype=F) if guess is None else np.asarray(guess, F)
    cs = covariances(src, k_correspondences, regularization)
    ct = covariances(tgt, k_correspondences, regularization)
    x0 = np.concatenate([so3_log(g[:3, :3].astype(D)).astype(F), g[:3, 3]]).astype(F)
    conv, nr, passes = False, 0, 0
    ratios, margins, used = [], [], []
    H = np.zeros((6, 6), D)
    for i in range(max_iterations):
        nr = i
        P = one_pass(src, cs, tgt, ct, trans_of(x0), neighbor_search_radius)
        passes += 1
        H = P.H
        used.append(P.n_used)
        margins.append(P.clamp_margin)
        if P.n_used == 0:
            break
        delta = ldlt6_solve(P.H, P.g).astype(F)
        if not np.isfinite(delta).all():
            break
        Rn = _mul3(so3_exp(-delta[:3].astype(D)), so3_exp(x0[:3].astype(D)))
        x0 = np.concatenate([so3_log(Rn).astype(F), x0[3:] - delta[3:]]).astype(F)
        ratios.append(convergence_ratio(delta, rotation_epsilon, transformation_epsilon))
        if ratios[-1] < 1.0:
            conv = True
            break
    return dict(T=trans_of(x0), converged=conv, iterations=nr, passes=passes, ratios=ratios, clamp_margin=min(margins) if margins else np.inf, used=used, H=H)


def _mul3(a, b):
    """3 x 3 product in double, every entry (a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c."""
    out = np.empty((3, 3), D)
    for r in range(3):
        for c in range(3):
            out[r, c] = (a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]
    return out
