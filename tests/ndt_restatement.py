"""NumPy restatement of pclomp::NormalDistributionsTransform (NDT_OMP), the parity reference of include/gorio_ndt.h.

Paths relative to ndt_omp/include/pclomp of the Go-RIO sources:
  VGC = voxel_grid_covariance_omp_impl.hpp   NDT = ndt_omp_impl.hpp   NDTH = ndt_omp.h

The reference cannot be compiled here (no PCL, no Eigen), so this is "parity unpinned" in DESIGN.md's sense; it is pinned on the CPU
by tests/test_ndt_restatement.py (finite differences, closed cases, known-transform recovery).  Fixed here where the reference leaves
it to a library (the same definitions as include/gorio_ndt.h):
  * float sin / cos / atan2 / exp are the correctly rounded float results (computed in double, rounded once);
  * 3-term float products sum left to right, un-fused; pcl::transformPointCloud is ((m0 x + m1 y) + m2 z) + m3;
  * Transform<float, 3, Affine>::rotation() (NDT:109) is taken as the linear part (exact for an orthonormal guess);
  * DIRECT26 walks the 26 offsets of pcl::getAllNeighborCellIndices (PCL 1.10 voxel_grid.h): no centre cell;
  * the Hessian of computeDerivatives is its upper triangle (hessian(i, j), i <= j, NDT:529) mirrored;
  * JacobiSVD<6x6>::solve: symmetric eigen-decomposition, singular values <= 6 eps sigma_max are zero;
  * non-finite target points are skipped and the bounding box is that of the finite points (VGC:136-138, 213-215).
Reference quirk kept: the float table row d1 holds +sy (NDT:383) where the double one of computeHessian holds -sy (NDT:361).
"""
import numpy as np

f32 = np.float32
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3  # NDTH:52-57
COORD_LIMIT = 1 << 30


class Unsupported(Exception):
    pass


def _half_cells():  # pcl::getHalfNeighborCellIndices
    c = []
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            c.append((i, j, -1))
    for i in (-1, 0, 1):
        c.append((i, -1, 0))
    c.append((-1, 0, 0))
    return c


def offsets(search):
    """Displacement columns in the order of VGC:406-442."""
    if search == DIRECT1:
        return np.zeros((1, 3), np.int64)
    if search == DIRECT7:
        return np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)
    if search == DIRECT26:
        h = np.array(_half_cells(), np.int64)
        return np.concatenate([h, -h])
    raise Unsupported("KDTREE")


class VoxelMap:
    pass


def build_voxel_map(target, resolution, min_points=6, eig_mult=0.01):
    """VoxelGridCovariance::applyFilter, VGC:60-370.  Leaves in ascending linear index (the order of the reference's std::map)."""
    if not resolution > 0:
        raise Unsupported("resolution")
    vm = VoxelMap()
    vm.leaf = f32(resolution)
    vm.inv = f32(1.0) / vm.leaf  # inverse_leaf_size_
    vm.min_points = int(min_points)
    T = np.asarray(target, f32).reshape(-1, 3)
    P = T[np.isfinite(T).all(axis=1)]  # VGC:213-215
    vm.n_leaves = 0
    vm.min_b = np.zeros(3, np.int64)
    vm.max_b = np.zeros(3, np.int64)
    vm.div_b = np.zeros(3, np.int64)
    vm.mul = np.zeros(3, np.int64)
    vm.idx = np.zeros(0, np.int64)
    if P.shape[0] == 0:
        vm.count = np.zeros(0, np.int64)
        vm.mean = np.zeros((0, 3))
        vm.cov_raw = vm.cov = vm.icov = np.zeros((0, 3, 3))
        return vm
    min_p, max_p = P.min(axis=0), P.max(axis=0)
    d = ((max_p - min_p) * vm.inv).astype(np.float64)  # VGC:75-77 (float arithmetic, then int64)
    if np.prod(np.floor(d) + 1.0) > 2147483647.0:      # VGC:79
        raise Unsupported("leaf size too small")
    fmin, fmax = np.floor(min_p * vm.inv), np.floor(max_p * vm.inv)
    if np.abs(fmin).max() >= COORD_LIMIT or np.abs(fmax).max() >= COORD_LIMIT:
        raise Unsupported("coordinates")
    vm.min_b = fmin.astype(np.int64)  # VGC:87-92
    vm.max_b = fmax.astype(np.int64)
    vm.div_b = vm.max_b - vm.min_b + 1
    vm.mul = np.array([1, vm.div_b[0], vm.div_b[0] * vm.div_b[1]], np.int64)  # VGC:103
    ijk = (np.floor(P * vm.inv) - vm.min_b.astype(f32)).astype(np.int64)  # VGC:218-220, float32 throughout
    lin = ijk @ vm.mul                                                   # VGC:223
    order = np.argsort(lin, kind="stable")
    vm.idx, starts, counts = np.unique(lin[order], return_index=True, return_counts=True)
    L = vm.idx.shape[0]
    Pd = P.astype(np.float64)[order]
    S1, S2 = np.zeros((L, 3)), np.zeros((L, 3, 3))
    for k in range(int(counts.max())):  # input order inside every leaf: mean_ += p, cov_ += p p^T (VGC:233-237)
        m = counts > k
        p = Pd[starts[m] + k]
        S1[m] += p
        S2[m] += p[:, :, None] * p[:, None, :]
    n = counts.astype(np.float64)
    mean = S1 / n[:, None]  # VGC:293
    big = counts >= vm.min_points  # VGC:297
    cov_raw = np.zeros((L, 3, 3))
    nb = n[big, None, None]
    c = (S2[big] - 2.0 * (S1[big][:, :, None] * mean[big][:, None, :])) / nb + mean[big][:, :, None] * mean[big][:, None, :]  # VGC:329
    cov_raw[big] = c * ((nb - 1.0) / nb)                                                                                   # VGC:330
    count = counts.astype(np.int64).copy()
    cov = cov_raw.copy()
    icov = np.zeros((L, 3, 3))
    for l in np.nonzero(big)[0]:
        w, V = np.linalg.eigh(cov_raw[l])  # SelfAdjointEigenSolver reads the lower triangle, ascending values (VGC:333-335)
        if w[0] < 0 or w[1] < 0 or w[2] <= 0:  # VGC:337-341
            count[l] = -1
            continue
        lo = eig_mult * w[2]  # VGC:345-356
        if w[0] < lo:
            w[0] = lo
            if w[1] < lo:
                w[1] = lo
            cov[l] = V @ np.diag(w) @ np.linalg.inv(V)
        ic = np.linalg.inv(cov[l])  # VGC:359
        if ic.max() == np.inf or ic.min() == -np.inf:  # VGC:360-364
            count[l] = -1
            continue
        icov[l] = ic
    vm.n_leaves, vm.count, vm.mean, vm.cov_raw, vm.cov, vm.icov = L, count, mean, cov_raw, cov, icov
    return vm


def neighbourhood(vm, q, search):
    """getNeighborhoodAtPoint* (VGC:374-441) for float32 points q [N, 3]: per displacement, the leaf position or -1."""
    q = np.asarray(q, f32).reshape(-1, 3)
    fl = np.floor(q / vm.leaf)  # VGC:379-381, float division
    ok = (np.abs(fl) < COORD_LIMIT).all(axis=1) & np.isfinite(fl).all(axis=1)
    ijk = np.where(ok[:, None], fl, 0).astype(np.int64)
    out = []
    for dsp in offsets(search):
        inside = ok & ((vm.min_b - ijk) <= dsp).all(axis=1) & ((vm.max_b - ijk) >= dsp).all(axis=1)  # VGC:382-392
        pos = np.full(q.shape[0], -1, np.int64)
        if vm.n_leaves:
            lin = (ijk + dsp - vm.min_b) @ vm.mul
            s = np.minimum(np.searchsorted(vm.idx, lin), vm.n_leaves - 1)
            hit = inside & (vm.idx[s] == lin) & (vm.count[s] >= vm.min_points)  # VGC:394-395
            pos[hit] = s[hit]
        out.append(pos)
    return out


def gauss_constants(resolution, outlier_ratio):
    """NDT:89-93; resolution_ is a float member."""
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / float(f32(resolution)) ** 3
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return d1, d2, d3


def angle_tables(p):
    """computeAngleDerivatives (NDT:288-395) in double: j_ang [8, 3], h_ang [15, 3] with the DOUBLE d1 row (NDT:361)."""
    def cs(a):
        return (1.0, 0.0) if abs(a) < 10e-5 else (np.cos(a), np.sin(a))
    cx, sx = cs(p[3])
    cy, sy = cs(p[4])
    cz, sz = cs(p[5])
    ja = np.array([[-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy],
                   [cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy],
                   [-sy * cz, sy * sz, cy],
                   [sx * cy * cz, -sx * cy * sz, sx * sy],
                   [-cx * cy * cz, cx * cy * sz, -cx * sy],
                   [-cy * sz, -cy * cz, 0.0],
                   [cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0.0],
                   [sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0.0]])
    ha = np.array([[-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy],    # a2
                   [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy],   # a3
                   [cx * cy * cz, -cx * cy * sz, cx * sy],                         # b2
                   [sx * cy * cz, -sx * cy * sz, sx * sy],                         # b3
                   [-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0.0],         # c2
                   [cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0.0],         # c3
                   [-cy * cz, cy * sz, -sy],                                       # d1
                   [-sx * sy * cz, sx * sy * sz, sx * cy],                         # d2
                   [cx * sy * cz, -cx * sy * sz, -cx * cy],                        # d3
                   [sy * sz, sy * cz, 0.0],                                        # e1
                   [-sx * cy * sz, -sx * cy * cz, 0.0],                            # e2
                   [cx * cy * sz, cx * cy * cz, 0.0],                              # e3
                   [-cy * cz, cy * sz, 0.0],                                       # f1
                   [-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0.0],        # f2
                   [-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0.0]])       # f3
    return ja, ha


def _sinf(a):
    return f32(np.sin(np.float64(a)))


def _cosf(a):
    return f32(np.cos(np.float64(a)))


def _atan2f(a, b):
    return f32(np.arctan2(np.float64(a), np.float64(b)))


def _angle_axis(angle, axis):
    """AngleAxis<float>::toRotationMatrix (Eigen 3.3.7) about a unit axis."""
    a = np.zeros(3, f32)
    a[axis] = 1.0
    s, c = _sinf(angle), _cosf(angle)
    sa = s * a
    c1 = (f32(1.0) - c) * a
    R = np.zeros((3, 3), f32)
    t = c1[0] * a[1]
    R[0, 1], R[1, 0] = t - sa[2], t + sa[2]
    t = c1[0] * a[2]
    R[0, 2], R[2, 0] = t + sa[1], t - sa[1]
    t = c1[1] * a[2]
    R[1, 2], R[2, 1] = t - sa[0], t + sa[0]
    for k in range(3):
        R[k, k] = c1[k] * a[k] + c
    return R


def _mul3f(A, B):
    C = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return C


def pose_matrix(p):
    """Translation * AngleAxis(X) * AngleAxis(Y) * AngleAxis(Z) in float (NDT:827-830)."""
    pf = np.asarray(p, np.float64).astype(f32)
    T = np.eye(4, dtype=f32)
    T[:3, :3] = _mul3f(_mul3f(_angle_axis(pf[3], 0), _angle_axis(pf[4], 1)), _angle_axis(pf[5], 2))
    T[:3, 3] = pf[:3]
    return T


def euler_angles_012(R):
    """MatrixBase::eulerAngles(0, 1, 2) of a float 3x3 (Eigen 3.3.7 EulerAngles.h)."""
    R = np.asarray(R, f32)
    r0 = _atan2f(R[1, 2], R[2, 2])
    c2 = f32(np.sqrt(R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1]))
    if r0 > 0:
        r0 = r0 - f32(np.pi)
        r1 = _atan2f(-R[0, 2], -c2)
    else:
        r1 = _atan2f(-R[0, 2], c2)
    s1, c1 = _sinf(r0), _cosf(r0)
    r2 = _atan2f(s1 * R[2, 0] - c1 * R[1, 0], c1 * R[1, 1] - s1 * R[2, 1])
    return np.array([-r0, -r1, -r2], f32)


def transform_cloud(T, x):
    """pcl::transformPointCloud in float: ((m0 x + m1 y) + m2 z) + m3."""
    T = np.asarray(T, f32)
    x = np.asarray(x, f32).reshape(-1, 3)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def _dot3(a, b):
    """Left-to-right 3-term dot over the last axis (arrays of any float type)."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# which h_ang rows make the (i, j) block of the point Hessian, i, j in 3..5 (NDT:421-438): first row, rows used, x component present
_HBLOCK = {(3, 3): (0, False), (3, 4): (2, False), (3, 5): (4, False), (4, 4): (6, True), (4, 5): (9, True), (5, 5): (12, True)}


def _point_hessian(xh, i, j):
    """The 3-vector of block (i, j) from x_h_ang [N, 15]; zeros unless both i, j >= 3."""
    if i < 3 or j < 3:
        return None
    r, has_x = _HBLOCK[(min(i, j), max(i, j))]
    z = np.zeros_like(xh[:, 0])
    return np.stack([xh[:, r], xh[:, r + 1], xh[:, r + 2]], axis=1) if has_x else np.stack([z, xh[:, r], xh[:, r + 1]], axis=1)


def derivatives(vm, source, p, search, d1, d2, compute_hessian=True, T=None):
    """computeDerivatives (NDT:180-285) at pose vector p; the cloud is transformed by T (default pose_matrix(p)).
    Returns (score, gradient [6], hessian [6, 6] mirrored upper triangle, n_pairs)."""
    src = np.asarray(source, f32).reshape(-1, 3)
    T = pose_matrix(p) if T is None else np.asarray(T, f32)
    q = transform_cloud(T, src)
    ja, ha = angle_tables(np.asarray(p, np.float64))
    jaf, haf = ja.astype(f32), ha.astype(f32)
    haf[6, 2] = -haf[6, 2]  # NDT:383: the float table holds +sy
    d2f = f32(d2)
    score, g, H, pairs = 0.0, np.zeros(6), np.zeros((6, 6)), 0
    sc_pt, g_pt, H_pt = np.zeros(src.shape[0]), np.zeros((src.shape[0], 6)), np.zeros((src.shape[0], 6, 6))
    for pos in neighbourhood(vm, q, search):
        m = pos >= 0
        if not m.any():
            continue
        x, xt_pt, leaf = src[m], q[m], pos[m]
        pairs += int(m.sum())
        xt = (xt_pt.astype(np.float64) - vm.mean[leaf]).astype(f32)  # NDT:259-262, 492
        C = vm.icov[leaf].astype(f32)                                # NDT:494
        xC = np.stack([_dot3(xt, C[:, :, c]) for c in range(3)], axis=1)  # x_trans4 * c_inv4
        arg = (-d2f * _dot3(xt, xC)) * f32(0.5)
        e = np.exp(arg.astype(np.float64)).astype(f32)               # NDT:499
        inc = (-d1 * e.astype(np.float64)).astype(f32)               # NDT:501, a float
        e = d2f * e
        keep = ~((e > 1) | (e < 0) | np.isnan(e))                    # NDT:506
        e = (e.astype(np.float64) * d1).astype(f32)                  # NDT:510
        xj = np.stack([_dot3(jaf[r][None, :], x) for r in range(8)], axis=1)  # NDT:405
        G = np.zeros((x.shape[0], 3, 6), f32)                        # point_gradient4, NDT:223-224, 407-414
        G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
        G[:, 1, 3], G[:, 2, 3] = xj[:, 0], xj[:, 1]
        G[:, 0, 4], G[:, 1, 4], G[:, 2, 4] = xj[:, 2], xj[:, 3], xj[:, 4]
        G[:, 0, 5], G[:, 1, 5], G[:, 2, 5] = xj[:, 5], xj[:, 6], xj[:, 7]
        CG = np.stack([np.stack([_dot3(C[:, r, :], G[:, :, k]) for k in range(6)], axis=1) for r in range(3)], axis=1)  # [N, 3, 6], NDT:512
        xCG = np.stack([_dot3(xt, CG[:, :, k]) for k in range(6)], axis=1)                                             # NDT:513
        w = keep.astype(np.float64)
        idx = np.nonzero(m)[0]
        sc_pt[idx] += inc.astype(np.float64) * w
        g_pt[idx] += (e[:, None] * xCG).astype(np.float64) * w[:, None]  # NDT:515
        if compute_hessian:
            xh = np.stack([_dot3(haf[r][None, :], x) for r in range(15)], axis=1)  # NDT:418
            for i in range(6):
                for j in range(i, 6):
                    t = (-d2f * xCG[:, i]) * xCG[:, j]
                    h = _point_hessian(xh, i, j)
                    if h is not None:
                        t = t + _dot3(xC, h)  # NDT:525
                    t = t + _dot3(G[:, :, j], CG[:, :, i])  # NDT:519, element (j, i)
                    H_pt[idx, i, j] += (e * t).astype(np.float64) * w  # NDT:529
    score, g, H = sc_pt.sum(), g_pt.sum(axis=0), H_pt.sum(axis=0)  # NDT:278-282
    H = np.triu(H) + np.triu(H, 1).T
    return float(score), g, H, pairs


def hessian_only(vm, source, p, search, d1, d2, T=None):
    """computeHessian / updateHessian (NDT:540-645): double throughout, the double tables."""
    src = np.asarray(source, f32).reshape(-1, 3)
    T = pose_matrix(p) if T is None else np.asarray(T, f32)
    q = transform_cloud(T, src)
    ja, ha = angle_tables(np.asarray(p, np.float64))
    H = np.zeros((6, 6))
    for pos in neighbourhood(vm, q, search):
        m = pos >= 0
        if not m.any():
            continue
        x, leaf = src[m].astype(np.float64), pos[m]
        xt = q[m].astype(np.float64) - vm.mean[leaf]
        C = vm.icov[leaf]
        Cx = np.stack([_dot3(C[:, r, :], xt) for r in range(3)], axis=1)
        e = d2 * np.exp(-d2 * _dot3(xt, Cx) / 2)  # NDT:622
        keep = ~((e > 1) | (e < 0) | np.isnan(e))
        e = np.where(keep, e * d1, 0.0)
        xj = x @ ja.T
        xh = x @ ha.T
        G = np.zeros((x.shape[0], 3, 6))
        G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
        G[:, 1, 3], G[:, 2, 3] = xj[:, 0], xj[:, 1]
        G[:, 0, 4], G[:, 1, 4], G[:, 2, 4] = xj[:, 2], xj[:, 3], xj[:, 4]
        G[:, 0, 5], G[:, 1, 5], G[:, 2, 5] = xj[:, 5], xj[:, 6], xj[:, 7]
        CG = np.einsum("nrc,nck->nrk", C, G)
        xCG = np.einsum("nr,nrk->nk", xt, CG)
        for i in range(6):
            for j in range(i, 6):
                t = -d2 * xCG[:, i] * xCG[:, j] + np.einsum("nr,nr->n", G[:, :, j], CG[:, :, i])
                h = _point_hessian(xh, i, j)
                if h is not None:
                    t = t + np.einsum("nr,nrc,nc->n", xt, C, h)
                H[i, j] += (e * t).sum()
    return np.triu(H) + np.triu(H, 1).T


def calculate_score(vm, source, T, search, d1, d2, d3):
    """calculateScore (NDT:935-983) of the cloud transformed by the float matrix T."""
    src = np.asarray(source, f32).reshape(-1, 3)
    q = transform_cloud(T, src)
    nb = neighbourhood(vm, q, search)
    n_nb = np.sum([pos >= 0 for pos in nb], axis=0)
    score = 0.0
    for pos in nb:
        m = pos >= 0
        if not m.any():
            continue
        xt = q[m].astype(np.float64) - vm.mean[pos[m]]
        C = vm.icov[pos[m]]
        Cx = np.stack([_dot3(C[:, r, :], xt) for r in range(3)], axis=1)
        inc = -d1 * np.exp(-d2 * _dot3(xt, Cx) / 2) - d3
        score += (inc / n_nb[m]).sum()
    return score / float(src.shape[0])


def svd_solve(Hm, b):
    """JacobiSVD<6x6 double>(H).solve(b) for a symmetric H: V |L|^+ sign V^T b, singular values <= 6 eps sigma_max are zero."""
    w, V = np.linalg.eigh(Hm)
    smax = np.abs(w).max()
    keep = np.abs(w) > 6 * np.finfo(np.float64).eps * smax
    y = V.T @ b
    y = np.where(keep, y / np.where(keep, w, 1.0), 0.0)
    return V @ y


def _trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t):
    """trialValueSelectionMT, NDT:689-769 (IEEE arithmetic: a zero denominator gives inf / NaN as in C++)."""
    a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t = (np.float64(v) for v in (a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t))
    with np.errstate(all="ignore"):
        if f_t > f_l:
            z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
            w = np.sqrt(z * z - g_t * g_l)
            a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
            a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t))
            return a_c if abs(a_c - a_l) < abs(a_q - a_l) else 0.5 * (a_q + a_c)
        if g_t * g_l < 0:
            z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
            w = np.sqrt(z * z - g_t * g_l)
            a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
            a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
            return a_c if abs(a_c - a_t) >= abs(a_s - a_t) else a_s
        if abs(g_t) <= abs(g_l):
            z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
            w = np.sqrt(z * z - g_t * g_l)
            a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)
            a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
            nxt = a_c if abs(a_c - a_t) < abs(a_s - a_t) else a_s
            lim = a_t + 0.66 * (a_u - a_t)
            # std::min / std::max (NDT:755-757): a NaN second argument is never selected
            return (nxt if nxt < lim else lim) if a_t > a_l else (nxt if lim < nxt else lim)
        z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u
        w = np.sqrt(z * z - g_t * g_u)
        return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w)


def _update_interval(iv, a_t, f_t, g_t):
    """updateIntervalMT, NDT:648-686; iv = [a_l, f_l, g_l, a_u, f_u, g_u]."""
    if f_t > iv[1]:
        iv[3:6] = [a_t, f_t, g_t]
        return False
    if g_t * (iv[0] - a_t) > 0:
        iv[0:3] = [a_t, f_t, g_t]
        return False
    if g_t * (iv[0] - a_t) < 0:
        iv[3:6] = iv[0:3]
        iv[0:3] = [a_t, f_t, g_t]
        return False
    return True


class Ndt:
    """The registration object: parameters of NDTH, computeTransformation (NDT:81-171) and computeStepLengthMT (NDT:772-932)."""

    def __init__(self, resolution=1.0, step_size=0.1, outlier_ratio=0.55, transformation_epsilon=0.1, max_iterations=35, search=DIRECT7,
                 min_points=6, eig_mult=0.01):
        self.resolution, self.step_size, self.outlier_ratio = resolution, step_size, outlier_ratio
        self.transformation_epsilon, self.max_iterations, self.search = transformation_epsilon, max_iterations, search
        self.min_points, self.eig_mult = min_points, eig_mult
        self.vm = self.source = None
        self.n_eval = self.n_mt = self.n_hessian = 0

    def set_target(self, target):
        self.vm = build_voxel_map(target, self.resolution, self.min_points, self.eig_mult)

    def set_source(self, source):
        self.source = np.asarray(source, f32).reshape(-1, 3)

    def _gauss(self):
        return gauss_constants(self.resolution, self.outlier_ratio)

    def derivatives(self, p, compute_hessian=True, T=None):
        d1, d2, _ = self._gauss()
        self.n_eval += 1
        return derivatives(self.vm, self.source, p, self.search, d1, d2, compute_hessian, T)[:3]

    def _step_length(self, x, step_dir, step_init, step_max, step_min, st):
        """computeStepLengthMT; st holds score, gradient, hessian, T and is updated in place.  Returns (a_t, step_dir)."""
        phi_0 = -st["score"]
        d_phi_0 = -float(st["g"] @ step_dir)
        if d_phi_0 >= 0:
            if d_phi_0 == 0:
                return 0.0, step_dir
            d_phi_0, step_dir = -d_phi_0, -step_dir
        mu, nu = 1.e-4, 0.9
        iv = [0.0, 0.0, d_phi_0 - mu * d_phi_0, 0.0, 0.0, d_phi_0 - mu * d_phi_0]  # psi(0) = 0, psi'(0), NDT:809-816
        interval_converged, open_interval = (step_max - step_min) < 0, True
        a_t = step_max if step_max < step_init else step_init  # std::min(a_t, step_max), NDT:822
        a_t = step_min if a_t < step_min else a_t              # std::max(a_t, step_min)
        x_t = x + step_dir * a_t
        st["T"] = pose_matrix(x_t)
        st["score"], st["g"], st["H"] = self.derivatives(x_t, True)
        phi_t, d_phi_t = -st["score"], -float(st["g"] @ step_dir)
        psi_t, d_psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t, d_phi_t - mu * d_phi_0
        it = 0
        while not interval_converged and it < 10 and not (psi_t <= 0 and d_phi_t <= -nu * d_phi_0):
            a_t = _trial_value(*iv, a_t, psi_t, d_psi_t) if open_interval else _trial_value(*iv, a_t, phi_t, d_phi_t)
            a_t = step_max if step_max < a_t else a_t  # std::min(a_t, step_max), NDT:866: a NaN stays
            a_t = step_min if a_t < step_min else a_t  # std::max(a_t, step_min)
            a_t = float(a_t)
            x_t = x + step_dir * a_t
            st["T"] = pose_matrix(x_t)
            st["score"], st["g"], _ = self.derivatives(x_t, False)
            phi_t, d_phi_t = -st["score"], -float(st["g"] @ step_dir)
            psi_t, d_psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t, d_phi_t - mu * d_phi_0
            if open_interval and psi_t <= 0 and d_psi_t >= 0:
                open_interval = False
                iv[1] = iv[1] + phi_0 - mu * d_phi_0 * iv[0]
                iv[2] = iv[2] + mu * d_phi_0
                iv[4] = iv[4] + phi_0 - mu * d_phi_0 * iv[3]
                iv[5] = iv[5] + mu * d_phi_0
            interval_converged = _update_interval(iv, a_t, psi_t, d_psi_t) if open_interval else _update_interval(iv, a_t, phi_t, d_phi_t)
            it += 1
        if it:  # NDT:928-929
            d1, d2, _ = self._gauss()
            st["H"] = hessian_only(self.vm, self.source, x_t, self.search, d1, d2)
            self.n_hessian += 1
        self.n_mt += it
        return a_t, step_dir

    def align(self, guess=None):
        """computeTransformation.  Returns a dict: T (float32 4x4), converged, nr_iterations, trans_probability, n_derivatives
        (computeDerivatives calls), n_hessians (computeHessian calls), n_mt (More-Thuente inner iterations)."""
        self.n_eval = self.n_mt = self.n_hessian = 0
        guess = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32)
        T = guess.copy()  # NDT:95-104 (identity when the guess is the identity)
        p = np.concatenate([T[:3, 3], euler_angles_012(T[:3, :3])]).astype(np.float64)  # NDT:107-111
        st = {"T": T}
        st["score"], st["g"], st["H"] = self.derivatives(p, True, T=T)  # NDT:119: the cloud moved by the guess itself
        nr, converged, n = 0, False, float(self.source.shape[0])
        while not converged:
            delta = svd_solve(st["H"], -st["g"])  # NDT:127-129
            norm = float(np.sqrt((delta * delta).sum()))
            if norm == 0 or norm != norm:  # NDT:134-139
                return self._result(st, norm == norm, nr, st["score"] / n)
            delta = delta / norm
            norm, delta = self._step_length(p, delta, norm, self.step_size, self.transformation_epsilon / 2, st)
            delta = delta * norm
            p = p + delta
            if nr > self.max_iterations or (nr and abs(norm) < self.transformation_epsilon):  # NDT:158-162
                converged = True
            nr += 1
        return self._result(st, True, nr, st["score"] / n)

    def _result(self, st, converged, nr, prob):
        return {"T": st["T"].copy(), "converged": bool(converged), "nr_iterations": nr, "trans_probability": prob, "n_derivatives": self.n_eval,
                "n_hessians": self.n_hessian, "n_mt": self.n_mt, "score": st["score"]}
