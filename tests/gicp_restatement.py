"""NumPy restatement of fast_gicp::FastGICP and fast_gicp::FastVGICP (TEST INFRASTRUCTURE ONLY).

float64 throughout, written after the reference sources (paths relative to fast_apdgicp/include/fast_gicp/gicp of the reference):
  GICP = impl/fast_gicp_impl.hpp       update_correspondences :126-165, linearize :169-231, compute_error :234-257
  VG   = impl/fast_vgicp_impl.hpp      update_correspondences :73-116, linearize :119-180, compute_error :183-204
  VOX  = fast_vgicp_voxel.hpp          neighbor_offsets :10-44, voxels :57-122, GaussianVoxelMap :124-182
  LSQ  = impl/lsq_registration_impl.hpp computeTransformation :55-80, step_gn :107-123, step_lm :127-173
The neighbourhood covariances are not restated here: calculate_covariances is the same code in FastGICP and FastAPDGICP, so the
tests take them from the CPU oracle (oracle.apd.calculate_covariances).  The 6 x 6 LDLT solve and so3_exp of the optimiser shell
are the oracle's exported routines (oracle/apd_oracle.c), whose pivoting and series branches the oracle tests pin.

Order of the sums: pairs enter in (source index, offset index) order; numpy adds them up blockwise, the reference per OpenMP thread --
neither order is a contract, results agree to rounding.  What IS defined to the bit is the transform that feeds voxel_coord:
((m0 x + m1 y) + m2 z) + m3 per row, explicit products and sums (no matmul, which BLAS may fuse or reorder).
"""
import ctypes as C

import numpy as np

DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = 0, 1, 2, 3  # NeighborSearchMethod, gicp_settings.hpp
ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE = 0, 1, 2   # VoxelAccumulationMode


# ------------------------------------------------------------------------------------------------ shared pieces

def transform_points(T, xyz):
    """Eigen Isometry3d * Vector4d for every point (GICP:195, VG:85): rows ((m0 x + m1 y) + m2 z) + m3 * 1, elementwise."""
    T = np.asarray(T, np.float64)
    p = np.asarray(xyz, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.ones((p.shape[0], 4), np.float64)
    for r in range(3):
        a = T[r, 0] * x
        a = a + T[r, 1] * y
        a = a + T[r, 2] * z
        out[:, r] = a + T[r, 3]
    return out


def transform_points_f32(T, xyz):
    """trans.cast<float>() * point (GICP:130, 142): the same order in float32."""
    Tf = np.asarray(T, np.float64).astype(np.float32)
    p = np.asarray(xyz, np.float32)
    out = np.empty((p.shape[0], 3), np.float32)
    for r in range(3):
        a = Tf[r, 0] * p[:, 0]
        a = a + Tf[r, 1] * p[:, 1]
        a = a + Tf[r, 2] * p[:, 2]
        out[:, r] = a + Tf[r, 3]
    return out


def nearest_neighbours(q, tgt, chunk=512):
    """Exact 1-NN under FLANN's float L2_Simple, ((dx dx) + dy dy) + dz dz in float32, ties to the lowest index (GICP:144)."""
    t = np.asarray(tgt, np.float32)
    idx = np.empty(q.shape[0], np.int32)
    sqd = np.empty(q.shape[0], np.float32)
    for s in range(0, q.shape[0], chunk):
        qq = q[s:s + chunk]
        d = None
        for a in range(3):
            diff = qq[:, None, a] - t[None, :, a]
            d = diff * diff if d is None else d + diff * diff
        j = np.argmin(d, axis=1)
        idx[s:s + chunk] = j
        sqd[s:s + chunk] = d[np.arange(qq.shape[0]), j]
    return idx, sqd


def _jacobians(Ta):
    """dtdx0 = [skew(T a) | -I] (GICP:207-209, VG:156-158), N x 4 x 6."""
    n = Ta.shape[0]
    J = np.zeros((n, 4, 6))
    J[:, 0, 1], J[:, 0, 2] = -Ta[:, 2], Ta[:, 1]
    J[:, 1, 0], J[:, 1, 2] = Ta[:, 2], -Ta[:, 0]
    J[:, 2, 0], J[:, 2, 1] = -Ta[:, 1], Ta[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    return J


def _mahalanobis(T, cov_a, cov_b):
    """RCR = cov_B + T cov_A T^T; RCR(3,3) = 1; inverse; (3,3) = 0 (GICP:159-163, VG:110-114), batched 4 x 4."""
    T = np.asarray(T, np.float64)
    rcr = cov_b + np.einsum("ij,njk,lk->nil", T, cov_a, T)
    rcr[:, 3, 3] = 1.0
    m = np.linalg.inv(rcr)
    m[:, 3, 3] = 0.0
    return m


def _accumulate(J, M, e, w):
    MJ = np.einsum("nij,njk->nik", M, J)
    H = np.einsum("n,nji,njk->ik", w, J, MJ)
    Me = np.einsum("nij,nj->ni", M, e)
    b = np.einsum("n,nji,nj->i", w, J, Me)
    err = float(np.sum(w * np.einsum("ni,ni->n", e, Me)))
    return err, H, b


# ------------------------------------------------------------------------------------------------ FastGICP

class Gicp:
    """FastGICP with given covariances.  `nn` (optional): callable (T, src, tgt) -> (index, squared distance) standing in for the
    kd-tree query of GICP:142-144 (any exact float32 search returns the same)."""

    def __init__(self, src, tgt, src_cov, tgt_cov, corr_dist_threshold=np.finfo(np.float32).max, nn=None):
        self.src = np.asarray(src, np.float32)
        self.tgt = np.asarray(tgt, np.float32)
        self.src_cov = np.asarray(src_cov, np.float64)
        self.tgt_cov = np.asarray(tgt_cov, np.float64)
        self.thr = float(corr_dist_threshold)
        self.nn = nn
        self.corr = self.sqd = self.maha = None

    def update_correspondences(self, T):  # GICP:126-165
        if self.nn is not None:
            j, d = self.nn(T, self.src, self.tgt)
        else:
            j, d = nearest_neighbours(transform_points_f32(T, self.src), self.tgt)
        self.sqd = np.asarray(d, np.float32)
        self.corr = np.where(self.sqd.astype(np.float64) < self.thr * self.thr, j, -1).astype(np.int32)  # GICP:148
        ok = self.corr >= 0
        self.maha = np.zeros((self.src.shape[0], 4, 4))
        self.maha[ok] = _mahalanobis(T, self.src_cov[ok], self.tgt_cov[self.corr[ok]])

    def _residuals(self, T):
        ok = np.nonzero(self.corr >= 0)[0]
        Ta = transform_points(T, self.src[ok])
        mean_b = np.concatenate([self.tgt[self.corr[ok]].astype(np.float64), np.ones((ok.size, 1))], axis=1)
        return ok, Ta, mean_b - Ta  # GICP:195-196

    def linearize(self, T):  # GICP:169-231 -> (error, H, b)
        self.update_correspondences(T)
        ok, Ta, e = self._residuals(T)
        return _accumulate(_jacobians(Ta), self.maha[ok], e, np.ones(ok.size))

    def compute_error(self, T):  # GICP:234-257
        ok, _, e = self._residuals(T)
        return float(np.sum(np.einsum("ni,nij,nj->n", e, self.maha[ok], e)))


# ------------------------------------------------------------------------------------------------ Gaussian voxel map

def neighbor_offsets(search):  # VOX:10-44
    if search == DIRECT1:
        return np.array([[0, 0, 0]])
    if search == DIRECT7:
        return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    if search == DIRECT27:
        return np.array([[i - 1, j - 1, k - 1] for i in range(3) for j in range(3) for k in range(3)])
    raise ValueError("unsupported neighbor search method")  # the reference aborts, VOX:13-15


def voxel_coord(p, resolution):
    """(x.array() / voxel_resolution_ - 0.5).floor().cast<int>(), VOX:158-160 (p: N x >= 3 float64)."""
    return np.floor(np.asarray(p, np.float64)[:, :3] / resolution - 0.5).astype(np.int64)


def inverse_cofactor(m):
    """Matrix4d::inverse() of a covariance-shaped matrix (row / column 3 zero but for (3,3)).  Eigen inverts fixed-size 4 x 4 matrices by
    cofactors, adjugate * (1 / determinant), not by an LU factorisation; with the zero row / column the expansion is the 3 x 3 adjugate
    of the block over its determinant (the remaining factors are products with 1 and sums with 0, which are exact) and 1 / m(3,3).
    A LAPACK inverse (numpy.linalg.inv) differs from that by cond(m) * 1e-16 -- 1e-12 and more for the plane-regularised covariances
    (eigenvalues 1, 1, 1e-3), which the information-weighted mean of a multiplicative voxel then carries."""
    a00, a01, a02, a11, a12, a22 = m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    r = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02)
    out = np.zeros((4, 4))
    out[0, 0], out[0, 1], out[0, 2] = c00 * r, c01 * r, c02 * r
    out[1, 1], out[1, 2], out[2, 2] = (a00 * a22 - a02 * a02) * r, (a01 * a02 - a00 * a12) * r, (a00 * a11 - a01 * a01) * r
    out[1, 0], out[2, 0], out[2, 1] = out[0, 1], out[0, 2], out[1, 2]
    out[3, 3] = 1.0 / m[3, 3]
    return out


def _matvec(m, v):
    """Matrix4d * Vector4d, coefficient-wise: ((m0 v0 + m1 v1) + m2 v2) + m3 v3 per row"""
    return np.array([((m[r, 0] * v[0] + m[r, 1] * v[1]) + m[r, 2] * v[2]) + m[r, 3] * v[3] for r in range(4)])


class VoxelMap:
    """GaussianVoxelMap::create_voxelmap (VOX:129-156): a dict keyed by integer triples, points appended in input order.
    Afterwards the voxels as arrays in ascending (x, y, z) coordinate order: coord, num_points, mean (4), cov (4 x 4)."""

    def __init__(self, xyz, covs, resolution, mode=ADDITIVE):
        pts = np.concatenate([np.asarray(xyz, np.float32).astype(np.float64), np.ones((len(xyz), 1))], axis=1)  # getVector4fMap().cast<double>()
        covs = np.asarray(covs, np.float64)
        self.resolution = float(resolution)
        self.mode = mode
        coords = voxel_coord(pts, resolution)
        voxels = {}
        for i in range(pts.shape[0]):
            key = (int(coords[i, 0]), int(coords[i, 1]), int(coords[i, 2]))
            v = voxels.get(key)
            if v is None:
                v = voxels[key] = [0, np.zeros(4), np.zeros((4, 4))]  # GaussianVoxel(): num_points, mean, cov (VOX:62-66)
            v[0] += 1
            if mode in (ADDITIVE, ADDITIVE_WEIGHTED):  # VOX:112-116
                v[1] += pts[i]
                v[2] += covs[i]
            else:  # VOX:86-94
                ci = covs[i].copy()
                ci[3, 3] = 1.0
                ci = inverse_cofactor(ci)
                v[2] += ci
                v[1] += _matvec(ci, pts[i])
        for v in voxels.values():
            if mode in (ADDITIVE, ADDITIVE_WEIGHTED):  # VOX:118-121
                v[1] = v[1] / v[0]
                v[2] = v[2] / v[0]
            else:  # VOX:96-102
                v[2][3, 3] = 1.0
                v[1][3] = 1.0
                v[2] = inverse_cofactor(v[2])
                v[1] = _matvec(v[2], v[1])
        keys = sorted(voxels)
        self.voxels = voxels
        self.index = {k: n for n, k in enumerate(keys)}
        self.coord = np.array(keys, np.int64).reshape(-1, 3)
        self.num_points = np.array([voxels[k][0] for k in keys], np.int64)
        self.mean = np.array([voxels[k][1] for k in keys]).reshape(-1, 4)
        self.cov = np.array([voxels[k][2] for k in keys]).reshape(-1, 4, 4)
        # vectorised lookup_voxel (VOX:167-174): exact match of the integer triple
        self._lo = self.coord.min(axis=0) - 1
        self._dim = self.coord.max(axis=0) + 1 - self._lo + 1
        self._codes = self._encode(self.coord)
        assert np.all(np.diff(self._codes) > 0)

    def _encode(self, c):
        r = c - self._lo
        return (r[:, 0] * self._dim[1] + r[:, 1]) * self._dim[2] + r[:, 2]

    def lookup(self, coords):
        """voxel position in the ascending order, or -1, for every integer triple."""
        c = np.asarray(coords, np.int64)
        inside = np.all((c >= self._lo) & (c < self._lo + self._dim), axis=1)
        code = self._encode(np.where(inside[:, None], c, self._lo))
        pos = np.minimum(np.searchsorted(self._codes, code), self._codes.size - 1)
        return np.where(inside & (self._codes[pos] == code), pos, -1).astype(np.int32)


def _inverse_cofactor_rows(m):
    """inverse_cofactor for a stack [n, 4, 4]: the same expressions element by element, so the same bits"""
    a00, a01, a02, a11, a12, a22 = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2], m[:, 1, 1], m[:, 1, 2], m[:, 2, 2]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    r = 1.0 / (a00 * c00 + a01 * c01 + a02 * c02)
    out = np.zeros(m.shape)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c00 * r, c01 * r, c02 * r
    out[:, 1, 1], out[:, 1, 2], out[:, 2, 2] = (a00 * a22 - a02 * a02) * r, (a01 * a02 - a00 * a12) * r, (a00 * a11 - a01 * a01) * r
    out[:, 1, 0], out[:, 2, 0], out[:, 2, 1] = out[:, 0, 1], out[:, 0, 2], out[:, 1, 2]
    out[:, 3, 3] = 1.0 / m[:, 3, 3]
    return out


def _matvec_rows(m, v):
    """_matvec for stacks [n, 4, 4] and [n, 4]"""
    return ((m[:, :, 0] * v[:, 0:1] + m[:, :, 1] * v[:, 1:2]) + m[:, :, 2] * v[:, 2:3]) + m[:, :, 3] * v[:, 3:4]


class VoxelMapVec(VoxelMap):
    """VoxelMap without the loop over the points, for clouds of 1e5 points and more: the voxels are found by a stable sort of the
    integer triples, and the k-th point of every voxel (in INPUT order) is added in step k -- the additions every voxel sees, and their
    order, are those of VoxelMap, so every array is equal to the bit (tests/test_voxel_scenes.py holds the two together with
    np.array_equal on every scene of at most 4097 points)."""

    def __init__(self, xyz, covs, resolution, mode=ADDITIVE):
        pts = np.concatenate([np.asarray(xyz, np.float32).astype(np.float64), np.ones((len(xyz), 1))], axis=1)
        covs = np.asarray(covs, np.float64)
        self.resolution = float(resolution)
        self.mode = mode
        additive = mode in (ADDITIVE, ADDITIVE_WEIGHTED)
        coords = voxel_coord(pts, resolution)
        n = pts.shape[0]
        order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))  # stable: input order inside a voxel
        sc = coords[order]
        first = np.ones(n, bool)
        first[1:] = (sc[1:] != sc[:-1]).any(axis=1)
        starts = np.nonzero(first)[0]
        counts = np.diff(np.append(starts, n))
        if additive:  # VOX:112-116
            term_c, term_m = covs, pts
        else:  # VOX:86-94
            ci = covs.copy()
            ci[:, 3, 3] = 1.0
            term_c = _inverse_cofactor_rows(ci)
            term_m = _matvec_rows(term_c, pts)
        mean, cov = np.zeros((starts.size, 4)), np.zeros((starts.size, 4, 4))
        for k in range(int(counts.max())):
            m = counts > k
            i = order[starts[m] + k]
            mean[m] += term_m[i]
            cov[m] += term_c[i]
        if additive:  # VOX:118-121
            mean = mean / counts[:, None]
            cov = cov / counts[:, None, None]
        else:  # VOX:96-102
            cov[:, 3, 3] = 1.0
            mean[:, 3] = 1.0
            cov = _inverse_cofactor_rows(cov)
            mean = _matvec_rows(cov, mean)
        self.coord = sc[starts].reshape(-1, 3)
        self.num_points = counts.astype(np.int64)
        self.mean, self.cov = mean, cov
        self._lo = self.coord.min(axis=0) - 1
        self._dim = self.coord.max(axis=0) + 1 - self._lo + 1
        self._codes = self._encode(self.coord)
        assert np.all(np.diff(self._codes) > 0)


# ------------------------------------------------------------------------------------------------ FastVGICP

class Vgicp:
    def __init__(self, src, tgt, src_cov, tgt_cov, resolution=1.0, search=DIRECT1, mode=ADDITIVE, voxelmap=None):
        self.src = np.asarray(src, np.float32)
        self.src_cov = np.asarray(src_cov, np.float64)
        self.offsets = neighbor_offsets(search)
        self.map = voxelmap if voxelmap is not None else VoxelMap(tgt, tgt_cov, resolution, mode)  # VG:120-123
        self.slots = None  # [n_source][n_offsets] voxel position or -1
        self.pairs = self.maha = None

    def slot_table(self, T):  # VG:83-94 in the fixed (source, offset) layout
        coord = voxel_coord(transform_points(T, self.src), self.map.resolution)
        return np.stack([self.map.lookup(coord + off[None, :]) for off in self.offsets], axis=1)

    def update_correspondences(self, T):  # VG:73-116
        self.slots = self.slot_table(T)
        i, o = np.nonzero(self.slots >= 0)  # row-major: (source index, offset index) order
        self.pairs = (i, self.slots[i, o])
        self.maha = _mahalanobis(T, self.src_cov[i], self.map.cov[self.pairs[1]])

    def _residuals(self, T):
        i, v = self.pairs
        Ta = transform_points(T, self.src[i])
        return Ta, self.map.mean[v] - Ta, np.sqrt(self.map.num_points[v].astype(np.float64))  # VG:146-149

    def linearize(self, T):  # VG:119-180
        self.update_correspondences(T)
        Ta, e, w = self._residuals(T)
        return _accumulate(_jacobians(Ta), self.maha, e, w)

    def compute_error(self, T):  # VG:183-204
        _, e, w = self._residuals(T)
        return float(np.sum(w * np.einsum("ni,nij,nj->n", e, self.maha, e)))


# ------------------------------------------------------------------------------------------------ LsqRegistration shell

def _oracle_lib():
    from oracle import apd

    return apd.lib()


def ldlt6_solve(A, rhs):
    A = np.ascontiguousarray(A, np.float64)
    rhs = np.ascontiguousarray(rhs, np.float64)
    x = np.zeros(6)
    _oracle_lib().apdo_ldlt6_solve(A.ctypes.data_as(C.POINTER(C.c_double)), rhs.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_double)))
    return x


def delta_from_d(d):
    """[so3_exp(d[:3]).toRotationMatrix() | d[3:]] (LSQ:117-118, 140-142)."""
    d = np.ascontiguousarray(d, np.float64)
    delta = np.zeros((4, 4))
    _oracle_lib().apdo_delta_from_d(d.ctypes.data_as(C.POINTER(C.c_double)), delta.ctypes.data_as(C.POINTER(C.c_double)))
    return delta


def isom_mul(A, B):
    out = np.eye(4)
    for r in range(3):
        for c in range(3):
            out[r, c] = A[r, 0] * B[0, c] + A[r, 1] * B[1, c] + A[r, 2] * B[2, c]
        out[r, 3] = A[r, 0] * B[0, 3] + A[r, 1] * B[1, 3] + A[r, 2] * B[2, 3] + A[r, 3]
    return out


def is_converged(delta, rotation_epsilon, transformation_epsilon):  # LSQ:83-92
    r = np.abs(delta[:3, :3] - np.eye(3)) * (1.0 / rotation_epsilon)
    t = np.abs(delta[:3, 3]) * (1.0 / transformation_epsilon)
    return max(r.max(), t.max()) < 1.0


def align(reg, guess=None, optimizer="LM", max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4, lm_max_iterations=10,
          lm_init_lambda_factor=1e-9):
    """LsqRegistration::computeTransformation (LSQ:55-80) over an object with linearize(T) / compute_error(T).
    Returns dict(T float32, H, converged, nr_iterations, n_linearize, n_compute_error)."""
    x0 = np.asarray(np.eye(4) if guess is None else guess, np.float32).astype(np.float64)  # LSQ:56
    x0[3] = [0, 0, 0, 1]
    lam = -1.0  # LSQ:58
    converged = False
    nr_iterations = 0
    Hfin = np.eye(6)
    n_lin = n_err = 0
    for it in range(max_iterations):  # LSQ:67
        if converged:
            break
        nr_iterations = it  # LSQ:68
        y0, H, b = reg.linearize(x0)
        n_lin += 1
        ok = False
        if optimizer == "GN":  # LSQ:107-123
            d = ldlt6_solve(H, -b)
            delta = delta_from_d(d)
            x0 = isom_mul(delta, x0)
            Hfin = H.copy()
            ok = True
        else:  # LSQ:127-173
            if lam < 0.0:
                lam = lm_init_lambda_factor * np.abs(np.diag(H)).max()  # LSQ:131-133
            nu = 2.0
            for _ in range(lm_max_iterations):
                d = ldlt6_solve(H + lam * np.eye(6), -b)  # LSQ:137-138
                delta = delta_from_d(d)
                xi = isom_mul(delta, x0)  # LSQ:144
                yi = reg.compute_error(xi)
                n_err += 1
                den = 0.0
                for q in range(6):
                    den += d[q] * (lam * d[q] - b[q])
                rho = (y0 - yi) / den  # LSQ:146
                if rho < 0:  # LSQ:156-164
                    if is_converged(delta, rotation_epsilon, transformation_epsilon):
                        ok = True
                        break
                    lam = nu * lam
                    nu = 2 * nu
                    continue
                x0 = xi  # LSQ:166
                lam = lam * max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3)  # LSQ:167
                Hfin = H.copy()  # LSQ:168
                ok = True
                break
        if not ok:
            break  # "lm not converged!!", LSQ:71-74
        converged = is_converged(delta, rotation_epsilon, transformation_epsilon)  # LSQ:75
    return dict(T=x0.astype(np.float32), H=Hfin, converged=bool(converged), nr_iterations=nr_iterations, n_linearize=n_lin, n_compute_error=n_err)
