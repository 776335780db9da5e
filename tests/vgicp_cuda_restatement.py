"""NumPy restatement of GORIO_METHOD_VGICP_CUDA (include/gorio_apd.h): fast_gicp::FastVGICPCuda as this library defines it.

Reference lines (paths relative to the reference's fast_apdgicp/):
  VH / VI = include/fast_gicp/gicp/fast_vgicp_cuda.hpp and impl/fast_vgicp_cuda_impl.hpp   VC = src/fast_gicp/cuda/fast_vgicp_cuda.cu
  CE = src/fast_gicp/cuda/covariance_estimation.cu        RB = src/fast_gicp/cuda/covariance_estimation_rbf.cu
  CR = src/fast_gicp/cuda/covariance_regularization.cu    GV = src/fast_gicp/cuda/gaussian_voxelmap.cu
  FV = src/fast_gicp/cuda/find_voxel_correspondences.cu   CD = src/fast_gicp/cuda/compute_derivatives.cu

Every float32 operation is written out element-wise in ONE order (NumPy rounds every float32 product and sum on its own, nothing is
fused).  The float coordinate rule, the offset tables, the pair search, the packed voxel order and the LsqRegistration shell with its trace
are the ones of tests/ndt_cuda_restatement.py; what is restated here is this method's own arithmetic.  Covariances travel as six floats
(00 01 02 11 12 22).
"""
import numpy as np

import ndt_cuda_restatement as nr

F = np.float32
CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL = 0, 1, 2  # VH:21
NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS = 0, 1, 2, 3, 4  # gorio_regularization
DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = nr.DIRECT27, nr.DIRECT7, nr.DIRECT1, nr.DIRECT_RADIUS
RBF_BLOCK = 512  # RB:116
PLANE_RATIO = 0.1  # CR:29
UP = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


# ------------------------------------------------------------------------------------------------ k-NN lists and covariances (CE:26-34)

def sqdist(q, t, dtype=F):
    """[nq, nt] squared distances, (dx dx + dy dy) + dz dz."""
    d = q[:, None, :].astype(dtype) - t[None, :, :].astype(dtype)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn(cloud, k, chunk=512):
    """[n, k] neighbours of every point in its own cloud in ascending (float32 distance, index) order, the point itself included."""
    cloud = np.ascontiguousarray(cloud, F)
    out = np.empty((cloud.shape[0], k), np.int64)
    for a in range(0, cloud.shape[0], chunk):
        out[a:a + chunk] = np.argsort(sqdist(cloud[a:a + chunk], cloud), axis=1, kind="stable")[:, :k]
    return out


def cov_knn(cloud, lists, dtype=F):
    """[n, 6]: mean += p, S_ab += p_a p_b in list order; mean /= k; cov_ab = S_ab / k - mean_a mean_b."""
    p = np.ascontiguousarray(cloud, F).astype(dtype)
    n, k = lists.shape
    mean = np.zeros((n, 3), dtype)
    S = np.zeros((n, 6), dtype)
    for t in range(k):
        q = p[lists[:, t]]
        mean = mean + q
        for c, (a, b) in enumerate(UP):
            S[:, c] = S[:, c] + q[:, a] * q[:, b]
    fk = dtype(k)
    mean = mean / fk
    out = np.empty((n, 6), dtype)
    for c, (a, b) in enumerate(UP):
        out[:, c] = S[:, c] / fk - mean[:, a] * mean[:, b]
    return out


# ------------------------------------------------------------------------------------------------ RBF covariances (RB:67-151)

def max_dist(kernel_width, kernel_max_dist):
    return kernel_max_dist if kernel_max_dist > 0.0 else 5.0 * kernel_width  # VI:46-50


def cov_rbf(cloud, kernel_width, kernel_max_dist, dtype=F, pad=True):
    """[n, 6].  The cloud is extended with points at the origin to a multiple of 512 (pad=False: the un-quirked rule, for the test of the
    quirk); per point and per block of 512 the weighted moments start from zero and run in index order; the block partials are added in
    block order; mean = s / sw, cov_ab = (S_ab - mean_a s_b) / sw."""
    x = np.ascontiguousarray(cloud, F).astype(dtype)
    n = x.shape[0]
    g = dtype(F(kernel_width))
    md = dtype(F(max_dist(kernel_width, kernel_max_dist)))
    m2 = md * md
    nb = (n + RBF_BLOCK - 1) // RBF_BLOCK
    ext = np.zeros((nb * RBF_BLOCK if pad else n, 3), dtype)
    ext[:n] = x
    tot = np.zeros((n, 10), dtype)
    for b in range(nb):
        part = np.zeros((n, 10), dtype)
        for j in range(b * RBF_BLOCK, min((b + 1) * RBF_BLOCK, ext.shape[0])):
            p = ext[j]
            d = x - p[None, :]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            live = np.flatnonzero(~(d2 > m2))
            if live.size == 0:
                continue
            w = np.exp(-g * d2[live])
            wp = [w * p[a] for a in range(3)]
            part[live, 0] = part[live, 0] + w
            for a in range(3):
                part[live, 1 + a] = part[live, 1 + a] + wp[a]
            for c, (a, b_) in enumerate(UP):
                part[live, 4 + c] = part[live, 4 + c] + wp[a] * p[b_]
        tot = tot + part
    sw = tot[:, 0]
    s = tot[:, 1:4]
    mean = s / sw[:, None]
    out = np.empty((n, 6), dtype)
    for c, (a, b_) in enumerate(UP):
        out[:, c] = (tot[:, 4 + c] - mean[:, a] * s[:, b_]) / sw
    return out


# ------------------------------------------------------------------------------------------------ regularisation (CR:91-117)

def full(c6):
    c6 = np.asarray(c6)
    m = np.empty(c6.shape[:-1] + (3, 3), c6.dtype)
    for c, (a, b) in enumerate(UP):
        m[..., a, b] = c6[..., c]
        m[..., b, a] = c6[..., c]
    return m


def six(m):
    return np.stack([m[..., a, b] for a, b in UP], axis=-1)


def plane_ratio(raw6):
    """w1 / w2 of every raw covariance (eigenvalues ascending), the quantity CR:29 compares with 0.1"""
    w = np.linalg.eigvalsh(full(np.asarray(raw6, F).astype(np.float64)))
    with np.errstate(all="ignore"):
        return w[:, 1] / w[:, 2]


def regularize(raw6, method):
    """(keep [n] bool, cov [n, 6] float32): the rebuilt covariance of EVERY point (the caller drops the filtered ones)."""
    raw6 = np.asarray(raw6, F)
    a = full(raw6.astype(np.float64))
    n = a.shape[0]
    keep = np.ones(n, bool)
    if method in (NONE, NORMALIZED_MIN_EIG):  # CR:114-116: "unimplemented", the matrices stay
        return keep, raw6.copy()
    if method == FROBENIUS:
        C = a + 1e-3 * np.eye(3)
        fro = np.sqrt((np.linalg.inv(C) ** 2).sum(axis=(1, 2))) if n else np.zeros(0)
        return keep, six(fro[:, None, None] * C).astype(F)
    w, V = np.linalg.eigh(a) if n else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    if method == PLANE:
        keep = w[:, 1] > w[:, 2] * PLANE_RATIO
        lam = np.broadcast_to(np.array([1e-3, 1.0, 1.0]), w.shape)
    else:
        lam = np.maximum(w, 1e-3)
    return keep, six(np.einsum("nik,nk,njk->nij", V, lam, V)).astype(F)


# ------------------------------------------------------------------------------------------------ the map of the kept points (GV:229-252)

def build_map(points, cov6, resolution):
    """the dict of nr.build_map (without cov_raw) over the kept points: per voxel, in kept order, in float32, n, s += p, Csum += cov;
    mean = s / n, cov = Csum / n.  `cov` is kept as [nv, 3, 3] (what nr.pair_terms reads) and as cov6."""
    pts = np.ascontiguousarray(points, F).reshape(-1, 3)
    cov6 = np.ascontiguousarray(cov6, F).reshape(-1, 6)
    if pts.shape[0] == 0:
        z = np.zeros
        return dict(coord=z((0, 3), np.int64), num_points=z(0, np.int32), mean=z((0, 3), F), cov=z((0, 3, 3), F), cov6=z((0, 6), F), key=z(0, np.int64), res=F(resolution))
    c = nr.voxel_coord(pts, resolution)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))  # stable: kept order inside a voxel
    cs = c[order]
    start = np.flatnonzero(np.r_[True, np.any(cs[1:] != cs[:-1], axis=1)])
    cnt = np.diff(np.r_[start, len(order)])
    nv = len(start)
    s = np.zeros((nv, 3), F)
    C = np.zeros((nv, 6), F)
    for k in range(int(cnt.max())):
        idx = np.flatnonzero(cnt > k)
        sel = order[start[idx] + k]
        s[idx] = s[idx] + pts[sel]
        C[idx] = C[idx] + cov6[sel]
    fn = cnt.astype(F)
    coord = cs[start]
    c6 = C / fn[:, None]
    return dict(coord=coord, num_points=cnt.astype(np.int32), mean=s / fn[:, None], cov=full(c6), cov6=c6, key=nr._pack(coord), res=F(resolution))


def map_from_tables(tab, resolution):
    """a map dict from the arrays of the GPU's parity hook (ApdGicp.vgicp_cuda_voxels)"""
    coord = np.asarray(tab["coord"], np.int64).reshape(-1, 3)
    c6 = np.asarray(tab["cov"], F).reshape(-1, 6)
    return dict(coord=coord, num_points=np.asarray(tab["num_points"], np.int32), mean=np.asarray(tab["mean"], F).reshape(-1, 3), cov=full(c6), cov6=c6,
                key=nr._pack(coord) if len(coord) else np.zeros(0, np.int64), res=F(resolution))


# ------------------------------------------------------------------------------------------------ pairs and terms (FV; CD:50-92, 106-135)

def find_pairs(T, items, tmap, offs):
    if len(tmap["key"]) == 0 or len(items) == 0:
        return np.zeros((0, 2), np.int64)
    return nr.find_pairs(T, items, tmap, offs)


def pair_terms(pairs, items, item_cov6, tmap, T_eval, T_lin):
    """float32 H [m, 21], b [m, 6], err [m]: the D2D terms of nr.pair_terms (Q = cov_B + (R_lin cov_A) R_lin^T, C = adj(Q) / det(Q)) with
    w = sqrtf((float)num_points) in place of the Cauchy kernel and without the num_points > 6 gate.  nr.pair_terms computes
    w_c = k2 / (k2 + n n) and multiplies J, e by it; here the same expressions are evaluated with w substituted, so the function is written
    out again rather than rescaled (w A C is not (w_c A) C (w / w_c) in float)."""
    m = pairs.shape[0]
    H = np.zeros((m, 21), F)
    b = np.zeros((m, 6), F)
    err = np.zeros(m, F)
    if m == 0:
        return H, b, err
    it, vx = pairs[:, 0], pairs[:, 1]
    Te = np.asarray(T_eval, np.float64).astype(F)
    Tl = np.asarray(T_lin, np.float64).astype(F)
    a = nr.transform(Te, items[it])
    mb = tmap["mean"][vx]
    cb = tmap["cov"][vx]
    ca = full(np.asarray(item_cov6, F)[it])
    e = [mb[:, r] - a[:, r] for r in range(3)]
    q = [[cb[:, min(i, j), max(i, j)] for j in range(3)] for i in range(3)]
    A = [[ca[:, min(i, j), max(i, j)] for j in range(3)] for i in range(3)]
    R = [[Tl[i, j] for j in range(3)] for i in range(3)]
    M = [[(R[i][0] * A[0][j] + R[i][1] * A[1][j]) + R[i][2] * A[2][j] for j in range(3)] for i in range(3)]
    q = [[q[i][j] + ((M[i][0] * R[j][0] + M[i][1] * R[j][1]) + M[i][2] * R[j][2]) for j in range(3)] for i in range(3)]
    c = [[None] * 3 for _ in range(3)]
    c[0][0] = q[1][1] * q[2][2] - q[1][2] * q[2][1]
    c[0][1] = q[0][2] * q[2][1] - q[0][1] * q[2][2]
    c[0][2] = q[0][1] * q[1][2] - q[0][2] * q[1][1]
    c[1][0] = q[1][2] * q[2][0] - q[1][0] * q[2][2]
    c[1][1] = q[0][0] * q[2][2] - q[0][2] * q[2][0]
    c[1][2] = q[0][2] * q[1][0] - q[0][0] * q[1][2]
    c[2][0] = q[1][0] * q[2][1] - q[1][1] * q[2][0]
    c[2][1] = q[0][1] * q[2][0] - q[0][0] * q[2][1]
    c[2][2] = q[0][0] * q[1][1] - q[0][1] * q[1][0]
    det = (q[0][0] * c[0][0] + q[0][1] * c[1][0]) + q[0][2] * c[2][0]
    c = [[c[i][j] / det for j in range(3)] for i in range(3)]
    w = np.sqrt(tmap["num_points"][vx].astype(F))
    we = [w * e[r] for r in range(3)]
    u = [(we[0] * c[0][j] + we[1] * c[1][j]) + we[2] * c[2][j] for j in range(3)]
    err[:] = (u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]
    z, one = np.zeros(m, F), np.ones(m, F)
    J = [[z, -a[:, 2], a[:, 1], -one, z, z], [a[:, 2], z, -a[:, 0], z, -one, z], [-a[:, 1], a[:, 0], z, z, z, -one]]
    B = []
    for i in range(6):
        A0, A1, A2 = w * J[0][i], w * J[1][i], w * J[2][i]
        B.append([(A0 * c[0][j] + A1 * c[1][j]) + A2 * c[2][j] for j in range(3)])
    t = 0
    for i in range(6):
        for j in range(i, 6):
            H[:, t] = (B[i][0] * J[0][j] + B[i][1] * J[1][j]) + B[i][2] * J[2][j]
            t += 1
    for i in range(6):
        b[:, i] = (B[i][0] * e[0] + B[i][1] * e[1]) + B[i][2] * e[2]
    return H, b, err


# ------------------------------------------------------------------------------------------------ the object

class Cloud:
    """a cloud with the three stages this method derives from it"""

    def __init__(self, xyz):
        self.xyz = np.ascontiguousarray(xyz, F)
        self.raw = self.raw_key = None     # [n, 6], what it was made with
        self.kept = self.kept_key = None   # dict(index, xyz, cov)
        self.map = self.map_key = None


class VgicpCuda:
    """fast_gicp::FastVGICPCuda (VH:27-85) as defined in include/gorio_apd.h.  Defaults of VI:22-32: k = 20, CPU_PARALLEL_KDTREE, kernel
    0.5 / 3.0, PLANE, DIRECT1, resolution 1.0."""

    def __init__(self, nn_method=CPU_PARALLEL_KDTREE, k=20, kernel_width=0.5, kernel_max_dist=3.0, regularization=PLANE, search=DIRECT1, resolution=1.0, radius=-1.0):
        self.nn_method, self.k, self.kernel_width, self.kernel_max_dist = nn_method, k, kernel_width, kernel_max_dist
        self.regularization, self.search, self.resolution, self.radius = regularization, search, float(resolution), radius
        self.source = self.target = None
        self.pairs = self.x_lin = None
        self.builds = dict(raw=0, kept=0, map=0)

    def setInputSource(self, xyz):  # noqa: N802
        self.source, self.pairs = Cloud(xyz), None

    def setInputTarget(self, xyz):  # noqa: N802
        self.target, self.pairs = Cloud(xyz), None

    def swapSourceAndTarget(self):  # noqa: N802 -- VC:97-107: clouds and covariances change sides, the new target's map is built
        self.source, self.target = self.target, self.source
        self.pairs = None

    def _raw_key(self):
        if self.nn_method == GPU_RBF_KERNEL:
            return ("rbf", float(self.kernel_width), float(max_dist(self.kernel_width, self.kernel_max_dist)))
        return ("knn", self.k)

    def raw(self, c):
        if c.raw_key != self._raw_key():
            self.builds["raw"] += 1
            if self.nn_method == GPU_RBF_KERNEL:
                c.raw = cov_rbf(c.xyz, self.kernel_width, self.kernel_max_dist)
            else:
                if c.xyz.shape[0] < self.k:
                    raise ValueError("fewer points than k")
                c.raw = cov_knn(c.xyz, knn(c.xyz, self.k))
            c.raw_key, c.kept_key, c.map_key = self._raw_key(), None, None
        return c.raw

    def kept(self, c, raw=None):
        """raw: covariances to use instead of the restated ones (the GPU's own, through its parity hook)"""
        if raw is not None:
            c.raw, c.raw_key, c.kept_key, c.map_key = np.asarray(raw, F), self._raw_key(), None, None
        r = self.raw(c)
        if c.kept_key != self.regularization:
            self.builds["kept"] += 1
            keep, cov = regularize(r, self.regularization)
            idx = np.flatnonzero(keep)
            c.kept, c.kept_key, c.map_key = dict(index=idx, xyz=c.xyz[idx], cov=cov[idx]), self.regularization, None
        return c.kept

    def adopt(self, c, points, voxels=None):
        """take the stages of cloud c from the GPU's parity hooks (ApdGicp.vgicp_cuda_points / vgicp_cuda_voxels), so that only the
        arithmetic behind them is compared"""
        idx = np.asarray(points["kept_index"], np.int64)
        c.raw, c.raw_key = np.asarray(points["cov_raw"], F), self._raw_key()
        c.kept, c.kept_key = dict(index=idx, xyz=c.xyz[idx], cov=np.asarray(points["cov"], F).reshape(-1, 6)), self.regularization
        c.map, c.map_key = (None, None) if voxels is None else (map_from_tables(voxels, self.resolution), F(self.resolution))

    def target_map(self):
        c = self.target
        k = self.kept(c)
        if c.map_key != F(self.resolution):  # deviation: a changed resolution rebuilds the map
            self.builds["map"] += 1
            c.map, c.map_key = build_map(k["xyz"], k["cov"], self.resolution), F(self.resolution)
        return c.map

    def _sums(self, T):
        k = self.kept(self.source)
        H, b, e = pair_terms(self.pairs, k["xyz"], k["cov"], self.target.map, T, self.x_lin)
        return float(e.astype(np.float64).sum()), nr._unpack_h(H.astype(np.float64).sum(axis=0)), b.astype(np.float64).sum(axis=0)

    def linearize(self, T):  # VI:170-173
        tmap = self.target_map()
        T = np.asarray(T, np.float64)
        self.pairs = find_pairs(T, self.kept(self.source)["xyz"], tmap, nr.offsets(self.search, self.radius))
        self.x_lin = T.copy()
        return self._sums(T)

    def compute_error(self, T):  # VC:276-284 over the stale pairs with R_lin
        return self._sums(np.asarray(T, np.float64))[0]

    def align(self, guess=None, optimizer="LM", **kw):
        return nr.align(self, guess, optimizer, **kw)


# ------------------------------------------------------------------------------------------------ scenes

SCENE_SEED = 4  # chosen by running this restatement: no point of scene_pair(700) / scene_pair(3000) within 1 % of the PLANE threshold (k = 20, and RBF 0.5 / 3.0)


def rail_scene(n=3000, seed=SCENE_SEED, noise=0.02):
    """nr.structured_scene with a sixth of the points on four thin lines -- two rails along x near the floor, two poles along z -- so that
    the PLANE filter has something to drop (the plain scene drops nothing)."""
    rng = np.random.default_rng(seed)
    nl = n // 6
    room = nr.structured_scene(n - nl, nr.SCENE_SEED + seed, noise=noise).astype(np.float64)
    which = rng.integers(0, 4, nl)
    t = rng.uniform(0.0, 1.0, nl)
    a = np.array([[-7.0, -2.0, 0.4], [-7.0, 3.5, 0.4], [1.0, 1.0, 0.2], [-3.0, -5.5, 0.2]])
    d = np.array([[14.0, 0.0, 0.0], [14.0, 0.0, 0.0], [0.0, 0.0, 5.0], [0.0, 0.0, 5.0]])
    lines = a[which] + t[:, None] * d[which] + rng.normal(0.0, noise, (nl, 3))
    pts = np.concatenate([room, lines])
    return pts[rng.permutation(n)].astype(F)


def scene_pair(n=3000, seed=SCENE_SEED, T=None):
    """(source, target, T): target = a rail scene, source = T^-1 * another sampling of it, so that align() should return T."""
    T = nr.known_transform() if T is None else T
    tgt = rail_scene(n, seed)
    other = rail_scene(n, seed + 100).astype(np.float64)
    Ti = np.linalg.inv(T)
    return (other @ Ti[:3, :3].T + Ti[:3, 3]).astype(F), tgt, T
