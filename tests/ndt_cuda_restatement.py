"""NumPy restatement of GORIO_METHOD_NDT_CUDA (include/gorio_apd.h): fast_gicp::NDTCuda, P2D and D2D, as this library defines it.

Reference lines (paths relative to the reference's fast_apdgicp/):
  NC = src/fast_gicp/cuda/ndt_cuda.cu                  ND = src/fast_gicp/cuda/ndt_compute_derivatives.cu
  GV = src/fast_gicp/cuda/gaussian_voxelmap.cu         FV = src/fast_gicp/cuda/find_voxel_correspondences.cu
  CR = src/fast_gicp/cuda/covariance_regularization.cu NS = include/fast_gicp/ndt/ndt_settings.hpp
  LSQ = include/fast_gicp/gicp/impl/lsq_registration_impl.hpp

Every float32 operation is written out element-wise in ONE order (NumPy rounds every float32 product and sum on its own, nothing is
fused); `@` is used on float64 only.  The shell is the LsqRegistration restatement of tests/gicp_restatement.py, copied here with a trace
of every rho and convergence measure so that tests can pick scenes whose decisions a one-ulp difference cannot flip.
"""
import numpy as np

import gicp_restatement as gr

F = np.float32
P2D, D2D = 0, 1  # NS:6
DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = 0, 1, 2, 3
MIN_EIG = 1e-3  # CR:73-87


# ------------------------------------------------------------------------------------------------ offsets (NC:35-88)

def offsets(search, radius=-1.0):
    if search == DIRECT1:
        return np.zeros((1, 3), np.int64)
    if search == DIRECT7:  # NC:49-57
        return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)
    if search == DIRECT27:  # NC:59-68: i, j, k nested, k fastest
        return np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], np.int64)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError("radius must be positive and finite")
    if radius > 3.0:
        raise NotImplementedError("radius above 3")
    rng = int(np.ceil(radius))  # NC:72-82
    out = []
    for i in range(-rng, rng + 1):
        for j in range(-rng, rng + 1):
            for k in range(-rng, rng + 1):
                if np.sqrt(float(i * i + j * j + k * k)) <= radius + 1e-3:
                    out.append([i, j, k])
    return np.array(out, np.int64)


# ------------------------------------------------------------------------------------------------ voxel map (GV:118-121, 133-141, 185-188)

def voxel_coord(x, resolution):
    """(int)floorf(x / res - 0.5f) per axis, in float32."""
    q = np.asarray(x, F) / F(resolution)
    q = q - F(0.5)
    return np.floor(q).astype(np.int64)


def voxel_coord_double(x, resolution):
    """the double rule of the FastVGICP map (fast_vgicp_voxel.hpp:158-160), for the test that the two differ"""
    return np.floor(np.asarray(x, F).astype(np.float64) / float(resolution) - 0.5).astype(np.int64)


# a point where the float rule and the double rule of the FastVGICP map disagree: 2.25 / 0.3f rounds to 7.4999995 in float32 (voxel 6)
# while 2.25 / 0.3 - 0.5 is 7.0 in double (voxel 7)
FLOAT_RULE_POINT, FLOAT_RULE_RESOLUTION = 2.25, 0.3

_B = 1 << 20


def _pack(c):
    c = np.asarray(c, np.int64)
    assert np.all(np.abs(c) < _B), "the restatement packs coordinates into 21 bits each"
    return ((c[..., 0] + _B) << 42) | ((c[..., 1] + _B) << 21) | (c[..., 2] + _B)


def regularize(cov_raw):
    """sum_i max(1e-3, lambda_i) v_i v_i^T of the upper triangle of cov_raw widened to double, rounded to float32 once."""
    a = np.asarray(cov_raw, F).astype(np.float64)
    out = np.empty(a.shape, F)
    for v in range(a.shape[0]):
        m = np.triu(a[v]) + np.triu(a[v], 1).T
        w, V = np.linalg.eigh(m)
        out[v] = ((V * np.maximum(w, MIN_EIG)) @ V.T).astype(F)
    return out


def build_map(points, resolution):
    """dict(coord [nv,3] int, num_points, mean [nv,3], cov_raw [nv,3,3], cov [nv,3,3], key (packed, ascending), res): voxels in ascending
    lexicographic (x, y, z) coordinate order, every voxel's points accumulated in input order in float32."""
    pts = np.ascontiguousarray(points, F)
    c = voxel_coord(pts, resolution)
    order = np.lexsort((c[:, 2], c[:, 1], c[:, 0]))  # stable: input order inside a voxel
    cs = c[order]
    start = np.flatnonzero(np.r_[True, np.any(cs[1:] != cs[:-1], axis=1)])
    cnt = np.diff(np.r_[start, len(order)])
    nv = len(start)
    s = np.zeros((nv, 3), F)
    S = np.zeros((nv, 6), F)  # 00 01 02 11 12 22 (p p^T is symmetric bit for bit)
    for k in range(int(cnt.max())):
        idx = np.flatnonzero(cnt > k)
        p = pts[order[start[idx] + k]]
        s[idx] = s[idx] + p
        S[idx, 0] = S[idx, 0] + p[:, 0] * p[:, 0]
        S[idx, 1] = S[idx, 1] + p[:, 0] * p[:, 1]
        S[idx, 2] = S[idx, 2] + p[:, 0] * p[:, 2]
        S[idx, 3] = S[idx, 3] + p[:, 1] * p[:, 1]
        S[idx, 4] = S[idx, 4] + p[:, 1] * p[:, 2]
        S[idx, 5] = S[idx, 5] + p[:, 2] * p[:, 2]
    fn = cnt.astype(F)
    mean = s / fn[:, None]
    full = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 0): 1, (1, 1): 3, (1, 2): 4, (2, 0): 2, (2, 1): 4, (2, 2): 5}
    raw = np.empty((nv, 3, 3), F)
    for i in range(3):
        for j in range(3):
            raw[:, i, j] = (S[:, full[(i, j)]] - mean[:, i] * s[:, j]) / fn  # GV:188
    coord = cs[start]
    return dict(coord=coord, num_points=cnt.astype(np.int32), mean=mean, cov_raw=raw, cov=regularize(raw), key=_pack(coord), res=F(resolution))


def map_from_tables(tab, resolution):
    """a map dict from the arrays of the GPU's parity hook (ApdGicp.ndt_cuda_voxels)"""
    coord = np.asarray(tab["coord"], np.int64)
    return dict(coord=coord, num_points=np.asarray(tab["num_points"], np.int32), mean=np.asarray(tab["mean"], F), cov_raw=np.asarray(tab["cov_raw"], F),
                cov=np.asarray(tab["cov"], F), key=_pack(coord), res=F(resolution))


# ------------------------------------------------------------------------------------------------ pairs (FV:32-60, 83-111)

def transform(Tf, p):
    """R p + t per row, left to right, float32"""
    Tf = np.asarray(Tf, F)
    p = np.asarray(p, F)
    out = np.empty((p.shape[0], 3), F)
    for r in range(3):
        a = Tf[r, 0] * p[:, 0]
        a = a + Tf[r, 1] * p[:, 1]
        a = a + Tf[r, 2] * p[:, 2]
        out[:, r] = a + Tf[r, 3]
    return out


def find_pairs(T, items, tmap, offs):
    """[n_pairs, 2] (item, voxel), offset-major then item order"""
    Tf = np.asarray(T, np.float64).astype(F)
    c = voxel_coord(transform(Tf, items), tmap["res"])
    out = []
    for o in offs:
        key = _pack(c + o[None, :])
        pos = np.searchsorted(tmap["key"], key)
        pos = np.minimum(pos, len(tmap["key"]) - 1)
        hit = tmap["key"][pos] == key
        it = np.flatnonzero(hit)
        out.append(np.stack([it, pos[it]], axis=1))
    return np.concatenate(out, axis=0).astype(np.int64) if out else np.zeros((0, 2), np.int64)


# ------------------------------------------------------------------------------------------------ pair terms (ND:50-91, 120-163, 15-18)

def pair_terms(pairs, items, item_cov, tmap, T_eval, T_lin, d2d):
    """float32 H [m, 21] (upper triangle, row-major), b [m, 6], err [m] of the pairs whose TARGET voxel has more than 6 points (the others
    give zeros).  The written order of include/gorio_apd.h: a' = R a + t; e = mean_B - a'; Q = cov_B (+ (R_l cov_A) R_l^T); C = adj(Q) /
    det(Q), the nine cofactors minuend first, det = (q00 c00 + q01 c10) + q02 c20; w = k^2 / (k^2 + n n), n = sqrt((e0 e0 + e1 e1) + e2 e2);
    J = [skew(a') | -I]; A = w J^T; B = A C; H = B J; b = B e; err = ((w e)^T C) e; every 3-term sum left to right, zeros included."""
    m = pairs.shape[0]
    H = np.zeros((m, 21), F)
    b = np.zeros((m, 6), F)
    err = np.zeros(m, F)
    keep = np.flatnonzero(tmap["num_points"][pairs[:, 1]] > 6)  # ND:61, 132
    if keep.size == 0:
        return H, b, err
    it, vx = pairs[keep, 0], pairs[keep, 1]
    Te = np.asarray(T_eval, np.float64).astype(F)
    Tl = np.asarray(T_lin, np.float64).astype(F)
    a = transform(Te, items[it])
    mb = tmap["mean"][vx]
    cb = tmap["cov"][vx]
    e = [mb[:, r] - a[:, r] for r in range(3)]
    # the kernel reads cov_B as an upper triangle and mirrors it
    up = {(0, 0): (0, 0), (0, 1): (0, 1), (0, 2): (0, 2), (1, 0): (0, 1), (1, 1): (1, 1), (1, 2): (1, 2), (2, 0): (0, 2), (2, 1): (1, 2), (2, 2): (2, 2)}
    q = [[cb[:, up[(i, j)][0], up[(i, j)][1]] for j in range(3)] for i in range(3)]
    if d2d:
        ca = item_cov[it]
        A = [[ca[:, up[(i, j)][0], up[(i, j)][1]] for j in range(3)] for i in range(3)]
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
    res = F(tmap["res"])
    k2 = res * res
    nrm = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    w = k2 / (k2 + nrm * nrm)
    we = [w * e[r] for r in range(3)]
    u = [(we[0] * c[0][j] + we[1] * c[1][j]) + we[2] * c[2][j] for j in range(3)]
    err[keep] = (u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]
    z, one = np.zeros(len(keep), F), np.ones(len(keep), F)
    J = [[z, -a[:, 2], a[:, 1], -one, z, z], [a[:, 2], z, -a[:, 0], z, -one, z], [-a[:, 1], a[:, 0], z, z, z, -one]]
    B = []
    for i in range(6):
        A0, A1, A2 = w * J[0][i], w * J[1][i], w * J[2][i]
        B.append([(A0 * c[0][j] + A1 * c[1][j]) + A2 * c[2][j] for j in range(3)])
    t = 0
    for i in range(6):
        for j in range(i, 6):
            H[keep, t] = (B[i][0] * J[0][j] + B[i][1] * J[1][j]) + B[i][2] * J[2][j]
            t += 1
    for i in range(6):
        b[keep, i] = (B[i][0] * e[0] + B[i][1] * e[1]) + B[i][2] * e[2]
    return H, b, err


def _unpack_h(h21):
    H = np.zeros((6, 6))
    t = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = h21[t]
            t += 1
    return H


# ------------------------------------------------------------------------------------------------ the object

class NdtCuda:
    """fast_gicp::NDTCuda (NH:22-71) as defined in include/gorio_apd.h.  Defaults of NC:13-23: D2D, DIRECT7, resolution 1.0."""

    def __init__(self, distance_mode=D2D, search=DIRECT7, resolution=1.0, radius=-1.0):
        self.distance_mode, self.search, self.resolution, self.radius = distance_mode, search, float(resolution), radius
        self.source = self.target = None
        self.source_map = self.target_map = None
        self.pairs = None
        self.x_lin = None
        self.map_builds = 0

    def setInputSource(self, xyz):  # noqa: N802
        self.source, self.source_map, self.pairs = np.ascontiguousarray(xyz, F), None, None

    def setInputTarget(self, xyz):  # noqa: N802
        self.target, self.target_map, self.pairs = np.ascontiguousarray(xyz, F), None, None

    def swapSourceAndTarget(self):  # noqa: N802 -- NC:90-93
        self.source, self.target = self.target, self.source
        self.source_map, self.target_map = self.target_map, self.source_map
        self.pairs = None

    def setResolution(self, r):  # noqa: N802 -- deviation: a changed resolution marks the maps stale (the reference keeps them, NC:120-140)
        self.resolution = float(r)

    def _map(self, cloud, held):
        if held is not None and held["res"] == F(self.resolution):
            return held
        self.map_builds += 1
        return build_map(cloud, self.resolution)

    def create_voxelmaps(self):  # NC:115-140: P2D builds no source map
        self.target_map = self._map(self.target, self.target_map)
        if self.distance_mode == D2D:
            self.source_map = self._map(self.source, self.source_map)

    def _items(self):
        if self.distance_mode == D2D:
            return self.source_map["mean"], self.source_map["cov"]
        return self.source, None

    def _sums(self, T):
        items, icov = self._items()
        H, b, e = pair_terms(self.pairs, items, icov, self.target_map, T, self.x_lin, self.distance_mode == D2D)
        return float(e.astype(np.float64).sum()), _unpack_h(H.astype(np.float64).sum(axis=0)), b.astype(np.float64).sum(axis=0)

    def linearize(self, T):  # NI:82-85
        self.create_voxelmaps()
        T = np.asarray(T, np.float64)
        self.pairs = find_pairs(T, self._items()[0], self.target_map, offsets(self.search, self.radius))
        self.x_lin = T.copy()
        return self._sums(T)

    def compute_error(self, T):  # NC:162-177 over the stale pairs with R_lin
        return self._sums(np.asarray(T, np.float64))[0]

    def align(self, guess=None, optimizer="LM", **kw):
        return align(self, guess, optimizer, **kw)


def conv_measure(delta, rotation_epsilon, transformation_epsilon):
    """the quantity LSQ:83-92 compares with 1"""
    r = np.abs(delta[:3, :3] - np.eye(3)) * (1.0 / rotation_epsilon)
    t = np.abs(delta[:3, 3]) * (1.0 / transformation_epsilon)
    return float(max(r.max(), t.max()))


def align(reg, guess=None, optimizer="LM", max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4, lm_max_iterations=10, lm_init_lambda_factor=1e-9):
    """LsqRegistration::computeTransformation (LSQ:55-80), as tests/gicp_restatement.py:align, with a trace: rho of every LM trial and the
    convergence measure of every comparison with 1."""
    x0 = np.asarray(np.eye(4) if guess is None else guess, F).astype(np.float64)
    x0[3] = [0, 0, 0, 1]
    lam, converged, nr_iterations, Hfin, n_lin, n_err = -1.0, False, 0, np.eye(6), 0, 0
    rhos, measures = [], []
    delta = np.eye(4)
    for it in range(max_iterations):
        if converged:
            break
        nr_iterations = it
        y0, H, b = reg.linearize(x0)
        n_lin += 1
        ok = False
        if optimizer == "GN":
            d = gr.ldlt6_solve(H, -b)
            delta = gr.delta_from_d(d)
            x0 = gr.isom_mul(delta, x0)
            Hfin, ok = H.copy(), True
        else:
            if lam < 0.0:
                lam = lm_init_lambda_factor * np.abs(np.diag(H)).max()
            nu = 2.0
            for _ in range(lm_max_iterations):
                d = gr.ldlt6_solve(H + lam * np.eye(6), -b)
                delta = gr.delta_from_d(d)
                xi = gr.isom_mul(delta, x0)
                yi = reg.compute_error(xi)
                n_err += 1
                den = 0.0
                for q in range(6):
                    den += d[q] * (lam * d[q] - b[q])
                with np.errstate(all="ignore"):
                    rho = float(np.float64(y0 - yi) / np.float64(den))  # 0 / 0 = NaN when there are no pairs: not < 0, the step is taken
                rhos.append(rho)
                if rho < 0:
                    measures.append(conv_measure(delta, rotation_epsilon, transformation_epsilon))
                    if measures[-1] < 1.0:
                        ok = True
                        break
                    lam = nu * lam
                    nu = 2 * nu
                    continue
                x0 = xi
                f = 1 - (2 * rho - 1) ** 3
                lam = lam * (f if f > 1.0 / 3.0 else 1.0 / 3.0)  # fmax(1/3, f): 1/3 for a NaN f
                Hfin, ok = H.copy(), True
                break
        if not ok:
            break
        measures.append(conv_measure(delta, rotation_epsilon, transformation_epsilon))
        converged = measures[-1] < 1.0
    return dict(T=x0.astype(F), H=Hfin, converged=bool(converged), nr_iterations=nr_iterations, n_linearize=n_lin, n_compute_error=n_err, rhos=rhos,
                measures=measures)


# ------------------------------------------------------------------------------------------------ scenes

SCENE_SEED = 20261020


def structured_scene(n=4096, seed=SCENE_SEED, extent=8.0, noise=0.02):
    """A seeded room: a floor, two walls and three pillars, sampled with a little noise -- planes in three directions and some clutter."""
    rng = np.random.default_rng(seed)
    k = n // 8
    parts = []
    u = rng.uniform(-extent, extent, (3 * k, 2))
    parts.append(np.c_[u, np.zeros(3 * k)])  # floor z = 0
    u = rng.uniform([-extent, 0.0], [extent, 6.0], (2 * k, 2))
    parts.append(np.c_[u[:, 0], np.full(2 * k, extent), u[:, 1]])  # wall y = extent
    u = rng.uniform([-extent, 0.0], [extent, 6.0], (2 * k, 2))
    parts.append(np.c_[np.full(2 * k, -extent), u[:, 0], u[:, 1]])  # wall x = -extent
    rest = n - 7 * k
    cx = np.array([[3.0, -4.0], [-5.0, 2.5], [6.5, 6.0]])
    pil = rng.integers(0, 3, rest)
    ang = rng.uniform(0, 2 * np.pi, rest)
    parts.append(np.c_[cx[pil, 0] + 0.6 * np.cos(ang), cx[pil, 1] + 0.6 * np.sin(ang), rng.uniform(0.0, 5.0, rest)])
    pts = np.concatenate(parts) + rng.normal(0.0, noise, (n, 3))
    return pts[rng.permutation(n)].astype(F)


def known_transform(tx=0.25, ty=-0.15, tz=0.05, yaw=0.03, pitch=-0.01):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = [tx, ty, tz]
    return T


def scene_pair(n=4096, seed=SCENE_SEED, T=None):
    """(source, target, T): target = a structured scene, source = T^-1 * another sampling of it, so that align() should return T."""
    T = known_transform() if T is None else T
    tgt = structured_scene(n, seed)
    other = structured_scene(n, seed + 1).astype(np.float64)
    Ti = np.linalg.inv(T)
    src = (other @ Ti[:3, :3].T + Ti[:3, 3]).astype(F)
    return src, tgt, T
