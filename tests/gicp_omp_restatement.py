"""NumPy restatement of GICP_OMP (pclomp::GeneralizedIterativeClosestPoint, gicp_omp_impl.hpp:50-533) and of the BFGS minimiser that
DESIGN.md specifies rule by rule ("GICP_OMP: the BFGS specification", rules S, T, L, I, Q, C, G).  Written from those two documents, not
from the device code: the GPU tests compare the library against this file.

Conventions fixed by DESIGN.md 2: float sums run left to right without fused multiply-adds, a float transform is
((m0 x + m1 y) + m2 z) + m3, float sin / cos / atan2 / asin are the correctly rounded float results, k-NN and 1-NN ties go to the
lowest index.
"""
import math

import numpy as np

f32 = np.float32
EPS = np.finfo(np.float64).eps
RUNNING, SUCCESS, NO_PROGRESS, FAILED = -1, 0, 1, 2


# ---------------------------------------------------------------------------------------------- searches and float transforms
def sqdist(q, t):
    """[nq, nt] float distances, ((dx dx) + dy dy) + dz dz."""
    d = q[:, None, :].astype(f32) - t[None, :, :].astype(f32)
    r = d[..., 0] * d[..., 0]
    r = r + d[..., 1] * d[..., 1]
    return r + d[..., 2] * d[..., 2]


def knn(cloud, k, chunk=512):
    """k nearest neighbours of every point in its own cloud, ascending distance, ties to the lower index."""
    out = np.empty((cloud.shape[0], k), np.int32)
    for a in range(0, cloud.shape[0], chunk):
        d = sqdist(cloud[a:a + chunk], cloud)
        out[a:a + chunk] = np.argsort(d, axis=1, kind="stable")[:, :k]
    return out


def nn1(query, target, chunk=512):
    idx = np.empty(query.shape[0], np.int32)
    dist = np.empty(query.shape[0], f32)
    for a in range(0, query.shape[0], chunk):
        d = sqdist(query[a:a + chunk], target)
        j = np.argmin(d, axis=1)  # first minimum = lowest index
        idx[a:a + chunk] = j
        dist[a:a + chunk] = d[np.arange(d.shape[0]), j]
    return idx, dist


def transform_f(T, pts):
    T = np.asarray(T, f32)
    x, y, z = pts[:, 0].astype(f32), pts[:, 1].astype(f32), pts[:, 2].astype(f32)
    out = np.empty((pts.shape[0], 3), f32)
    for r in range(3):
        a = T[r, 0] * x
        a = a + T[r, 1] * y
        a = a + T[r, 2] * z
        out[:, r] = a + T[r, 3]
    return out


def mul_f(a, b):
    """float matrix product, every sum left to right."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    n = a.shape[0]
    c = np.zeros((n, n), f32)
    for r in range(n):
        for q in range(n):
            s = a[r, 0] * b[0, q]
            for k in range(1, n):
                s = f32(s + a[r, k] * b[k, q])
            c[r, q] = s
    return c


def rsin(a):
    return f32(math.sin(float(f32(a))))


def rcos(a):
    return f32(math.cos(float(f32(a))))


def apply_state(x):
    """applyState on the identity (GO:522-533): float Rz Ry Rx, float translation."""
    sa, ca, sb, cb, sc, cc = rsin(x[3]), rcos(x[3]), rsin(x[4]), rcos(x[4]), rsin(x[5]), rcos(x[5])
    o, z = f32(1), f32(0)
    Rx = np.array([[o, z, z], [z, ca, -sa], [z, sa, ca]], f32)
    Ry = np.array([[cb, z, sb], [z, o, z], [-sb, z, cb]], f32)
    Rz = np.array([[cc, -sc, z], [sc, cc, z], [z, z, o]], f32)
    T = np.eye(4, dtype=f32)
    T[:3, :3] = mul_f(mul_f(Rz, Ry), Rx)
    T[:3, 3] = np.asarray(x[:3], np.float64).astype(f32)
    return T


def state_of(T):
    """GO:194-200 with the float results rounded once."""
    T = np.asarray(T, f32)
    return np.array([T[0, 3], T[1, 3], T[2, 3], f32(math.atan2(float(T[2, 1]), float(T[2, 2]))), f32(math.asin(float(-T[2, 0]))),
                     f32(math.atan2(float(T[1, 0]), float(T[0, 0])))], np.float64)


# ---------------------------------------------------------------------------------------------- covariances, GO:50-122
def covariances(cloud, lists, eps=1e-3):
    n, k = lists.shape
    if k > n:
        raise ValueError("cloud smaller than k_correspondences")
    mean = np.zeros((n, 3))
    low = np.zeros((n, 6))  # (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
    pairs = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    for t in range(k):
        p = cloud[lists[:, t]].astype(f32)
        mean += p.astype(np.float64)
        for q, (a, b) in enumerate(pairs):
            low[:, q] += (p[:, a] * p[:, b]).astype(np.float64)  # a float product, added in double
    mean /= float(k)
    cov = np.zeros((n, 3, 3))
    for q, (a, b) in enumerate(pairs):
        v = low[:, q] / float(k) - mean[:, a] * mean[:, b]
        cov[:, a, b] = v
        cov[:, b, a] = v
    U, s, _ = np.linalg.svd(cov)  # columns by descending singular value
    out = np.zeros((n, 3, 3))
    for c, v in enumerate((1.0, 1.0, eps)):
        out += v * U[:, :, c, None] * U[:, None, :, c]
    return out, s


# ---------------------------------------------------------------------------------------------- correspondences and Mahalanobis, GO:398-476
def cofactor_inverse(T):
    cof = np.empty_like(T)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            cof[:, r, c] = T[:, r1, c1] * T[:, r2, c2] - T[:, r1, c2] * T[:, r2, c1]
    det = (cof[:, 0, 0] * T[:, 0, 0] + cof[:, 1, 0] * T[:, 1, 0]) + cof[:, 2, 0] * T[:, 2, 0]
    return np.transpose(cof, (0, 2, 1)) * (1.0 / det)[:, None, None]


def update(transformation, guess, output, target, C1, C2, corr_dist):
    """One pass of GO:411-476: (corr [-1 = none], float distances, Mahalanobis matrices in double, the same cast to float)."""
    query = transform_f(transformation, output)
    j, d = nn1(query, target)
    keep = d.astype(np.float64) < corr_dist * corr_dist
    Rd = (np.asarray(transformation, f32).astype(np.float64) @ np.asarray(guess, f32).astype(np.float64))[:3, :3]
    M = np.zeros((output.shape[0], 3, 3))
    if keep.any():
        temp = Rd @ C1[keep] @ Rd.T + C2[j[keep]]
        M[keep] = cofactor_inverse(temp)
    return np.where(keep, j, -1).astype(np.int32), d, M, M.astype(f32)


# ---------------------------------------------------------------------------------------------- the functor, GO:249-371
class Functor:
    """f / df / fdf over frozen pairs.  scale multiplies every reduction (the stability condition of the tests: 1 +- 1e-9)."""

    def __init__(self, output, target, corr, Mf, scale=1.0):
        sel = corr >= 0
        self.p = output[sel].astype(f32)
        self.q = target[corr[sel]].astype(f32)
        self.M = Mf[sel].astype(f32)
        self.m = int(sel.sum())
        self.scale = scale
        self.evaluations = 0

    def _res(self, x):
        return transform_f(apply_state(x), self.p) - self.q  # a float difference

    def f(self, x):
        self.evaluations += 1
        r, M = self._res(x), self.M
        t = [(M[:, a, 0] * r[:, 0] + M[:, a, 1] * r[:, 1]) + M[:, a, 2] * r[:, 2] for a in range(3)]
        ret = (r[:, 0] * t[0] + r[:, 1] * t[1]) + r[:, 2] * t[2]
        return float(ret.astype(np.float64).sum()) * self.scale / self.m

    def _sums(self, x):
        r = self._res(x).astype(np.float64)
        temp = np.einsum("nab,nb->na", self.M.astype(np.float64), r)
        f = float((r * temp).sum()) * self.scale / self.m
        g = np.zeros(6)
        g[:3] = temp.sum(axis=0) * self.scale * (2.0 / self.m)
        R = np.einsum("na,nb->ab", self.p.astype(np.float64), temp) * self.scale * (2.0 / self.m)
        g[3:] = r_derivative(x, R)
        return f, g, R

    def df(self, x):
        self.evaluations += 1
        return self._sums(x)[1]

    def fdf(self, x):
        self.evaluations += 1
        f, g, _ = self._sums(x)
        return f, g


def r_derivative(x, R):
    """computeRDerivative, GO:125-177."""
    phi, theta, psi = x[3], x[4], x[5]
    cphi, sphi, cth, sth, cpsi, spsi = math.cos(phi), math.sin(phi), math.cos(theta), math.sin(theta), math.cos(psi), math.sin(psi)
    dphi = np.array([[0, sphi * spsi + cphi * cpsi * sth, cphi * spsi - cpsi * sphi * sth],
                     [0, -cpsi * sphi + cphi * spsi * sth, -cphi * cpsi - sphi * spsi * sth],
                     [0, cphi * cth, -cth * sphi]])
    dth = np.array([[-cpsi * sth, cpsi * cth * sphi, cphi * cpsi * cth],
                    [-spsi * sth, cth * sphi * spsi, cphi * cth * spsi],
                    [-cth, -sphi * sth, -cphi * sth]])
    dpsi = np.array([[-cth * spsi, -cphi * cpsi - sphi * spsi * sth, cpsi * sphi - cphi * spsi * sth],
                     [cpsi * cth, -cphi * spsi + cpsi * sphi * sth, sphi * spsi + cphi * cpsi * sth],
                     [0, 0, 0]])
    return np.array([(d.T * R).sum() for d in (dphi, dth, dpsi)])  # matricesInnerProd: sum mat1(j, i) mat2(i, j)


# ---------------------------------------------------------------------------------------------- BFGS, DESIGN.md rules
def solve_quadratic(a, b, c):  # rule Q
    if a == 0:
        return [] if b == 0 else [-c / b]
    disc = b * b - 4 * a * c
    if disc > 0:
        if b == 0:
            r = math.sqrt(-c / a)
            return [-r, r]
        temp = -0.5 * (b + (1.0 if b > 0 else -1.0) * math.sqrt(disc))
        return sorted([temp / a, c / temp])
    if disc == 0:
        return [-0.5 * b / a] * 2
    return []


def interpolate(a, fa, fpa, b, fb, fpb, xmin, xmax, order=3):  # rules I, I2, I3
    zl, zh = (xmin - a) / (b - a), (xmax - a) / (b - a)
    if zl > zh:
        zl, zh = zh, zl
    f0, fp0, f1 = fa, fpa * (b - a), fb
    if order > 2 and not math.isnan(fpb):
        fp1 = fpb * (b - a)
        c = [f0, fp0, 3 * (f1 - f0) - 2 * fp0 - fp1, fp0 + fp1 - 2 * (f1 - f0)]

        def val(z):
            return c[0] + z * (c[1] + z * (c[2] + z * c[3]))
        zmin, fmin = zl, val(zl)
        cand = [zh] + [z for z in solve_quadratic(3 * c[3], 2 * c[2], c[1]) if zl < z < zh]
        for z in cand:
            if val(z) < fmin:
                zmin, fmin = z, val(z)
    else:
        def val(z):
            return f0 + z * (fp0 + z * (f1 - f0 - fp0))
        zmin, fmin = zl, val(zl)
        if val(zh) < fmin:
            zmin, fmin = zh, val(zh)
        c = 2 * (f1 - f0 - fp0)
        if c > 0:
            z = -fp0 / c
            if zl < z < zh and val(z) < fmin:
                zmin = z
    return a + zmin * (b - a)


class Bfgs:
    def __init__(self, fun, rho=0.01, sigma=0.01, tau1=9.0, tau2=0.05, tau3=0.5, step_size=1.0, order=3, bracket_iters=100, section_iters=100):
        self.fun = fun
        self.rho, self.sigma, self.tau1, self.tau2, self.tau3, self.step_size, self.order = rho, sigma, tau1, tau2, tau3, step_size, order
        self.bracket_iters, self.section_iters = bracket_iters, section_iters

    # rule C: the cache along x + alpha p
    def _change_direction(self):
        self.xa, self.ga, self.fa = self.x.copy(), self.g.copy(), self.f
        self.xk = self.fk = self.gk = self.dk = 0.0
        self.dfa = float(self.ga @ self.p)

    def _move(self, alpha):
        if alpha != self.xk:
            self.xa = self.x + alpha * self.p
            self.xk = alpha

    def _wf(self, alpha):
        if alpha == self.fk:
            return self.fa
        self._move(alpha)
        self.fa = self.fun.f(self.xa)
        self.fk = alpha
        return self.fa

    def _wdf(self, alpha):
        if alpha == self.dk:
            return self.dfa
        self._move(alpha)
        if alpha != self.gk:
            self.ga = self.fun.df(self.xa)
            self.gk = alpha
        self.dfa = float(self.ga @ self.p)
        self.dk = alpha
        return self.dfa

    def _wfdf(self, alpha):
        if alpha == self.fk and alpha == self.dk:
            return self.fa, self.dfa
        if alpha == self.fk or alpha == self.dk:
            return self._wf(alpha), self._wdf(alpha)
        self._move(alpha)
        self.fa, self.ga = self.fun.fdf(self.xa)
        self.fk = self.gk = alpha
        self.dfa = float(self.ga @ self.p)
        self.dk = alpha
        return self.fa, self.dfa

    def init(self, x):  # rule S
        self.x = np.array(x, np.float64)
        self.delta_f = 0.0
        self.f, self.g = self.fun.fdf(self.x)
        self.x0, self.g0 = self.x.copy(), self.g.copy()
        self.g0norm = float(np.sqrt(self.g0 @ self.g0))
        with np.errstate(divide="ignore", invalid="ignore"):
            self.p = self.g * (-1.0 / self.g0norm) if self.g0norm != 0 else self.g * np.nan
        self.pnorm = float(np.sqrt(self.p @ self.p))
        self.fp0 = -self.g0norm
        self._change_direction()

    def line_search(self, alpha1):  # rule L; returns (status, alpha)
        f0, fp0 = self._wfdf(0.0)
        alpha, alpha_prev = alpha1, 0.0
        falpha_prev, fpalpha_prev = f0, fp0
        a, b, fa, fb, fpa, fpb = 0.0, alpha, f0, 0.0, fp0, 0.0
        i = 0  # one counter for both loops; every loop test, passed or failed, consumes a count (rule L3)
        while True:
            i += 1
            if not i - 1 < self.bracket_iters:
                break
            if not math.isfinite(alpha):
                return FAILED, 0.0
            falpha = self._wf(alpha)
            if math.isnan(falpha):
                return FAILED, 0.0
            if falpha > f0 + alpha * self.rho * fp0 or falpha >= falpha_prev:
                a, fa, fpa = alpha_prev, falpha_prev, fpalpha_prev
                b, fb, fpb = alpha, falpha, math.nan
                break
            fpalpha = self._wdf(alpha)
            if abs(fpalpha) <= -self.sigma * fp0:
                return SUCCESS, alpha
            if fpalpha >= 0:
                a, fa, fpa = alpha, falpha, fpalpha
                b, fb, fpb = alpha_prev, falpha_prev, fpalpha_prev
                break
            delta = alpha - alpha_prev
            nxt = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta, alpha + self.tau1 * delta, self.order)
            alpha_prev, falpha_prev, fpalpha_prev = alpha, falpha, fpalpha
            alpha = nxt
        while True:
            i += 1
            if not i - 1 < self.section_iters:
                break
            delta = b - a
            alpha = interpolate(a, fa, fpa, b, fb, fpb, a + self.tau2 * delta, b - self.tau3 * delta, self.order)
            if not math.isfinite(alpha):
                return FAILED, 0.0
            falpha = self._wf(alpha)
            if math.isnan(falpha):
                return FAILED, 0.0
            if (a - alpha) * fpa <= EPS:
                return NO_PROGRESS, 0.0
            if falpha > f0 + self.rho * alpha * fp0 or falpha >= fa:
                b, fb, fpb = alpha, falpha, math.nan
            else:
                fpalpha = self._wdf(alpha)
                if abs(fpalpha) <= -self.sigma * fp0:
                    return SUCCESS, alpha
                if ((b - a) >= 0 and fpalpha >= 0) or ((b - a) <= 0 and fpalpha <= 0):
                    b, fb, fpb = a, fa, fpa
                a, fa, fpa = alpha, falpha, fpalpha
        return SUCCESS, 0.0  # rule L5

    def step(self):  # rule T
        f0 = self.f
        if self.pnorm == 0 or self.g0norm == 0 or self.fp0 == 0 or math.isnan(self.pnorm) or math.isnan(self.fp0):
            return NO_PROGRESS
        if self.delta_f < 0:
            alpha1 = min(1.0, 2.0 * max(-self.delta_f, 10 * EPS * abs(f0)) / (-self.fp0))
        else:
            alpha1 = abs(self.step_size)
        status, alpha = self.line_search(alpha1)
        if status != SUCCESS:
            return status
        self.f, _ = self._wfdf(alpha)
        self.x, self.g = self.xa.copy(), self.ga.copy()
        if not math.isfinite(self.f):
            return FAILED
        self.delta_f = self.f - f0
        dx, dg = self.x - self.x0, self.g - self.g0
        dxg, dgg, dxdg, dgnorm = float(dx @ self.g), float(dg @ self.g), float(dx @ dg), float(np.sqrt(dg @ dg))
        A = B = 0.0
        if dxdg != 0:
            B = dxg / dxdg
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg
        self.p = self.g - A * dx - B * dg
        self.g0, self.x0 = self.g.copy(), self.x.copy()
        self.g0norm = float(np.sqrt(self.g0 @ self.g0))
        self.pnorm = float(np.sqrt(self.p @ self.p))
        direction = -1.0 if float(self.p @ self.g) >= 0 else 1.0
        self.p = self.p * (direction / self.pnorm)
        self.pnorm = float(np.sqrt(self.p @ self.p))
        self.fp0 = float(self.p @ self.g0)
        self._change_direction()
        return SUCCESS

    def test_gradient(self, eps):  # rule G
        return SUCCESS if float(np.sqrt(self.g @ self.g)) < eps else RUNNING


def minimize(fun, x, max_inner, gradient_tol=1e-2):
    """GO:219-235: (x, status, inner iterations)."""
    s = Bfgs(fun)
    s.init(x)
    n, result = 0, RUNNING
    while True:
        n += 1
        result = s.step()
        if result:
            break
        result = s.test_gradient(gradient_tol)
        if not (result == RUNNING and n < max_inner):
            break
    return s.x.copy(), result, n


# ---------------------------------------------------------------------------------------------- computeTransformation, GO:375-520
class GicpOmp:
    def __init__(self, k_correspondences=20, gicp_epsilon=1e-3, rotation_epsilon=2e-3, transformation_epsilon=5e-4, max_iterations=200,
                 max_correspondence_distance=5.0, max_optimizer_iterations=20, scale=1.0):
        self.k, self.eps, self.rot_eps, self.trans_eps = k_correspondences, gicp_epsilon, rotation_epsilon, transformation_epsilon
        self.max_iterations, self.corr_dist, self.max_inner, self.scale = max_iterations, max_correspondence_distance, max_optimizer_iterations, scale
        self.src = self.tgt = self.C1 = self.C2 = None

    def set_source(self, pts):
        self.src, self.C1 = np.ascontiguousarray(pts, f32), None

    def set_target(self, pts):
        self.tgt, self.C2 = np.ascontiguousarray(pts, f32), None

    def compute_covariances(self):
        if self.C1 is None:
            self.knn_src = knn(self.src, self.k)
            self.C1, _ = covariances(self.src, self.knn_src, self.eps)
        if self.C2 is None:
            self.knn_tgt = knn(self.tgt, self.k)
            self.C2, _ = covariances(self.tgt, self.knn_tgt, self.eps)

    def align(self, guess=None):
        if self.k > self.src.shape[0] or self.k > self.tgt.shape[0]:
            raise ValueError("cloud smaller than k_correspondences")
        guess = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32)
        self.compute_covariances()
        output = transform_f(guess, self.src)
        Tr = np.eye(4, dtype=f32)
        prev = Tr.copy()
        converged, nr, inner_total, evals, status = False, 0, 0, 0, RUNNING
        while not converged:
            corr, _, _, Mf = update(Tr, guess, output, self.tgt, self.C1, self.C2, self.corr_dist)
            prev = Tr.copy()
            fun = Functor(output, self.tgt, corr, Mf, self.scale)
            if fun.m < 4:
                break
            x, status, inner = minimize(fun, state_of(Tr), self.max_inner)
            inner_total += inner
            evals += fun.evaluations
            if not (status in (NO_PROGRESS, SUCCESS) or inner == self.max_inner):
                break
            Tr = apply_state(x)
            delta = 0.0
            for k in range(4):
                for l in range(4):
                    ratio = 1.0 / self.rot_eps if (k < 3 and l < 3) else 1.0 / self.trans_eps
                    delta = max(delta, ratio * float(abs(f32(prev[k, l] - Tr[k, l]))))
            nr += 1
            if nr >= self.max_iterations or delta < 1:
                converged = True
                prev = Tr.copy()
        return dict(T=mul_f(prev, guess), converged=converged, nr_iterations=nr, inner_total=inner_total, evaluations=evals, last_status=status)
