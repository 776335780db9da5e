"""NumPy restatement of Patchwork++ ground segmentation as the preprocessing nodelet runs it (PREP:505-519), the yardstick of
include/gorio_ground.h.

PWP = include/patchworkpp/patchworkpp.hpp, PREP = apps/preprocessing_nodelet_ntu.cpp of the Go-RIO sources.  Float quantities are
kept in float32 with the reference's evaluation order; the LM plane fit runs in float64.  Choices the reference leaves open are the
project's (DESIGN.md "Patchwork++"): ties of the z sort by lowest input index; the 3 x 3 SVD is the cyclic float Jacobi of svd3 below;
the LM model cost change is taken from the scaled normal equations.
"""
import math

import numpy as np

F = np.float32
MAX_LM_ITER = 30  # PWP:552
FTOL, GTOL, PTOL = 1e-6, 1e-10, 1e-8  # Ceres 2.1 Solver::Options defaults
TERM = {0: "none", 1: "function_tolerance", 2: "parameter_tolerance", 3: "gradient_tolerance", 4: "max_iterations", 5: "min_radius"}


def default_params():
    """Params(), PWP:127-168, verbose off (PREP:100-102)."""
    return dict(enable_RNR=True, enable_RVPF=False, enable_TGR=True, num_iter=4, num_lpr=20, num_min_pts=10, RNR_ver_angle_thr=-15.0, RNR_intensity_thr=0.1,
                sensor_height=0.7, th_seeds=0.5, th_dist=1.0, max_range=50.0, min_range=1.0, uprightness_thr=0.5, adaptive_seed_selection_margin=-1.2,
                num_sectors_each_zone=[3, 1, 1, 3], num_rings_each_zone=[4, 4, 2, 2], max_flatness_storage=1000, max_elevation_storage=1000,
                elevation_thr=[0.0] * 4, flatness_thr=[0.0] * 4)


def range_covariance(P):
    """C_p = (R S)(R S)^T of estimate_plane_cov (PWP:501-518), upper triangle [m, 6]; dist and the two angles from float arithmetic."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    rxy2 = x * x + y * y  # float32
    dist = np.sqrt(rxy2 + z * z).astype(np.float64)
    sx, sy, sz = dist * 0.86 / 400, dist * math.sin(0.5 / 180 * math.pi), dist * math.sin(1.0 / 180 * math.pi)
    el = np.arctan2(np.sqrt(rxy2).astype(np.float64), z.astype(np.float64)).astype(F).astype(np.float64)
    az = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F).astype(np.float64)
    ce, se, ca, sa = np.cos(el), np.sin(el), np.cos(az), np.sin(az)
    A = np.stack([np.stack([ca * ce * sx, -sa * sy, ca * se * sz], -1), np.stack([sa * ce * sx, ca * sy, sa * se * sz], -1),
                  np.stack([-se * sx, 0.0 * sy, ce * sz], -1)], 1)  # R = yaw(az) pitch(el), A = R S
    out = [(A[:, r0, 0] * A[:, r1, 0] + A[:, r0, 1] * A[:, r1, 1]) + A[:, r0, 2] * A[:, r1, 2] for r0 in range(3) for r1 in range(r0, 3)]
    return np.stack(out, -1)


def moments(P, stale_mean, stale_cov):
    """pcl::computeMeanAndCovarianceMatrix (PCL 1.10): nine float accumulators summed in point order, divided by (float)m.  No point:
    mean and covariance are left as they were."""
    m = P.shape[0]
    if m == 0:
        return stale_mean.copy(), stale_cov.copy()
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    terms = [x * x, x * y, x * z, y * y, y * z, z * z, x, y, z]
    acc = [np.cumsum(t, dtype=F)[-1] for t in terms]  # np.cumsum adds strictly in order
    acc = [F(a) / F(m) for a in acc]
    mean = np.array(acc[6:9], F)
    c00, c01, c02 = acc[0] - acc[6] * acc[6], acc[1] - acc[6] * acc[7], acc[2] - acc[6] * acc[8]
    c11, c12, c22 = acc[3] - acc[7] * acc[7], acc[4] - acc[7] * acc[8], acc[5] - acc[8] * acc[8]
    cov = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]], F)
    return mean, cov


def svd3(cov):
    """Singular values (descending) and the third left singular vector of a symmetric 3 x 3 float matrix: cyclic Jacobi in float32,
    the same operations as svd3f in go-rio_amd/csrc/apd_ground.hip."""
    a = [[F(cov[r][c]) for c in range(3)] for r in range(3)]
    v = [[F(1.0) if r == c else F(0.0) for c in range(3)] for r in range(3)]
    one, two, eps, tiny = F(1.0), F(2.0), F(1.1920929e-7), F(1e-37)
    for _ in range(16):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq, app, aqq = a[p][q], a[p][p], a[q][q]
            thr = max(abs(app), abs(aqq)) * eps
            if abs(apq) <= thr or abs(apq) < tiny:
                continue
            rotated = True
            theta = (aqq - app) / (two * apq)
            t = one / (abs(theta) + np.sqrt(theta * theta + one))
            if theta < 0:
                t = -t
            c = one / np.sqrt(t * t + one)
            s = t * c
            for k in range(3):
                akp, akq = a[k][p], a[k][q]
                a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
                vkp, vkq = v[k][p], v[k][q]
                v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
            for k in range(3):
                apk, aqk = a[p][k], a[q][k]
                a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
        if not rotated:
            break
    e = [abs(a[0][0]), abs(a[1][1]), abs(a[2][2])]
    o = [0, 1, 2]
    if e[o[1]] > e[o[0]]:
        o[0], o[1] = o[1], o[0]
    if e[o[2]] > e[o[1]]:
        o[1], o[2] = o[2], o[1]
    if e[o[1]] > e[o[0]]:
        o[0], o[1] = o[1], o[0]
    return np.array([e[k] for k in o], F), np.array([v[k][o[2]] for k in range(3)], F)


def plane_residuals(x, P, C, jac=True):
    """PlaneFitCost (PWP:63-84): r = ((n.p + d)/|n|)^2 / (n^T C n), and its analytic Jacobian w.r.t. (n, d)."""
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    a = ((x[0] * p0 + x[1] * p1) + x[2] * p2) + x[3]
    q = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    sq = math.sqrt(q)
    cn0 = (C[:, 0] * x[0] + C[:, 1] * x[1]) + C[:, 2] * x[2]
    cn1 = (C[:, 1] * x[0] + C[:, 3] * x[1]) + C[:, 4] * x[2]
    cn2 = (C[:, 2] * x[0] + C[:, 4] * x[1]) + C[:, 5] * x[2]
    w = (x[0] * cn0 + x[1] * cn1) + x[2] * cn2
    dist = a / sq
    r = dist * dist / w
    if not jac:
        return r
    g, h = 2.0 * dist / w, 2.0 * r / w
    J = np.stack([g * ((p0 - dist * x[0] / sq) / sq) - h * cn0, g * ((p1 - dist * x[1] / sq) / sq) - h * cn1, g * ((p2 - dist * x[2] / sq) / sq) - h * cn2,
                  g / sq], -1)
    return r, J


def lm_plane(x0, P, C):
    """ceres_like_solve (oracle/ugpm_oracle.cpp) for the 4-parameter plane, max_num_iterations 30 (PWP:552), Ceres' default
    tolerances.  Returns (x, iterations, termination)."""
    Pd = P.astype(np.float64)
    x = np.array(x0, np.float64)
    r, J = plane_residuals(x, Pd, C)
    cost = 0.5 * np.sum(r * r)
    Jtr = J.T @ r
    if np.max(np.abs(Jtr)) <= GTOL:
        return x, 0, 3
    JtJ = J.T @ J
    scale = 1.0 / (1.0 + np.sqrt(np.diag(JtJ)))
    A, g = JtJ * scale[:, None] * scale[None, :], Jtr * scale
    radius, dec, reuse = 1e4, 2.0, False
    diag = np.zeros(4)
    xnorm = math.sqrt(float(np.sum(x * x)))
    it = 0
    while True:
        if it >= MAX_LM_ITER:
            return x, it, 4
        if radius < 1e-32:
            return x, it, 5
        it += 1
        if not reuse:
            diag = np.minimum(np.maximum(np.diag(A), 1e-6), 1e32)
        lhs = A + np.diag(diag / radius)
        valid = True
        try:
            L = np.linalg.cholesky(lhs)
            step = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            valid = bool(np.all(np.isfinite(step)))
        except np.linalg.LinAlgError:
            valid = False
        if valid:
            mcc = -(g @ step + step @ A @ step / 2.0)
            valid = mcc > 0.0
        if not valid:
            radius /= dec
            dec *= 2.0
            reuse = True
            continue
        dx = step * scale
        xn = x + dx
        step_norm = math.sqrt(float(np.sum(dx * dx)))
        rn, Jn = plane_residuals(xn, Pd, C)
        cost_new = 0.5 * np.sum(rn * rn)
        if step_norm <= PTOL * (xnorm + PTOL):
            return x, it, 2
        cc = cost - cost_new
        if abs(cc) <= FTOL * cost:
            return x, it, 1
        rho = cc / mcc
        if rho > 1e-3:
            x, cost = xn, cost_new
            xnorm = math.sqrt(float(np.sum(x * x)))
            Jtr = Jn.T @ rn
            if np.max(np.abs(Jtr)) <= GTOL:
                return x, it, 3
            JtJ = Jn.T @ Jn
            A, g = JtJ * scale[:, None] * scale[None, :], Jtr * scale
            t = 2.0 * rho - 1.0
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - t * t * t))
            dec, reuse = 2.0, False
        else:
            radius /= dec
            dec *= 2.0
            reuse = True


def estimate_plane(P, C, id, stale_mean, stale_cov):
    """estimate_plane (id 0, PWP:461-479) / estimate_plane_cov (id 1, PWP:497-580) over the float points P in order."""
    mean, cov = moments(P, stale_mean, stale_cov)
    sv, n = svd3(cov)
    if n[2] < 0:  # PWP:475 / 527
        n = -n
    d = -((n[0] * mean[0] + n[1] * mean[1]) + n[2] * mean[2])
    it = term = 0
    if id == 1:
        x = np.array([n[0], n[1], n[2], d], np.float64)
        if P.shape[0] > 0:
            x, it, term = lm_plane(x, P, C)
        if x[2] < 0:  # PWP:560-579
            x = -x
        nn = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        x = x / nn
        n, d = x[:3].astype(F), F(x[3])
    return dict(mean=mean, cov=cov, sv=sv, normal=np.asarray(n, F), d=F(d), m=P.shape[0], iters=it, term=term)


def calc_mean_stdev(vec, mean=0.0, stdev=0.0):
    """PWP:1131-1140: nothing for 0 or 1 values; stdev accumulates onto the value passed in."""
    if len(vec) <= 1:
        return mean, stdev
    s = 0.0
    for v in vec:  # std::accumulate, in order
        s += v
    mean = s / len(vec)
    for v in vec:
        stdev += (v - mean) * (v - mean)
    stdev /= len(vec) - 1
    return mean, math.sqrt(stdev)


def erase_under_ground(nonground, xyz, normal, d):
    """PWP:872-884: erase(begin + i) while i advances, so the point after every erased point is never tested.  Returns (kept, tested
    distances) for the margins."""
    ng = list(nonground)
    dists = []
    i = 0
    while i < len(ng):
        x, y, z = (float(v) for v in xyz[ng[i]])
        dist = float(normal[0]) * x + float(normal[1]) * y + float(normal[2]) * z + float(d)
        dists.append(dist)
        if dist < -1.0:
            del ng[i]
        i += 1
    return ng, dists


class Patchworkpp:
    """PatchWorkpp<PointT> (PWP:172-460) with its state across scans."""

    def __init__(self, **overrides):
        p = default_params()
        p.update(overrides)
        if p["enable_RVPF"]:
            raise ValueError("RVPF is not restated (off in the reference and every caller)")
        if p["num_lpr"] < 1 or not p["th_seeds"] > 0:
            # PWP:646-653: lpr_height is 0 with num_lpr = 0, so a patch above th_seeds has no seeds, and the reference's first fit of
            # that patch reads pc_mean_ / cov_ of the previous patch.  patch_chain starts every patch from zeros, as the kernels do.
            raise ValueError("num_lpr must be >= 1 and th_seeds > 0: a patch without seeds would inherit another patch's moments, which is not restated")
        self.p = p
        self.sensor_height = p["sensor_height"]
        self.elevation_thr = list(map(float, p["elevation_thr"]))
        self.flatness_thr = list(map(float, p["flatness_thr"]))
        self.upd_elev = [[] for _ in range(4)]
        self.upd_flat = [[] for _ in range(4)]
        self.last_mean = np.zeros(3, F)
        self.last_cov = np.zeros((3, 3), F)
        mn, mx = p["min_range"], p["max_range"]
        z2, z3, z4 = (7 * mn + mx) / 8.0, (3 * mn + mx) / 4.0, (mn + mx) / 2.0  # PWP:254-272
        R, S = p["num_rings_each_zone"], p["num_sectors_each_zone"]
        self.min_ranges = [mn, z2, z3, z4]
        self.ring_sizes = [(z2 - mn) / R[0], (z3 - z2) / R[1], (z4 - z3) / R[2], (mx - z4) / R[3]]
        self.sector_sizes = [2 * math.pi / S[z] for z in range(4)]
        self.zone_patch_off = list(np.cumsum([0] + [R[z] * S[z] for z in range(3)]))
        self.n_patches = sum(R[z] * S[z] for z in range(4))

    def state(self):
        return dict(elevation_thr=list(self.elevation_thr), flatness_thr=list(self.flatness_thr), sensor_height=self.sensor_height,
                    update_elevation=[list(v) for v in self.upd_elev], update_flatness=[list(v) for v in self.upd_flat])

    def set_state(self, elevation_thr, flatness_thr, sensor_height, update_elevation=None, update_flatness=None):
        self.elevation_thr, self.flatness_thr, self.sensor_height = list(elevation_thr), list(flatness_thr), float(sensor_height)
        self.upd_elev = [list(v) for v in (update_elevation or [[]] * 4)]
        self.upd_flat = [list(v) for v in (update_flatness or [[]] * 4)]

    def labels(self, xyz, intensity):
        """RNR (PWP:657-681) and pc2czm (PWP:1160-1185): -2 noise, -1 out of range, else the patch id."""
        p = self.p
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rn = np.sqrt(x * x + y * y).astype(np.float64)  # sqrt of a float sum
        zd = z.astype(np.float64)
        ver = np.arctan2(zd, rn) * 180 / math.pi
        noise = (ver < p["RNR_ver_angle_thr"]) & (zd < -self.sensor_height - 0.8) & (intensity.astype(np.float64) < p["RNR_intensity_thr"])
        if not p["enable_RNR"]:
            noise[:] = False
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        r = np.sqrt(xd * xd + yd * yd)
        inr = (r <= p["max_range"]) & (r > p["min_range"])
        a = np.arctan2(yd, xd)
        theta = np.where(a > 0, a, 2 * math.pi + a)
        mr = self.min_ranges
        zone = np.where(r < mr[1], 0, np.where(r < mr[2], 1, np.where(r < mr[3], 2, 3)))
        R, S = np.array(p["num_rings_each_zone"]), np.array(p["num_sectors_each_zone"])
        ring = np.minimum(((r - np.array(mr)[zone]) / np.array(self.ring_sizes)[zone]).astype(np.int64), R[zone] - 1)
        sector = np.minimum((theta / np.array(self.sector_sizes)[zone]).astype(np.int64), S[zone] - 1)
        pid = np.array(self.zone_patch_off)[zone] + ring * S[zone] + sector
        lab = np.where(inr, pid, -1)
        lab[noise] = -2
        return lab.astype(np.int32)

    def patch_chain(self, zone, P_sorted, C_sorted, id):
        """extract_piecewiseground with RVPF off (PWP:1024-1128), 2-argument extract_initial_seeds (PWP:621-655)."""
        p = self.p
        z = P_sorted[:, 2].astype(np.float64)
        init_idx = 0
        if zone == 0:
            init_idx = int(np.sum(z < p["adaptive_seed_selection_margin"] * self.sensor_height))
        s, cnt = 0.0, 0
        for k in range(init_idx, len(z)):
            if cnt >= p["num_lpr"]:
                break
            s += z[k]
            cnt += 1
        lpr = s / cnt if cnt != 0 else 0
        sel = z < lpr + p["th_seeds"]
        zero_m, zero_c = np.zeros(3, F), np.zeros((3, 3), F)
        fits = [estimate_plane(P_sorted[sel], C_sorted[sel], id, zero_m, zero_c)]
        margin = math.inf
        zmax = -self.sensor_height + 0.5
        for _ in range(p["num_iter"]):
            f = fits[-1]
            n = f["normal"]
            res = (P_sorted[:, 0] * n[0] + P_sorted[:, 1] * n[1]) + P_sorted[:, 2] * n[2]  # float32, un-fused
            thr = p["th_dist"] - float(f["d"])
            zok = z < zmax
            sel = (res.astype(np.float64) < thr) & zok
            if np.any(zok):
                margin = min(margin, float(np.min(np.abs(res.astype(np.float64)[zok] - thr))))
            fits.append(estimate_plane(P_sorted[sel], C_sorted[sel], id, f["mean"], f["cov"]))
        return fits, sel, margin

    def estimate_ground(self, xyz, intensity, id=1):
        """One estimate_ground call (PWP:684-890).  Returns a dict: ground, nonground (index arrays), labels, patch_order, patches,
        final (the plane of the under-ground pass), margin (the smallest distance of a decisive quantity that rests on the LM plane
        to its threshold)."""
        p = self.p
        xyz = np.ascontiguousarray(xyz, F)
        intensity = np.asarray(intensity, F)
        n = xyz.shape[0]
        lab = self.labels(xyz, intensity)
        nonground = list(np.nonzero(lab == -2)[0]) + list(np.nonzero(lab == -1)[0])
        ground = []
        patches, order = [], []
        margin = math.inf
        candidates, ringwise_flatness = [], []
        concentric_idx = 0
        R, S = p["num_rings_each_zone"], p["num_sectors_each_zone"]
        for zone in range(4):
            for ring in range(R[zone]):
                for sector in range(S[zone]):
                    pi = self.zone_patch_off[zone] + ring * S[zone] + sector
                    members = np.nonzero(lab == pi)[0]
                    rec = dict(zone=zone, ring=ring, sector=sector, concentric_idx=concentric_idx, n_points=len(members), segment_offset=len(order), decision=0)
                    patches.append(rec)
                    if len(members) < p["num_min_pts"]:  # PWP:734-738
                        order += list(members)
                        nonground += list(members)
                        continue
                    srt = members[np.lexsort((members, xyz[members, 2]))]  # (z, input index)
                    order += list(srt)
                    Ps = xyz[srt]
                    fits, sel, mg = self.patch_chain(zone, Ps, range_covariance(Ps), id)
                    if id == 1:
                        margin = min(margin, mg)
                    f = fits[-1]
                    self.last_mean, self.last_cov = f["mean"], f["cov"]
                    rg, rn = list(srt[sel]), list(srt[~sel])
                    sv = f["sv"]
                    upr, elev = float(f["normal"][2]), float(f["mean"][2])  # PWP:751-756
                    flat = float(min(sv))
                    line_var = float(sv[0] / sv[1]) if sv[1] != 0 else np.finfo(np.float64).max
                    heading = 0.0
                    for i in range(3):
                        heading += float(f["mean"][i] * f["normal"][i])
                    rec.update(fits=fits, n_ground=len(rg), uprightness=upr, elevation=elev, flatness=flat, line_variable=line_var, heading=heading)
                    near = concentric_idx < 4
                    upright = upr > p["uprightness_thr"]
                    not_elev = near and elev < self.elevation_thr[concentric_idx]
                    is_flat = near and flat < self.flatness_thr[concentric_idx]
                    heading_out = heading < 0.0
                    if id == 1:
                        margin = min(margin, abs(upr - p["uprightness_thr"]))
                        if near and upright:
                            margin = min(margin, abs(heading))
                    if upright and not_elev and near:  # PWP:785-791
                        self.upd_elev[concentric_idx].append(elev)
                        self.upd_flat[concentric_idx].append(flat)
                        ringwise_flatness.append(flat)
                    if not upright:
                        rec["decision"] = 1
                        nonground += rg
                    elif not near:
                        rec["decision"] = 2
                        ground += rg
                    elif not heading_out:
                        rec["decision"] = 3
                        nonground += rg
                    elif not_elev or is_flat:
                        rec["decision"] = 4
                        ground += rg
                    else:
                        candidates.append((rec, flat, line_var, rg))
                    nonground += rn
                if candidates:  # PWP:838-856
                    if p["enable_TGR"]:  # PWP:952-1018
                        mf, sf = calc_mean_stdev(ringwise_flatness)
                        for rec, flat, line_var, rg in candidates:
                            mu = mf + 1.5 * sf
                            try:
                                prob_flat = 1 / (1 + math.exp((flat - mu) / (mu / 10)))
                            except (ZeroDivisionError, OverflowError):
                                prob_flat = _c_prob(flat, mu)
                            if len(rg) > 1500 and flat < p["th_dist"] * p["th_dist"]:
                                prob_flat = 1.0
                            prob_line = 0.0 if line_var > 8.0 else 1.0
                            revert = prob_line * prob_flat > 0.5
                            if concentric_idx < 4:
                                rec["decision"] = 5 if revert else 6
                                (ground if revert else nonground).extend(rg)
                    else:
                        for rec, flat, line_var, rg in candidates:
                            rec["decision"] = 6
                            nonground += rg
                    candidates, ringwise_flatness = [], []
                concentric_idx += 1
        for i in range(4):  # update_elevation_thr, PWP:894-922
            if not self.upd_elev[i]:
                continue
            mean, stdev = calc_mean_stdev(self.upd_elev[i])
            if i == 0:
                self.elevation_thr[i] = mean + 3 * stdev
                self.sensor_height = -mean
            else:
                self.elevation_thr[i] = mean + 2 * stdev
            ex = len(self.upd_elev[i]) - p["max_elevation_storage"]
            if ex > 0:
                del self.upd_elev[i][:ex]
        for i in range(4):  # update_flatness_thr, PWP:924-950
            if len(self.upd_flat[i]) <= 1:
                break
            mean, stdev = calc_mean_stdev(self.upd_flat[i])
            self.flatness_thr[i] = mean + stdev
            ex = len(self.upd_flat[i]) - p["max_flatness_storage"]
            if ex > 0:
                del self.upd_flat[i][:ex]
        gi = np.array(ground, np.int64)
        Pg = xyz[gi] if len(gi) else np.zeros((0, 3), F)
        final = estimate_plane(Pg, range_covariance(Pg), id, self.last_mean, self.last_cov)  # PWP:866-867
        self.last_mean, self.last_cov = final["mean"], final["cov"]
        kept, dists = erase_under_ground(nonground, xyz, final["normal"], final["d"])
        if id == 1 and dists:
            margin = min(margin, float(np.min(np.abs(np.array(dists) + 1.0))))
        order = np.array(order + [-1] * (n - len(order)), np.int64)
        return dict(ground=gi, nonground=np.array(kept, np.int64), labels=lab, patch_order=order, patches=patches, final=final, margin=margin)


def _c_prob(flat, mu):
    """1 / (1 + exp((flat - mu) / (mu / 10))) with C's IEEE rules where Python raises (mu = 0, overflow)."""
    with np.errstate(all="ignore"):
        return float(np.float64(1) / (np.float64(1) + np.exp((np.float64(flat) - mu) / (np.float64(mu) / 10))))
