"""NumPy restatement of SCManager, the Intensity Scan Context loop-candidate search, the yardstick of include/gorio_sc.h.

SC = src/radar_graph_slam/Scancontext.cpp, SCH = include/scan_context/Scancontext.h, NF = include/scan_context/nanoflann.hpp (v1.3.2)
of the Go-RIO sources.  Float quantities stay float32 in the reference's evaluation order, double ones float64.  Choices the
reference leaves open are the project's (include/gorio_sc.h): atan2f is taken as correctly rounded, abs(azim_angle) as the float
overload, every sum in index order, and k-NN ties to the lower snapshot position.
"""
import numpy as np

F = np.float32
RINGS, SECTORS, MAX_RADIUS = 40, 20, 80.0  # SCH:112-114
EXCLUDE_RECENT, CANDIDATES, TREE_PERIOD = 10, 3, 10  # SCH:119-120, 129
SEARCH_RADIUS = int(round(0.5 * 0.1 * SECTORS))  # SC:134, SEARCH_RATIO 0.1 (SCH:123): 1
NO_POINT = -1000.0  # SC:170
BIG = 10000000.0  # the 1e7 the argmins start from (SC:107, 144, 312)
FLT_MAX = np.finfo(F).max


def bin_indices(x, y, azimuth_range):
    """SC:180-195 for float32 arrays x, y: (keep mask, ring 1..40, sector 1..20, azimuth float32, range float32)."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(invalid="ignore", over="ignore"):
        rr = np.sqrt(x * x + y * y)  # SC:183: float sqrt of float sum
        a = np.arctan2(x.astype(np.float64), y.astype(np.float64)).astype(F)  # atan2f, correctly rounded
        az = (((a.astype(np.float64) - np.pi / 2) * 180.0) / np.pi).astype(F)  # SC:185, double, stored as float
        keep = ~(np.abs(az).astype(np.float64) > azimuth_range) & ~(rr.astype(np.float64) > MAX_RADIUS)  # SC:187-191: NaN passes both
        rv = np.ceil((rr.astype(np.float64) / MAX_RADIUS) * RINGS)  # SC:193
        sv = np.ceil(((az.astype(np.float64) - (-azimuth_range)) / (azimuth_range - (-azimuth_range))) * SECTORS)  # SC:195
    # int(NaN) is INT_MIN on x86, and std::max(std::min(N, INT_MIN), 1) = 1
    ring = np.where(np.isnan(rv), 1, np.clip(np.nan_to_num(rv, nan=1.0), 1, RINGS)).astype(np.int64)
    sec = np.where(np.isnan(sv), 1, np.clip(np.nan_to_num(sv, nan=1.0), 1, SECTORS)).astype(np.int64)
    return keep, ring, sec, az, rr


def make_scancontext(xyz, intensity, azimuth_range=56.5):
    """makeScancontext (SC:162-215): [40, 20] float64, each bin the maximum intensity, -1000 -> 0.  z is never used (SC:182)."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    inten = np.asarray(intensity, F).reshape(-1)
    desc = np.full((RINGS, SECTORS), NO_POINT)
    if xyz.shape[0] == 0:
        return np.where(desc == NO_POINT, 0.0, desc)
    keep, ring, sec, _, _ = bin_indices(xyz[:, 0], xyz[:, 1], azimuth_range)
    keep &= inten.astype(np.float64) > NO_POINT  # desc < intensity, strict (SC:201): NaN and <= -1000 never update
    np.maximum.at(desc, (ring[keep] - 1, sec[keep] - 1), inten[keep].astype(np.float64))
    return np.where(desc == NO_POINT, 0.0, desc)  # SC:205-209


def ring_key(desc):
    """makeRingkeyFromScancontext (SC:219-229): row means, summed in index order."""
    s = np.zeros(RINGS)
    for c in range(SECTORS):
        s = s + desc[:, c]
    return s / float(SECTORS)


def sector_key(desc):
    """makeSectorkeyFromScancontext (SC:235-245): column means, summed in index order."""
    s = np.zeros(SECTORS)
    for r in range(RINGS):
        s = s + desc[r, :]
    return s / float(RINGS)


def col_norms(desc):
    """VectorXd::norm of every column, index order."""
    s = np.zeros(SECTORS)
    for r in range(RINGS):
        s = s + desc[r, :] * desc[r, :]
    return np.sqrt(s)


def circshift(mat, num_shift):
    """SC:42-62: column c moves to (c + num_shift) mod cols."""
    assert num_shift >= 0
    out = np.zeros_like(mat)
    for c in range(mat.shape[1]):
        out[:, (c + num_shift) % mat.shape[1]] = mat[:, c]
    return out


def fast_align(vkey1, vkey2):
    """fastAlignUsingVkey (SC:104-122): strict argmin from 1e7 of ||vkey1 - circshift(vkey2, s)|| (after the sqrt)."""
    v1, v2 = np.asarray(vkey1, np.float64).reshape(-1), np.asarray(vkey2, np.float64).reshape(-1)
    n = v1.shape[0]
    shifted = np.stack([circshift(v2.reshape(1, -1), s)[0] for s in range(n)])  # [shift, column]
    sq = np.zeros(n)
    for j in range(n):  # index order
        diff = v1[j] - shifted[:, j]
        sq = sq + diff * diff
    norms = np.sqrt(sq)
    arg, best = 0, BIG
    for s in range(n):
        if norms[s] < best:
            arg, best = s, norms[s]
    return arg


def dist_direct(sc1, sc2):
    """distDirectSC (SC:80-101): 1 - mean cosine over the columns where neither side has norm 0; NaN without such a column."""
    n1, n2 = col_norms(sc1), col_norms(sc2)
    dot = np.zeros(sc1.shape[1])
    for r in range(sc1.shape[0]):  # index order
        dot = dot + sc1[r, :] * sc2[r, :]
    total, n_eff = 0.0, 0
    for c in range(sc1.shape[1]):
        if n1[c] == 0 or n2[c] == 0:
            continue
        total = total + dot[c] / (n1[c] * n2[c])
        n_eff += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - np.float64(total) / np.float64(n_eff)


def search_shifts(align):
    """SC:134-141: {a, a + 1, a - 1} mod 20, sorted ascending."""
    space = [align]
    for ii in range(1, SEARCH_RADIUS + 1):
        space.append((align + ii + SECTORS) % SECTORS)
        space.append((align - ii + SECTORS) % SECTORS)
    return sorted(space)


def distance(sc1, sc2):
    """distanceBtnScanContext (SC:127-160) -> (min_sc_dist, argmin_shift); (1e7, 0) when every shift gives NaN."""
    align = fast_align(sector_key(sc1), sector_key(sc2))
    arg, best = 0, BIG
    for s in search_shifts(align):
        d = dist_direct(sc1, circshift(sc2, s))
        if d < best:  # strict: a NaN never wins
            arg, best = s, d
    return float(best), arg


def key_distances(query_key_f, keys_f):
    """L2_Adaptor::evalMetric (NF:383-406) in float32: four squared differences per group, the group summed left to right, then
    added to the running result.  query [40] float32, keys [m, 40] float32 -> [m] float32."""
    d = (np.asarray(query_key_f, F)[None, :] - np.asarray(keys_f, F)).astype(F)
    sq = (d * d).astype(F)
    res = np.zeros(d.shape[0], F)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(RINGS // 4):
            grp = ((sq[:, 4 * g] + sq[:, 4 * g + 1]) + sq[:, 4 * g + 2]) + sq[:, 4 * g + 3]
            res = (res + grp).astype(F)
    return res


def knn(query_key_f, keys_f):
    """KNNResultSet<float>(3) filled by the kd-tree (SC:317-324, NF:158-190): (positions [3], squared distances [3] float32, found).
    The index vector is zero-initialised and init() sets only the last distance to FLT_MAX; an empty snapshot returns before any
    search (NF:1225).  Only distances below FLT_MAX enter (NF:1360); ties go to the lower position."""
    pos = np.zeros(CANDIDATES, np.int64)
    dist = np.zeros(CANDIDATES, F)
    dist[-1] = FLT_MAX
    keys_f = np.asarray(keys_f, F).reshape(-1, RINGS)
    if keys_f.shape[0] == 0:
        return pos, dist, 0
    d = key_distances(query_key_f, keys_f)
    ok = np.nonzero(d < FLT_MAX)[0]
    order = ok[np.lexsort((ok, d[ok]))][:CANDIDATES]
    pos[:len(order)] = order
    dist[:len(order)] = d[order]
    return pos, dist, len(order)


def yaw_rad(nn_align, azimuth_range):
    """deg2rad(nn_align * PC_UNIT_SECTOR_ANGLE) (SC:18-21, 369): the product in double, passed as float, returned as float."""
    unit = (azimuth_range - (-azimuth_range)) / float(SECTORS)  # SC:72
    deg = F(nn_align * unit)
    return F(np.float64(deg) * np.pi / 180.0)


class SCManagerRef:
    """SCManager with LoopDetector's two settings (LD:88-89)."""

    def __init__(self, sc_dist_thresh=0.5, azimuth_range=56.5):
        self.thresh, self.range = sc_dist_thresh, azimuth_range
        self.descs, self.ring_keys, self.sector_keys, self.ring_keys_f = [], [], [], []
        self.counter = 0
        self.snapshot = []  # database indices in snapshot position order

    def add_scan(self, xyz, intensity):
        """makeAndSaveScancontextAndKeys (SC:255-269)."""
        d = make_scancontext(xyz, intensity, self.range)
        rk = ring_key(d)
        self.descs.append(d)
        self.ring_keys.append(rk)
        self.sector_keys.append(sector_key(d))
        self.ring_keys_f.append(rk.astype(F))  # eig2stdvec (SC:73-77): KeyMat of float
        return len(self.descs) - 1

    def distance(self, i, j):
        return distance(self.descs[i], self.descs[j])

    def detect(self, query, candidates):
        """detectLoopClosureID (SC:272-373) -> (loop_id, yaw (float32), min_dist, diag dict as include/gorio_sc.h defines it)."""
        candidates = [int(c) for c in candidates]
        if not candidates:
            raise ValueError("empty candidate list")  # the reference indexes out of bounds; the ABI refuses
        diag = dict(early_return=0, rebuilt=0, counter=0, snapshot_size=0, n_found=0, position=np.zeros(3, np.int64), key_dist=np.zeros(3, F),
                    keyframe=np.full(3, -1), sc_dist=np.full(3, np.nan), sc_shift=np.full(3, -1))
        if query < EXCLUDE_RECENT:  # SC:284-288, the counter does not change
            diag.update(early_return=1, counter=self.counter)
            return -1, F(0.0), BIG, diag
        if self.counter % TREE_PERIOD == 0:  # SC:294-306; size_t arithmetic: a candidate after the query wraps and is kept
            self.snapshot = [c for c in candidates if (query - c) % (1 << 64) >= EXCLUDE_RECENT]
            diag["rebuilt"] = 1
        self.counter += 1
        keys = np.array([self.ring_keys_f[i] for i in self.snapshot], F).reshape(-1, RINGS)
        pos, kd, found = knn(self.ring_keys_f[query], keys)
        diag.update(counter=self.counter, snapshot_size=len(self.snapshot), n_found=found, position=pos, key_dist=kd)
        min_dist, nn_align, nn_idx = BIG, 0, 0
        for k in range(CANDIDATES):  # SC:330-348, positions mapped through THIS call's candidate list
            if pos[k] > len(candidates) - 1:
                continue
            kf = candidates[pos[k]]
            d, s = distance(self.descs[query], self.descs[kf])
            diag["keyframe"][k], diag["sc_dist"][k], diag["sc_shift"][k] = kf, d, s
            if d < min_dist:
                min_dist, nn_align, nn_idx = d, s, kf
        loop_id = nn_idx if min_dist < self.thresh else -1  # SC:354-356
        return loop_id, yaw_rad(nn_align, self.range), min_dist, diag
