"""NumPy float32 brute-force restatement of include/gorio_search.h, written from its definitions (not from the kernels):

  distance   ((dx * dx) + dy * dy) + dz * dz, every operation rounded to float32 (FLANN L2_Simple, un-fused)
  k-NN       the first min(k, n) of the cloud ordered by (distance, original index); unused slots -1 / +inf; count = min(k, n)
  radius     the points with distance < float32(float64(r) * float64(r)), strictly, ordered by (distance, original index);
             max_nn > 0 keeps the first max_nn of that order
  a query with a non-finite coordinate has no neighbour at all

test_search_restatement.py pins it against the oracle's knn_self; the GPU tests compare with it for exact equality."""
import numpy as np

CHUNK = 256  # queries per distance block (memory only)


def sqdist(q, xyz):
    """[nq, n] float32 squared distances, un-fused."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = None
        for a in range(3):
            diff = q[:, None, a] - x[None, :, a]
            d = diff * diff if d is None else d + diff * diff
    return d.astype(np.float32, copy=False)


def _finite(q):
    return np.isfinite(q).all(axis=1)


def _ordered(drow):
    """indices of one query's row ordered by (distance, index)"""
    return np.lexsort((np.arange(drow.shape[0]), drow))


def knn(xyz, queries, k):
    """(idx [nq, k] int32, sqd [nq, k] float32, count [nq] int32); queries None = the cloud itself."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    q = x if queries is None else np.asarray(queries, np.float32).reshape(-1, 3)
    nq, n = q.shape[0], x.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    sqd = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.int32)
    live = _finite(q)
    m = min(k, n)
    for b in range(0, nq, CHUNK):
        d = sqdist(q[b:b + CHUNK], x)
        for r in range(d.shape[0]):
            if not live[b + r] or m == 0:
                continue
            o = _ordered(d[r])[:m]
            idx[b + r, :m] = o
            sqd[b + r, :m] = d[r, o]
            cnt[b + r] = m
    return idx, sqd, cnt


def radius_bound(radius):
    """float32(r * r) with the product in float64"""
    return np.float32(np.float64(radius) * np.float64(radius))


def radius(xyz, queries, radius_m, max_nn=0):
    """CSR (offsets [nq + 1] int64, idx [total] int32, sqd [total] float32); queries None = the cloud itself."""
    x = np.asarray(xyz, np.float32).reshape(-1, 3)
    q = x if queries is None else np.asarray(queries, np.float32).reshape(-1, 3)
    nq = q.shape[0]
    r2 = radius_bound(radius_m)
    live = _finite(q)
    offs = np.zeros(nq + 1, np.int64)
    idx, sqd = [], []
    for b in range(0, nq, CHUNK):
        d = sqdist(q[b:b + CHUNK], x)
        for r in range(d.shape[0]):
            o = np.zeros(0, np.int64)
            if live[b + r] and x.shape[0]:
                inside = np.nonzero(d[r] < r2)[0]  # strict
                o = inside[np.lexsort((inside, d[r, inside]))]
                if max_nn > 0:
                    o = o[:max_nn]
            idx.append(o.astype(np.int32))
            sqd.append(d[r, o].astype(np.float32) if o.size else np.zeros(0, np.float32))
            offs[b + r + 1] = offs[b + r] + o.size
    return offs, (np.concatenate(idx) if idx else np.zeros(0, np.int32)), (np.concatenate(sqd) if sqd else np.zeros(0, np.float32))
