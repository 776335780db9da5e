"""NumPy restatement of pcl::ApproximateVoxelGrid as include/gorio_prep.h defines it (recalled from PCL 1.10
filters/impl/approximate_voxel_grid.hpp; parity as recalled, unpinned): the sequential history-table loop, and the parallel form the
device kernels implement (csrc/apd_approx_voxel.hip).  float32 arithmetic throughout, the hash wrapped to 32 bits.

    python tests/approx_voxel_restatement.py      # self-test: both forms agree bit for bit on seven random clouds
"""
import numpy as np

HIST = 512
CELL_LIMIT = np.float32(2.0 ** 30)


class Refused(ValueError):
    """A non-finite coordinate, or a cell coordinate outside (-2^30, 2^30): the library answers GORIO_ERR_INVALID."""


def leaf3(leaf):
    return np.broadcast_to(np.asarray(leaf, np.float64).reshape(-1), (3,)).astype(np.float32)


def cells(p, leaf):
    """Cell coordinates [n, 3] int64: (int)floorf(p[a] * (1.0f / leaf[a]))."""
    p = np.asarray(p, np.float32)
    inv = (np.float32(1.0) / leaf3(leaf)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor((p[:, :3] * inv[None, :]).astype(np.float32))
        ok = np.abs(fl) < CELL_LIMIT  # false for NaN and the infinities
    if not ok.all():
        raise Refused("a coordinate is not finite or a cell coordinate leaves (-2^30, 2^30)")
    return fl.astype(np.int64)


def bucket(c):
    """(uint32)(c0 * 7171 + c1 * 3079 + c2 * 4231) & 511 with the sum wrapped to 32 bits (two's complement)."""
    h = (c[:, 0] * 7171 + c[:, 1] * 3079 + c[:, 2] * 4231) & 0xFFFFFFFF
    return (h & (HIST - 1)).astype(np.int64)


def sequential(p, leaf):
    """The definition: 512 history entries, eviction on a different cell, the final flush in ascending bucket order."""
    p = np.ascontiguousarray(p, np.float32)
    n, nf = p.shape
    if n == 0:
        return np.zeros((0, nf), np.float32)
    c = cells(p, leaf)
    b = bucket(c)
    cnt = [0] * HIST
    cell = [None] * HIST
    acc = [None] * HIST
    ct = [tuple(r) for r in c.tolist()]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            k = b[i]
            if cnt[k] and cell[k] != ct[i]:
                out.append(acc[k] / np.float32(cnt[k]))
                cnt[k] = 0
            if cnt[k] == 0:
                acc[k] = np.zeros(nf, np.float32)
            cell[k] = ct[i]
            cnt[k] += 1
            acc[k] = acc[k] + p[i]
        for k in range(HIST):
            if cnt[k]:
                out.append(acc[k] / np.float32(cnt[k]))
    return np.array(out, np.float32).reshape(-1, nf)


def parallel(p, leaf):
    """The parallel form of DESIGN.md section 4: stable order by bucket, runs, evictor ranks, in-order sums."""
    p = np.ascontiguousarray(p, np.float32)
    n, nf = p.shape
    if n == 0:
        return np.zeros((0, nf), np.float32)
    c = cells(p, leaf)
    b = bucket(c)
    order = np.argsort(b, kind="stable")  # key (bucket, input index)
    bs, cs = b[order], c[order]
    start = np.ones(n, bool)
    start[1:] = (cs[1:] != cs[:-1]).any(1)  # equal cells share a bucket, so a bucket change is a cell change too
    evicting = start.copy()
    evicting[0] = False
    evicting[1:] &= bs[1:] == bs[:-1]  # a run that is not the first of its bucket: its first point evicts the run before it
    is_ev = np.zeros(n, np.int64)
    is_ev[order[evicting]] = 1
    rank = np.cumsum(is_ev) - is_ev  # evicting points with a smaller input index
    nev = int(is_ev.sum())
    starts = np.flatnonzero(start)
    ends = np.append(starts[1:], n)
    nonempty = np.zeros(HIST, np.int64)
    nonempty[np.unique(b)] = 1
    finrank = np.cumsum(nonempty) - nonempty
    out = np.zeros((nev + int(nonempty.sum()), nf), np.float32)
    assert out.shape[0] == len(starts)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, e in zip(starts, ends):
            a = np.zeros(nf, np.float32)
            for j in order[s:e]:
                a = a + p[j]
            pos = rank[order[e]] if e < n and evicting[e] else nev + finrank[bs[s]]
            out[pos] = a / np.float32(e - s)
    return out


def self_test():
    rng = np.random.default_rng(0)
    for n, span, leaf in [(0, 1, 0.5), (1, 1, 0.5), (700, 3, 0.5), (3000, 40, 0.25), (3000, 2, 1.0), (2000, 200, 0.1), (513, 1000, 0.01)]:
        p = (rng.standard_normal((n, 4)) * span).astype(np.float32)
        a, q = sequential(p, leaf), parallel(p, leaf)
        assert a.shape == q.shape and a.tobytes() == q.tobytes(), (n, span, leaf)
        print(f"n={n} span={span} leaf={leaf}: {len(a)} outputs, forms agree")


if __name__ == "__main__":
    self_test()
