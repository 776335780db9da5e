"""Structure of the search index as run_index_build leaves it (bbox_morton_kernel, the bitonic Morton sort, kd_refine_kernel with its
gather, sorted-segment skipping and tile / super-tile boxes, box_block_kernel), read back through gorio_apd_debug_get_index and
compared with a NumPy restatement, written here, of "chunk by Morton rank, then median splits on the widest axis":

  * keys  (33-bit Morton code of the point in cubic cells of the cloud's bounding box) << 31 | index, sorted; chunk c holds the ranks
    c * kd_chunk .. (c + 1) * kd_chunk - 1, positions past n are padding (1e30, original index 0x7fffffff);
  * per level (segments of kd_chunk .. 64 positions): widest axis of the segment's valid points (the lowest axis among equal extents),
    ascending sort of the segment on (coordinate, position before the level), split in halves.

What is asserted for every case: `orig` is a permutation of 0 .. n - 1 followed by padding only; sx / sy / sz / s4 are the points `orig`
names; every tile, super-tile and block box is the exact min / max of its points (empty: +inf / -inf); the SET of points of every
32-point leaf equals the restatement's, and -- because the build keeps the tie-break (position) of the restatement, which is what lets
kd_refine_kernel skip segments that are sorted already -- so does the whole permutation.  A leaf that holds a point of a tied median
(equal split coordinates on both sides of a median) is left out of the set comparison, as either side would be a valid split; the
share left out is printed, is 0 on the inputs with distinct coordinates and stays under 5 % on the input with duplicated points
(test_inputs_keep_their_tie_share checks that on the CPU with the restatement alone).
"""
import importlib

import numpy as np
import pytest

PAD = 0x7FFFFFFF
SMALL_CLOUD = 131072  # kKdSmallCloud: kd chunks of 2048 points up to here, 4096 above
SIZES = (1, 31, 32, 33, 2047, 2048, 2049, 16384, 100000, 140000)
CASES = [("distinct", n) for n in SIZES] + [("duplicates", 16384), ("planar", 16384)]
DUP_SHARE_MAX = 0.05


# ------------------------------------------------------------------------------------------------------------------------ inputs

def make(kind, n, seed=5):
    """distinct: every coordinate of every axis occurs once (a shuffled 1 mm grid per axis, scaled 10 : 3 : 1 so that some segments keep
    their parent's widest axis -- the ones kd_refine_kernel does not sort again -- and others change it); duplicates: 256 of the 16 384 points (one in 64) are exact copies of others -- the share of
    leaves left out grows with the share of copies, one in 48 already passes 5 %; planar: z constant, x and y distinct."""
    rng = np.random.default_rng(seed + n)
    xyz = np.stack([(rng.permutation(n) - n / 2) * s for s in (1e-3, 0.3e-3, 0.1e-3)], axis=1)
    xyz = (xyz * (100000.0 / max(n, 1000))).astype(np.float32)
    if kind == "duplicates":
        dst = rng.choice(n, n // 64, replace=False)
        src = rng.choice(np.setdiff1d(np.arange(n), dst), n // 64)
        xyz[dst] = xyz[src]
    elif kind == "planar":
        xyz[:, 2] = np.float32(1.25)
    return np.ascontiguousarray(xyz)


def distinct_axes(xyz):
    return [len(np.unique(xyz[:, a])) == len(xyz) for a in range(3)]


# ------------------------------------------------------------------------------------------------------------------- restatement

def f2ord(f):
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def spread11(v):
    x = v.astype(np.uint64) & np.uint64(0x7FF)
    for sh, m in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(m)
    return x


def morton_order(xyz):
    """original indices in the order of the sorted keys (float32 arithmetic throughout, as the kernel)"""
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    ext = np.float32(max(np.float32(1e-6), (hi - lo).max()))
    t = (xyz - lo) / ext * np.float32(2047.0)
    assert t.dtype == np.float32
    q = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(2047.0)).astype(np.uint32)
    code = spread11(q[:, 0]) | (spread11(q[:, 1]) << np.uint64(1)) | (spread11(q[:, 2]) << np.uint64(2))
    key = (code << np.uint64(31)) | np.arange(len(xyz), dtype=np.uint64)
    return np.argsort(key, kind="stable")


def restate(xyz, chunk):
    """-> (orig [n_spad], tied [n_spad], kept): the index order, which positions hold a point of a tied median, and how many segments
    with a valid point had the widest axis of their parent (their sort is the identity)"""
    n = len(xyz)
    n_spad = -(-n // 512) * 512
    n_chunks = -(-n_spad // chunk)
    total = n_chunks * chunk
    orig = np.full(total, PAD, np.int64)
    orig[:n] = morton_order(xyz)
    pts = np.full((total, 3), np.float32(1e30), np.float32)
    pts[:n] = xyz[orig[:n]]
    tied = np.zeros(total, bool)
    seg, kept, parent_axis = chunk, 0, None
    while seg >= 64:
        P = pts.reshape(-1, seg, 3)
        valid = (orig != PAD).reshape(-1, seg)
        lo = np.where(valid[..., None], P, np.float32(np.inf)).min(axis=1)
        hi = np.where(valid[..., None], P, np.float32(-np.inf)).max(axis=1)
        ext = np.where(hi >= lo, hi - lo, np.float32(0.0))  # a segment of padding only: 0 on every axis
        axis = ext.argmax(axis=1)  # the first among equals
        if parent_axis is not None:
            kept += int(((axis == np.repeat(parent_axis, 2)) & valid.any(axis=1)).sum())
        parent_axis = axis
        c = np.take_along_axis(P, axis[:, None, None], axis=2)[..., 0]
        key = (f2ord(c).astype(np.uint64).reshape(-1, seg) << np.uint64(12)) | (np.arange(total, dtype=np.uint64) % np.uint64(chunk)).reshape(-1, seg)
        perm = np.argsort(key, axis=1, kind="stable") + (np.arange(total // seg) * seg)[:, None]
        perm = perm.reshape(-1)
        pts, orig, tied = pts[perm], orig[perm], tied[perm]
        cs = np.take_along_axis(pts.reshape(-1, seg, 3), axis[:, None, None], axis=2)[..., 0]
        v = (orig != PAD).reshape(-1, seg)
        m = seg // 2
        is_tie = (cs[:, m - 1] == cs[:, m]) & v[:, m - 1] & v[:, m]
        tied |= ((cs == cs[:, m : m + 1]) & v & is_tie[:, None]).reshape(-1)
        seg //= 2
    return orig[:n_spad].astype(np.int32), tied[:n_spad], kept


def left_out(tied):
    """per 32-point leaf: holds a point of a tied median"""
    return tied.reshape(-1, 32).any(axis=1)


# ------------------------------------------------------------------------------------------------------------------------- tests

def test_inputs_keep_their_tie_share():
    """the restatement alone: distinct inputs have distinct coordinates on every axis and no tied median; the planar input none on the
    axes that are ever split; the input with duplicates stays under DUP_SHARE_MAX"""
    for kind, n in CASES:
        xyz = make(kind, n)
        chunk = 2048 if n <= SMALL_CLOUD else 4096
        orig, tied, kept = restate(xyz, chunk)
        assert np.array_equal(np.sort(orig[orig != PAD]), np.arange(n))
        share = float(left_out(tied).mean())
        print(f"{kind} n={n}: leaves left out {share:.4f}, segments in order before their sort {kept}")
        assert kept > 0 or n < 2048  # the path that skips a sort is exercised
        if kind == "distinct":
            assert distinct_axes(xyz) == [True, True, True] and share == 0.0
        elif kind == "planar":
            assert distinct_axes(xyz) == [True, True, False] and share == 0.0
        else:
            assert len(np.unique(xyz, axis=0)) <= n - n // 64 and 0.0 < share < DUP_SHARE_MAX


def boxes_of(ix, group):
    """exact min / max of the index's own points per `group` positions (positions from n on are padding and do not count)"""
    n, n_spad = ix["n"], ix["n_spad"]
    pts = np.stack([ix["sx"], ix["sy"], ix["sz"]], axis=1)
    m = -(-n_spad // group)
    full = np.full((m * group, 3), np.float32(1e30), np.float32)
    full[:n_spad] = pts
    real = (np.arange(m * group) < n)[:, None]
    lo = np.where(real, full, np.float32(np.inf)).reshape(m, group, 3).min(axis=1)
    hi = np.where(real, full, np.float32(-np.inf)).reshape(m, group, 3).max(axis=1)
    z = np.zeros((m, 1), np.float32)
    return np.concatenate([lo, z, hi, z], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", CASES)
def test_index_structure(gpu, gorio, kind, n):
    xyz = make(kind, n)
    src = np.ascontiguousarray(xyz[: min(n, 64)])
    g = gorio.ApdGicp(search=1)
    g.setInputTarget(xyz, None)
    g.setInputSource(src, None)
    g.setSourceCovariances(np.tile(np.eye(4), (len(src), 1, 1)))  # only the index build and one search run
    g.setTargetCovariances(np.tile(np.eye(4), (n, 1, 1)))
    g.linearize(np.eye(4))
    ix = g.debugGetIndex(1)
    chunk = 2048 if n <= SMALL_CLOUD else 4096
    n_spad = -(-n // 512) * 512
    assert (ix["n"], ix["n_spad"], ix["kd_chunk"]) == (n, n_spad, chunk)
    orig = ix["orig"]
    # a permutation with the padding at the tail, and the points it names
    assert np.array_equal(np.sort(orig[:n]), np.arange(n)) and np.all(orig[n:] == PAD)
    want_pts = np.full((n_spad, 3), np.float32(1e30), np.float32)
    want_pts[:n] = xyz[orig[:n]]
    for a, name in enumerate(("sx", "sy", "sz")):
        assert np.array_equal(ix[name], want_pts[:, a]), name
    assert np.array_equal(ix["s4"][:, :3], want_pts) and np.array_equal(ix["s4"][:, 3].view(np.int32), orig)
    # boxes
    for name, group in (("tbox", 32), ("sbox", 512), ("bbox", 32768)):
        assert ix[name].shape == (-(-n_spad // group), 8), name
        assert np.array_equal(ix[name], boxes_of(ix, group)), name
    # leaves against the restatement
    orig_r, tied, kept = restate(xyz, chunk)
    out = left_out(tied)
    share = float(out.mean())
    got, want = np.sort(orig.reshape(-1, 32), axis=1), np.sort(orig_r.reshape(-1, 32), axis=1)
    bad = np.flatnonzero((got != want).any(axis=1) & ~out)
    print(f"[index] {kind} n={n} chunk={chunk}: {len(out)} leaves, left out for tied medians {share:.4f}, differing {len(bad)}, segments in order before their sort {kept}")
    if kind == "duplicates":
        assert share < DUP_SHARE_MAX
    else:
        assert share == 0.0
    assert len(bad) == 0, (kind, n, bad[:8])
    # the sorts skipped for segments that are in order already must be the identity: today's permutation, tie-break included
    assert np.array_equal(orig, orig_r), (kind, n, int((orig != orig_r).sum()))
