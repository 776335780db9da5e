"""NumPy restatement of the radius neighbourhood of NDT (include/gorio_ndt.h, gorio_ndt_set_radius_search): what
pcl::NormalDistributionsTransform and pclomp's KDTREE compute (NDT:234-235, 573-574, 948-949; VGC:282-326).

Only what the mode changes is written here: the centroid cloud and the neighbourhoods.  The pair arithmetic, the score, the Newton /
More-Thuente shell and the voxel map are the functions of tests/ndt_restatement.py itself, re-bound so that the name `neighbourhood`
they look up resolves to the radius search below (same code objects, other globals): nothing of that file is copied or edited.

  * centroid cloud: one point per leaf with nr_points >= min_points_per_voxel, ascending leaf index; a leaf the reference disables
    afterwards (VGC:337-341, 360-364) stays, with the zero icov build_voxel_map leaves it;
  * centroid coordinates: the running float32 sum of the leaf's points in input order (VGC:242-243) / float32(nr_points) (VGC:289);
  * search: search_restatement.radius over the float centroids, radius = float32(resolution), max_nn = 0: ascending
    (distance, centroid index), which is the order a point's pair terms are added in; no cell-range test.
"""
import types

import numpy as np

import ndt_restatement as R
import search_restatement as SR

f32 = np.float32
RADIUS = "radius"  # the `search` value the re-bound functions carry through to neighbourhood()


def build_voxel_map(target, resolution, min_points=6, eig_mult=0.01):
    """R.build_voxel_map plus the centroid cloud: vm.cent float32 [C, 3], vm.cent_leaf int64 [C] (positions in the leaf order)."""
    vm = R.build_voxel_map(target, resolution, min_points, eig_mult)
    vm.cent, vm.cent_leaf = np.zeros((0, 3), f32), np.zeros(0, np.int64)
    if vm.n_leaves == 0:
        return vm
    T = np.asarray(target, f32).reshape(-1, 3)
    P = T[np.isfinite(T).all(axis=1)]
    lin = (np.floor(P * vm.inv) - vm.min_b.astype(f32)).astype(np.int64) @ vm.mul  # VGC:218-223, as build_voxel_map has it
    order = np.argsort(lin, kind="stable")
    idx, starts, counts = np.unique(lin[order], return_index=True, return_counts=True)
    assert np.array_equal(idx, vm.idx)
    Pf = P[order]
    S = np.zeros((idx.shape[0], 3), f32)
    for k in range(int(counts.max())):  # centroid.head<3>() += pt, float, in input order (VGC:242-243)
        m = counts > k
        S[m] = S[m] + Pf[starts[m] + k]
    cent = S / counts.astype(f32)[:, None]  # VGC:289: /= (float) nr_points, a true division per element
    in_cloud = counts >= vm.min_points      # VGC:297; the `continue` of VGC:337-341 comes after the push_back
    vm.cent, vm.cent_leaf = cent[in_cloud], np.nonzero(in_cloud)[0].astype(np.int64)
    return vm


def neighbour_csr(vm, q):
    """target_cells_.radiusSearch(q, resolution_) for float32 points q: CSR (offsets, leaf positions, squared distances)."""
    offs, idx, sqd = SR.radius(vm.cent, np.asarray(q, f32).reshape(-1, 3), float(vm.leaf), 0)
    return offs, vm.cent_leaf[idx].astype(np.int32), sqd


def neighbourhood(vm, q, search):
    """The shape R.neighbourhood returns -- a list of per-point leaf positions (-1: none) -- with entry k the k-th neighbour of every
    point in (distance, centroid index) order, so that the callers add a point's pair terms in that order."""
    assert search == RADIUS
    offs, leaf, _ = neighbour_csr(vm, q)
    cnt = np.diff(offs)
    out = []
    for k in range(int(cnt.max()) if cnt.size else 0):
        pos = np.full(cnt.shape[0], -1, np.int64)
        m = cnt > k
        pos[m] = leaf[offs[:-1][m] + k]
        out.append(pos)
    return out


_GLOBALS = dict(vars(R))
_GLOBALS["neighbourhood"] = neighbourhood


def _rebound(fn):
    g = types.FunctionType(fn.__code__, _GLOBALS, fn.__name__, fn.__defaults__, fn.__closure__)
    g.__kwdefaults__ = fn.__kwdefaults__
    return g


derivatives = _GLOBALS["derivatives"] = _rebound(R.derivatives)
hessian_only = _GLOBALS["hessian_only"] = _rebound(R.hessian_only)
calculate_score = _GLOBALS["calculate_score"] = _rebound(R.calculate_score)


class Ndt(R.Ndt):
    """R.Ndt with the radius neighbourhood: its methods are R.Ndt's code over the functions above."""

    def __init__(self, **params):
        assert "search" not in params
        super().__init__(search=RADIUS, **params)

    def set_target(self, target):
        self.vm = build_voxel_map(target, self.resolution, self.min_points, self.eig_mult)


for _name in ("derivatives", "_step_length", "align"):
    setattr(Ndt, _name, _rebound(getattr(R.Ndt, _name)))
