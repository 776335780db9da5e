"""ctypes binding of include/gorio_map.h: MapCloudGenerator::generate on the GPU, fed from a KeyframeStore by id (no numerics here, no
CPU fallback)."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

MAP_SYMBOLS = ["gorio_map_create", "gorio_map_destroy", "gorio_map_generate", "gorio_map_get", "gorio_map_info", "gorio_map_get_counters", "gorio_map_get_capacities",
               "gorio_map_last_error"]


class MapInfo(C.Structure):
    """gorio_map_info_t (include/gorio_map.h)."""
    _fields_ = [("n_listed", C.c_int), ("n_kept", C.c_int), ("n_finite", C.c_int), ("n_voxels", C.c_int), ("anchor", C.c_double * 3), ("min_k", C.c_int * 3), ("max_k", C.c_int * 3)]


def _ptr(a, offset=0):
    return C.c_void_p(a.__array_interface__["data"][0] + offset)


class MapCloud:
    """gorio_map_t: the back end's MapCloudGenerator with the keyframes taken from a KeyframeStore on the same GPU."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.lib.gorio_map_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self._n = 0  # the size of the cloud held: gorio_map_generate reports it
        self._check(self.lib.gorio_map_create(C.byref(self.h), int(device)))

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_map_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def generate_only(self, store, ids, poses, resolution):
        """gorio_map_generate alone: the map stays on the device.  Returns its size."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        if poses.shape[0] != ids.shape[0]:
            raise ValueError("one 4 x 4 pose per keyframe id")
        n = C.c_int(-1)
        self._check(self.lib.gorio_map_generate(self.h, store.h, _ptr(ids) if ids.size else None, _ptr(poses) if poses.size else None, int(ids.shape[0]), C.c_double(resolution),
                                                C.byref(n)))
        self._n = n.value
        return n.value

    def get(self):
        """(xyz [n, 3], intensity [n]) of the last successful generate."""
        n = self._n
        buf = np.zeros((max(n, 1), 4), np.float32)
        self._check(self.lib.gorio_map_get(self.h, _ptr(buf), _ptr(buf, 12), 16, buf.shape[0]))
        return buf[:n, :3].copy(), buf[:n, 3].copy()

    def generate(self, store, ids, poses, resolution):
        """MapCloudGenerator::generate(keyframes, resolution): ids of `store`, poses [count, 4, 4] double.  Returns (xyz [n, 3], intensity [n])."""
        self.generate_only(store, ids, poses, resolution)
        return self.get()

    def info(self):
        i = MapInfo()
        self._check(self.lib.gorio_map_info(self.h, C.byref(i)))
        return dict(n_listed=i.n_listed, n_kept=i.n_kept, n_finite=i.n_finite, n_voxels=i.n_voxels, anchor=[float(v) for v in i.anchor], min_k=list(i.min_k), max_k=list(i.max_k))

    def counters(self):
        g, d, u = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.gorio_map_get_counters(self.h, C.byref(g), C.byref(d), C.byref(u)))
        return dict(generates=g.value, points_downloaded=d.value, bytes_uploaded=u.value)

    def capacities(self):
        c = (C.c_longlong * 6)()
        self._check(self.lib.gorio_map_get_capacities(self.h, c))
        return dict(zip(("frames", "block_counts", "stage", "keys", "result", "record"), c))
