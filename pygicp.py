"""`import pygicp` from a checkout, as the reference's src/kitti.py writes it: re-exports go-rio_amd/pygicp.py (the directory name has a
hyphen, hence importlib)."""
import importlib as _importlib

_m = _importlib.import_module("go-rio_amd.pygicp")
from_names = list(_m.__all__) + ["__version__"]
globals().update({k: getattr(_m, k) for k in from_names})
__all__ = list(_m.__all__)
del _importlib, from_names
