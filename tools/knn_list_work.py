"""List work of the K = 20 selection kernels (knn_kth_kernel, knn_collect_kernel) per wave, on clouds of the C4 benchmark, from a library
built with -DGORIO_STATS and given through GORIO_AMD_LIB:

    make -C go-rio_amd/csrc OUT=../../tools/variants/stats.so EXTRA=-DGORIO_STATS
    GORIO_AMD_LIB=tools/variants/stats.so python tools/knn_list_work.py [pairs]

The C4 batch runs 64 queries per wave; a call on one pair would run 32 (run_covariances), so GORIO_KNN_QPW pins 64 here.  The waves never
cooperate, so the counts per wave are those of the batch."""
import ctypes as C
import importlib
import os
import sys

os.environ.setdefault("GORIO_KNN_QPW", "64")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
gorio = importlib.import_module("go-rio_amd")
synth = gorio.synth
lib = gorio.load_library()
pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
out = (C.c_ulonglong * 24)()
objs = []
for q in range(pairs):
    sx, sl, tx, tl, _ = synth.scan_pair(16384, 16384, seed=synth.BASE_SEED + 3 + q)
    o = gorio.ApdGicp(corr_dist_threshold=2.0, search=1)
    o.setInputTarget(tx, tl)
    o.setInputSource(sx, sl)
    objs.append(o)
lib.gorio_debug_search_stats(out, 1)
for o in objs:
    o.calculateCovariances()
lib.gorio_debug_search_stats(out, 1)
v = [int(x) for x in out]
kw, cw = max(v[4], 1), max(v[0], 1)
print("knn_kth_kernel waves", v[4], "executed insertions per wave %.1f" % (v[5] / kw))
for name, k in (("D[4]", 6), ("D[9]", 7), ("D[14]", 8)):
    print("  no lane below %-5s %.1f per wave = %.1f %% of the insertions" % (name, v[k] / kw, 100.0 * v[k] / max(v[5], 1)))
print("knn_collect_kernel waves", v[0], "tiles per wave %.1f" % (v[1] / cw), "flagged waves", v[10])
print("  longest column (rounds) per wave %.2f" % (v[9] / max(cw - v[10], 1)), "waves at 20..24:", v[12:17])
