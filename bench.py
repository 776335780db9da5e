#!/usr/bin/env python3
"""bench.py -- throughput of the Go-RIO hot path on MI355X (contract: see the task statement / DESIGN.md "Measurement").

    python bench.py --gpus N --steps K --warmup W            (N > 1: this process only spawns N rank processes, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one pass of the hot path over one batch of synthetic input that is already resident in HBM:
  workload c4 (default; BASELINE.json configs[3]): 64 scan pairs of 16 384 x 16 384 synthetic radar points, each
      setInputTarget + setInputSource (device-to-device) + k-NN covariance estimation + a Gauss-Newton loop of 20 fixed
      iterations (convergence test disabled, as SURVEY 8d prescribes for the throughput configs), plus 64 GP
      pre-integration windows (1 s @ 200 Hz) on a second stream.
  workload c3 (configs[2]): one 16 384-pt scan against a 100 000-pt local map, 20 iterations.
metric = APD-GICP linearisations per second (one unit = one linearize(): correspondence search + Mahalanobis + H/b/error
reduction for one pair at one pose); GP windows/s is reported beside it.  Multi-GPU: every rank owns its own batch (weak
scaling, no data-path collective), value = all units / max-over-ranks time.

A plain run sets up, warms up, times --steps steps, writes the last step's results if --dump-outputs DIR is given, and prints
the JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).  Everything else is behind --full: per-stage
device times, rooflines and the untimed exhaustive-search step, the RCCL co-registration of N > 1, the CPU baseline, and the
post-run CHECK of the timed path's results against the CPU oracle (one pair, one window), which fails the run on a mismatch:
with --full a throughput line is only printed for results that are right.

--dump-outputs DIR writes what the last timed step returned to its caller, rank 0's batch, as DIR/<name>.npy (float32 /
float64): apd_T [pairs, 4, 4], apd_H [pairs, 6, 6], apd_converged, apd_nr_iterations, apd_n_linearize [pairs], and for c4
ugpm_records [windows, 83] (the raw record of gorio_ugpm_preint_batch).  Inputs are seeded: the same arguments give the same
inputs on every run.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# MI355X_MICROARCH.md: 256 CUs x 4 SIMDs, 2.4 GHz; a wave64 fp32 VALU instruction occupies its SIMD for 2 cycles
PEAK_FP32_TFLOPS = 157.3   # = 1024 SIMDs x 2.4e9 / 2 cycles x 64 lanes x 2 flop (an FMA per lane per issue slot)
PEAK_FP64_TFLOPS = 78.6    # vector == v_mfma_f64_16x16x4_f64 rate
PEAK_HBM_GBS = 8000.0
VALU_SLOTS_PER_S = 1024 * 2.4e9 / 2.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c4", choices=["c4", "c3", "c5"],
                    help="c4 (default, the metric's configuration); c3: one 16k scan vs a 100k map; c5: ONE RANK'S SHARE of the 8-GPU configuration -- "
                         "--pairs scans against one shared --map-points map (map index and covariances are setup, not part of a step)")
    ap.add_argument("--map-points", type=int, default=1000000)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--optimizer", default="gn", choices=["gn", "lm"],
                    help="gn (default): the metric's fixed Gauss-Newton iterations, convergence test disabled; lm: the optimiser and tolerances the reference "
                         "ships (Levenberg-Marquardt, trans-eps 0.1, rot-eps 2e-3, <= 64 iterations) -- a secondary line, aligns/s is its natural unit")
    ap.add_argument("--search", default="pruned", choices=["brute", "pruned"], help="correspondence / k-NN search: both are exact and return identical indices")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: per-stage device times and rooflines, the exhaustive-search step, "
                         "the N > 1 co-registration, the CPU baseline and the comparison with the CPU oracle")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0) as DIR/<name>.npy, for comparing two builds output for output")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-check", action="store_true", help="with --full: skip the post-run comparison with the CPU oracle (profiling runs)")
    ap.add_argument("--no-overlap", action="store_true", help="run the GP windows after the scan matching instead of beside it")
    ap.add_argument("--ugpm-four-launch", action="store_true", help="experiment: the rotation fit as four launches per iteration (gorio_ugpm_debug_set_schedule(0))")
    ap.add_argument("--no-exhaustive", action="store_true", help="with --full: skip the extra untimed step that times the exhaustive search kernel")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="nccl (= RCCL) in production; gloo only to rehearse the N > 1 path on one GPU")
    ap.add_argument("--all-ranks-on-device", type=int, default=-1, help="rehearsal only: put every rank on this device instead of LOCAL_RANK")
    ap.add_argument("--cpu-sample-pairs", type=int, default=1)
    ap.add_argument("--coreg-points", type=int, default=262144, help="N > 1 with --full: source points of the sharded-source co-registration that follows the timed batch")
    ap.add_argument("--coreg-map-points", type=int, default=1000000)
    ap.add_argument("--coreg-only", action="store_true", help="N > 1: skip the batch workload and run only the RCCL co-registration (tests)")
    ap.add_argument("--latency", action="store_true",
                    help="instead of the throughput workload: ONE pair at a time through the host-memory entry points the C++ class uses (48-byte PointXYZINormal "
                         "stride, PCIe included), shipped LM tolerances, median over --latency-reps aligns, for 5k x 5k, 16k x 16k and 16k x 100k")
    ap.add_argument("--latency-reps", type=int, default=100)
    return ap.parse_args()


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N rank processes (one per GPU) BEFORE anything here touches the GPU and
    return the worst exit code.  Rank 0 inherits stdout, so the one JSON line comes out of this process' stdout."""
    import torch

    ndev = torch.cuda.device_count()  # may touch the HIP runtime (ROCm builds without amdsmi fall back to hipGetDeviceCount): from here on this
    # process only SPAWNS children and waits for them -- it must never replace itself with another program (exec)
    if args.all_ranks_on_device < 0 and ndev < args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} needs {args.gpus} visible GPUs, found {ndev}; refusing to run fewer ranks and report them as {args.gpus}\n")
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = None
    while procs:
        for p in list(procs):
            code = p.poll()
            if code is None:
                continue
            procs.remove(p)
            if code != 0 and rc == 0:
                rc = code
                deadline = time.time() + 20.0  # a rank died: the others would wait in a collective for ever
        if deadline is not None and time.time() > deadline:
            for p in procs:
                p.kill()
            break
        time.sleep(0.05)
    return rc


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the launcher and the flag must agree\n")
        sys.exit(2)
    import torch

    dist = None
    if args.all_ranks_on_device >= 0:
        local_rank = args.all_ranks_on_device
    if torch.cuda.device_count() <= local_rank:
        sys.stderr.write(f"bench.py: rank {rank} needs GPU {local_rank}, only {torch.cuda.device_count()} visible\n")
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    red_dev = dev if args.dist_backend == "nccl" else torch.device("cpu")  # where the two tiny reduction tensors live
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)

    gorio = importlib.import_module("go-rio_amd")
    if args.ugpm_four_launch:
        importlib.import_module("go-rio_amd.ugpm").ugpm_debug_set_schedule(False)
    synth = gorio.synth
    if args.latency:
        if rank == 0:
            print(json.dumps(latency_mode(args, gorio, local_rank)), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        sys.exit(0)
    if args.coreg_only:
        if dist is None:
            sys.stderr.write("bench.py: --coreg-only needs --gpus N with N > 1\n")
            sys.exit(2)
        out = guarded(lambda: coregistration(args, gorio, dist, torch, rank, world, local_rank, dev, red_dev), torch, local_rank, 300.0)
        if rank == 0:
            print(json.dumps({"metric": "sharded-source co-registration (RCCL all-reduce of the 6x6 normal equations)", "n_gpus": world, "coreg": out}), flush=True)
        if out.get("timed_out"):
            os._exit(3)
        dist.destroy_process_group()
        sys.exit(0 if out.get("ok", False) else 3)
    GN = 0
    n = args.points
    params = dict(corr_dist_threshold=2.0, max_iterations=args.iters, optimizer=GN, rotation_epsilon=0.0, transformation_epsilon=0.0,
                  search=1 if args.search == "pruned" else 0)
    if args.optimizer == "lm":  # launch/ntu_loop3.launch:85-96 + LSQ:13-21
        params.update(max_iterations=64, optimizer=1, rotation_epsilon=2e-3, transformation_epsilon=0.1)

    # ---- synthetic inputs, generated on the host then made resident in HBM (torch is only the allocator here)
    seed0 = synth.BASE_SEED + 3 + 1000 * rank
    pairs = []
    if args.workload == "c4":
        n_pairs, m = args.pairs, n
        for q in range(n_pairs):
            pairs.append(synth.scan_pair(n, m, seed=seed0 + q))
    elif args.workload == "c3":
        n_pairs, m = 1, 100000
        sx, sl = synth.radar_scan(n, seed=seed0)
        tx, tl = synth.local_map(m, seed=seed0 + 1)
        pairs.append((sx, sl, tx, tl, synth.gt_transform()))
    else:  # c5: every rank holds the SAME map (replicated) and its own scans, taken along the path the map was built on
        n_pairs, m = args.pairs, args.map_points
        n_scans = max(6, m // 16384)
        tx, tl = synth.local_map(m, seed=synth.BASE_SEED + 77, n_scans=n_scans)
        for q in range(n_pairs):
            pose = np.eye(4)
            pose[0, 3] = 0.8 * ((q * 7 + 13 * rank) % n_scans)  # a keyframe position of local_map()
            sx, sl = synth.radar_scan(n, seed=seed0 + q, sensor_pose=pose)
            pairs.append((sx, sl, tx, tl, synth.gt_transform() @ pose, pose))  # answer = T_gt pose; the guess is off by T_gt, as in C4
    guesses = np.stack([np.asarray(pr[5] if len(pr) > 5 else np.eye(4), np.float32) for pr in pairs])

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    shared_map = args.workload == "c5"
    resident = []
    for pr in pairs:
        sx, sl, tx, tl = pr[:4]
        resident.append(dict(
            s=[to_dev(sx[:, 0]), to_dev(sx[:, 1]), to_dev(sx[:, 2]), to_dev(sl)],
            t=None if shared_map else [to_dev(tx[:, 0]), to_dev(tx[:, 1]), to_dev(tx[:, 2]), to_dev(tl)], n=sx.shape[0], m=tx.shape[0]))
    torch.cuda.synchronize()
    objs = [gorio.ApdGicp(device=local_rank, **params) for _ in range(n_pairs)]
    objs[0].setProfiling(args.full)  # HIP events per stage on the launch stream: only --full reports them
    map_setup_s = None
    if shared_map:  # ONE upload, index and k-NN of the map per GPU; every other handle references it (gorio_apd_set_target_shared)
        t0 = time.perf_counter()
        objs[0].setInputTarget(pairs[0][2], pairs[0][3])
        objs[0].calculateCovariances()
        for o in objs[1:]:
            o.setInputTargetShared(objs[0])
        torch.cuda.synchronize()
        map_setup_s = time.perf_counter() - t0

    windows = None
    ugpm_batch = None
    if args.workload == "c4":
        windows = [synth.imu_window(seed=seed0 + 500 + q) for q in range(n_pairs)]
        # host-side marshalling of the window structs happens once (it is wrapper work, not the path); every step passes the same
        # HOST arrays through the C ABI, which stages, uploads, computes and downloads inside the timed call
        ugpm_batch = gorio.UgpmBatch(windows, device=local_rank)

    phase = {"set_input": 0.0, "align_batch": 0.0, "ugpm": 0.0}
    ugpm_stage = {}
    ugpm_count = {}
    last = {}
    dev_inputs = gorio.DeviceInputs(objs, sources=[([t.data_ptr() for t in r["s"]], r["n"]) for r in resident],
                                    targets=None if shared_map else [([t.data_ptr() for t in r["t"]], r["m"]) for r in resident])
    UG = ("lpm", "gram", "corr", "lm", "infer", "ata_lm", "ata_corr")

    def set_inputs():
        # setInputTarget / setInputSource of every pair from its HBM-resident buffers (copies them, invalidates covariances and
        # search indices): the batched form of the per-object calls, one copy launch for the 2 x pairs clouds
        t0 = time.perf_counter()
        dev_inputs.apply()
        phase["set_input"] += time.perf_counter() - t0

    def apd_part():
        t1 = time.perf_counter()
        res = gorio.align_batch(objs, guesses)
        phase["align_batch"] += time.perf_counter() - t1
        last["apd"] = res
        return sum(r["n_linearize"] for r in res)

    def ugpm_part():
        if windows is None:
            return 0
        t0 = time.perf_counter()
        last["ugpm"] = ugpm_batch.run()
        phase["ugpm"] += time.perf_counter() - t0
        st, cn = gorio.ugpm_stage_times()  # thread-local: must be read on the thread that ran the batch
        for k, v, c_ in zip(UG, st, cn):
            ugpm_stage[k] = ugpm_stage.get(k, 0.0) + v
            ugpm_count[k] = ugpm_count.get(k, 0) + c_
        return len(windows)

    from concurrent.futures import ThreadPoolExecutor

    pool = ThreadPoolExecutor(max_workers=2)

    def step():
        # the two halves of the hot path are independent: the GP windows run on their own streams from a second host thread
        # (ctypes releases the GIL), so they overlap with the scan matching on the same GPU
        if args.no_overlap:
            set_inputs()
            units = apd_part()
            return units, ugpm_part()
        fu = pool.submit(ugpm_part)
        set_inputs()
        units = apd_part()
        return units, fu.result()

    for _ in range(args.warmup):
        step()
    objs[0].setProfiling(args.full)  # reset the stage clocks: they now cover exactly the timed region
    for k in phase:
        phase[k] = 0.0
    ugpm_stage.clear()
    ugpm_count.clear()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    units = wins = 0
    for _ in range(args.steps):
        u, w = step()
        units += u
        wins += w
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=red_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        cnt = torch.tensor([units, wins], dtype=torch.float64, device=red_dev)
        dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
        units, wins = int(cnt[0].item()), int(cnt[1].item())

    stage_s, stage_n = objs[0].getStageTimes()
    resident_shape = [dict(n=r["n"], m=r["m"]) for r in resident]
    timed_T = [r["T"].copy() for r in last["apd"]]
    timed_rec = None if windows is None else last["ugpm"].copy()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last["apd"], timed_rec)

    # the exhaustive kernel on the same resident data, one untimed step, for the roofline of the north star's brute-force search
    brute = None
    if args.full and args.search == "pruned" and not args.no_exhaustive:
        for o in objs:
            o.set_params(search=0)
        objs[0].setProfiling(True)
        set_inputs()
        gorio.align_batch(objs, guesses)
        bs, bn = objs[0].getStageTimes()
        brute = bs[1] / max(bn[1], 1)
        for o in objs:
            o.set_params(search=1)

    coreg = None
    coreg_hung = False
    if args.full and dist is not None and args.workload == "c4" and args.all_ranks_on_device >= 0 and not os.environ.get("GORIO_BENCH_FORCE_COREG"):
        coreg = {"skipped": "rehearsal with every rank on one device: RCCL cannot place two ranks of a communicator on one GPU", "ok": True}
    elif args.full and dist is not None and args.workload == "c4":
        # BASELINE configs[4] / SURVEY 8(e) row 2: ONE large co-registration, source sharded over the ranks, one ncclAllReduce of the 28
        # normal-equation sums per linearisation -- after (and outside) the timed weak-scaling batch.  Every rank runs it in a CHILD
        # process (`bench.py --coreg-only`, its own rendezvous): a collective that never completes, or a crash inside it, must not take
        # the throughput line with it.
        coreg = coreg_in_children(args, dist, torch, rank, world, local_rank, red_dev)

    rc = 0
    if rank == 0:
        out = report(args, world, n_pairs, n, m, resident_shape, units, wins, dt, stage_s, stage_n, dict(ugpm_stage), dict(ugpm_count), dict(phase), brute)
        if coreg is not None:
            out["coreg"] = coreg
            if not coreg.get("ok", False):
                sys.stderr.write("bench.py: the RCCL co-registration did NOT pass its checks (the throughput line is unaffected): " + json.dumps(coreg) + "\n")
        if map_setup_s is not None:
            out["map_setup_ms"] = 1e3 * map_setup_s  # upload + search index + k-NN covariances of the shared map, once per GPU
        check = None
        oracle_sample = None
        if args.full and not args.no_check:
            check, oracle_sample = check_against_oracle(args, pairs, windows, timed_T, timed_rec)
            out["check"] = check
            if not check["ok"]:
                rc = 3
        if args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(pairs[: args.cpu_sample_pairs], args, windows)
        if rc == 0:
            print(json.dumps(out), flush=True)
        else:
            sys.stderr.write("bench.py: the timed path disagrees with the CPU oracle, no throughput line is printed: " + json.dumps(check) + "\n")
    if coreg_hung:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(rc)  # a collective is stuck on this rank's GPU stream: leave without the teardown that would wait for it
    if dist is not None:
        dist.destroy_process_group()
    sys.exit(rc)


def coreg_in_children(args, dist, torch, rank, world, local_rank, red_dev):
    """Every rank starts `bench.py --gpus N --coreg-only` as a child on its own GPU (fresh rendezvous port agreed through the parent's
    process group), waits for it with a timeout and kills it when it does not finish; rank 0 returns the child's `coreg` record (or why
    there is none).  The parents only spawn and wait: nothing here replaces a running program."""
    port = torch.zeros(1, dtype=torch.int64, device=red_dev)
    if rank == 0:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port[0] = sk.getsockname()[1]
    dist.broadcast(port, src=0)
    env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(int(port.item())),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--coreg-only", "--coreg-points", str(args.coreg_points),
           "--coreg-map-points", str(args.coreg_map_points), "--iters", str(args.iters), "--dist-backend", args.dist_backend]
    if args.all_ranks_on_device >= 0:  # rehearsal of the plumbing only: RCCL itself refuses two ranks on one device
        cmd += ["--all-ranks-on-device", str(args.all_ranks_on_device)]
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, text=True)
    out, err, timed_out = "", "", False
    try:
        out, err = child.communicate(timeout=420.0)
    except subprocess.TimeoutExpired:
        timed_out = True
        child.kill()
        try:
            out, err = child.communicate(timeout=10.0)
        except Exception:  # noqa: BLE001
            pass
    rec = None
    if rank == 0:
        for ln in (out or "").splitlines():
            if ln.startswith("{"):
                try:
                    rec = json.loads(ln).get("coreg")
                except Exception:  # noqa: BLE001
                    rec = None
        if rec is None:
            rec = {"ok": False, "timed_out": timed_out, "exit_code": child.returncode, "error": ((err or "")[-600:] or "the co-registration child printed no record")}
        rec["ran_in"] = "child processes (one per rank), after the timed region"
    dist.barrier()
    return rec


def guarded(fn, torch, local_rank, timeout_s):
    """Run fn on a worker thread and give up after timeout_s: returns fn's dict, or {"ok": False, "timed_out": True} / the exception text."""
    import threading

    box = {}

    def work():
        try:
            torch.cuda.set_device(local_rank)
            box["out"] = fn()
        except Exception as e:  # noqa: BLE001 -- reported in the JSON line
            box["out"] = {"ok": False, "error": f"{type(e).__name__}: {e}"}

    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(timeout_s)
    if th.is_alive():
        return {"ok": False, "timed_out": True, "error": f"no result after {timeout_s:.0f} s"}
    return box["out"]


def dump_outputs(path, apd_results, ugpm_records):
    """--dump-outputs: what the last timed step handed its caller (align_batch's result dicts, UgpmBatch.run()'s record array), one
    .npy per array in float32 / float64.  C4 writes about 60 kB."""
    os.makedirs(path, exist_ok=True)
    arrays = {
        "apd_T": np.stack([r["T"] for r in apd_results]).astype(np.float32),
        "apd_H": np.stack([r["H"] for r in apd_results]).astype(np.float64),
        "apd_converged": np.array([r["converged"] for r in apd_results], np.float64),
        "apd_nr_iterations": np.array([r["nr_iterations"] for r in apd_results], np.float64),
        "apd_n_linearize": np.array([r["n_linearize"] for r in apd_results], np.float64),
    }
    if ugpm_records is not None:
        arrays["ugpm_records"] = np.asarray(ugpm_records, np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


# ------------------------------------------------------------------------------------------- RCCL co-registration (N > 1)

def coregistration(args, gorio, dist, torch, rank, world, local_rank, dev, red_dev):
    """One --coreg-points scan against one --coreg-map-points map, the SOURCE sharded over the ranks behind the C ABI
    (gorio_apd_comm_init): every rank searches and linearises its contiguous share, one in-place ncclAllReduce(28 doubles) per
    linearisation follows on the launch stream, and every rank runs the identical 6x6 solve -- so the poses must agree bit for bit
    without a broadcast.  Rank 0 also runs the same align unsharded.  Returns the evidence (RCCL's own rank count, all-reduce count,
    pose agreement) and the rate."""
    synth = gorio.synth
    n, m = args.coreg_points, args.coreg_map_points
    n_scans = max(6, m // 16384)
    tx, tl = synth.local_map(m, seed=synth.BASE_SEED + 77, n_scans=n_scans)  # the same map on every rank (replicated)
    pose = np.eye(4)
    pose[0, 3] = 0.8 * (n_scans // 2)
    sx, sl = synth.radar_scan(n, seed=synth.BASE_SEED + 99, sensor_pose=pose)
    guess = pose.astype(np.float32)
    uid = torch.zeros(128, dtype=torch.uint8, device=red_dev)
    if rank == 0:
        uid = torch.frombuffer(bytearray(gorio.ApdGicp.commUniqueId()), dtype=torch.uint8).to(red_dev)
    dist.broadcast(uid, src=0)
    uid_bytes = bytes(uid.cpu().numpy().tobytes())
    kw = dict(device=local_rank, corr_dist_threshold=2.0, max_iterations=args.iters, optimizer=0, rotation_epsilon=0.0, transformation_epsilon=0.0, search=1)
    g = gorio.ApdGicp(**kw)
    g.commInit(world, rank, uid_bytes)
    g.setInputTarget(tx, tl)
    g.setInputSource(sx, sl)
    g.align(guess)  # warm-up: search indices and covariances (every rank estimates them for the whole clouds: setup, not the path)
    reps = 3
    dist.barrier()
    torch.cuda.synchronize()
    _, _, c0 = g.commInfo()
    t0 = time.perf_counter()
    lin = 0
    for _ in range(reps):
        r = g.align(guess)
        lin += r["n_linearize"]
    torch.cuda.synchronize()
    dist.barrier()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt], dtype=torch.float64, device=red_dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    w_seen, r_seen, c1 = g.commInfo()
    mine = torch.from_numpy(np.ascontiguousarray(r["T"], np.float32).view(np.uint32).astype(np.int64).reshape(16)).to(red_dev)
    allT = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(allT, mine)
    seen = torch.tensor([w_seen], dtype=torch.int64, device=red_dev)
    dist.all_reduce(seen, op=dist.ReduceOp.MIN)
    g.commDestroy()
    out = {"source_points": n, "map_points": m, "iterations_per_align": args.iters, "aligns_timed": reps, "linearisations_per_s": lin / float(tt.item()),
           "ms_per_align": 1e3 * float(tt.item()) / reps, "allreduce_count": int(c1 - c0), "allreduce_per_linearisation": (c1 - c0) / max(lin, 1),
           "ranks_seen_by_rccl": int(seen.item()), "world": world,
           "pose_identical_on_every_rank": bool(all(torch.equal(a, allT[0]) for a in allT))}
    if rank == 0:
        one = gorio.ApdGicp(**kw)
        one.setInputTarget(tx, tl)
        one.setInputSource(sx, sl)
        ru = one.align(guess)
        out["max_abs_diff_vs_unsharded"] = float(np.abs(ru["T"].astype(np.float64) - r["T"].astype(np.float64)).max())
        t1 = time.perf_counter()
        one.align(guess)
        out["unsharded_ms_per_align"] = 1e3 * (time.perf_counter() - t1)
        out["ok"] = bool(out["pose_identical_on_every_rank"] and out["ranks_seen_by_rccl"] == world and out["allreduce_count"] >= lin and out["max_abs_diff_vs_unsharded"] < 1e-6)
    else:
        out["ok"] = True  # the verdict is rank 0's (every rank's evidence reached it through the collectives above)
    return out


# ------------------------------------------------------------------------------------------------------ single-pair latency

def latency_mode(args, gorio, device):
    """What the odometry nodelet sees (scan_matching_odometry_nodelet.cpp:464-468 times one align; fast_apdgicp/src/align.cpp:51-104 is
    the reference's own harness: clear -> setInputTarget -> setInputSource -> align): ONE pair, clouds handed over as HOST arrays of
    pcl::PointXYZINormal (48-byte stride, so the AoS gather and the PCIe copies are inside the timed call), the optimiser and tolerances the
    launch files ship (Levenberg-Marquardt, trans-eps 0.1, rot-eps 2e-3, <= 64 iterations), nothing reused between aligns.  The oracle's
    time for the same call sequence on the host cores stands beside it."""
    import oracle
    from oracle import apd as oa

    oracle.build()
    synth = gorio.synth
    shapes = [("C1 5000 x 5000", 5000, 5000), ("16384 x 16384", 16384, 16384), ("C3 16384 x 100000 (local map)", 16384, 100000)]
    res = []

    def pcl_points(xyz, lab):
        p = np.zeros((xyz.shape[0], 12), np.float32)
        p[:, :3] = xyz
        p[:, 3] = 1.0
        p[:, 4] = lab
        return p

    for name, n, m in shapes:
        if m <= 20000:
            sx, sl, tx, tl, _ = synth.scan_pair(n, m, seed=synth.BASE_SEED + 11)
        else:
            sx, sl = synth.radar_scan(n, seed=synth.BASE_SEED + 12)
            tx, tl = synth.local_map(m, seed=synth.BASE_SEED + 13)
        ps, pt = pcl_points(sx, sl), pcl_points(tx, tl)
        g = gorio.ApdGicp(device=device, corr_dist_threshold=2.0, max_iterations=64, optimizer=1, rotation_epsilon=2e-3, transformation_epsilon=0.1, search=1)
        t_set, t_align, t_all, lins = [], [], [], []
        for rep in range(args.latency_reps + 3):
            g.clearSource()
            g.clearTarget()
            t0 = time.perf_counter()
            g.setInputTargetPcl(pt)
            g.setInputSourcePcl(ps)
            t1 = time.perf_counter()
            r = g.align()
            t2 = time.perf_counter()
            if rep >= 3:
                t_set.append(t1 - t0)
                t_align.append(t2 - t1)
                t_all.append(t2 - t0)
                lins.append(r["n_linearize"])
        # the same call sequence on the CPU restatement (exact kd-tree search, OpenMP on the granted cores)
        p = oa.launch_params(search=1)
        p.num_threads = usable_cores()
        to = []
        for _ in range(3 if m <= 20000 else 2):
            t0 = time.perf_counter()
            cs, ct = oa.calculate_covariances(sx, p), oa.calculate_covariances(tx, p)
            ro = oa.align(np.eye(4), sx, sl, tx, tl, cs, ct, p)
            to.append(time.perf_counter() - t0)
        d = np.linalg.inv(ro["T"].astype(float)) @ r["T"].astype(float)
        res.append({"shape": name, "median_ms": 1e3 * float(np.median(t_all)), "p90_ms": 1e3 * float(np.percentile(t_all, 90)), "set_inputs_ms": 1e3 * float(np.median(t_set)),
                    "align_ms": 1e3 * float(np.median(t_align)), "linearisations_per_align": float(np.mean(lins)), "converged": bool(r["converged"]),
                    "linearisations_per_s": float(np.mean(lins)) / float(np.median(t_all)),
                    "cpu_oracle_ms": 1e3 * float(np.median(to)), "cpu_cores": usable_cores(), "oracle_linearisations": int(ro["n_linearize"]),
                    "pose_diff_vs_oracle_m": float(np.linalg.norm(d[:3, 3]))})
    return {"metric": "APD-GICP single-pair align latency (host clouds in, pose out)", "unit": "ms", "higher_is_better": False, "n_gpus": 1, "reps": args.latency_reps,
            "data": "synthetic", "dtype": "f32 search / f64 accumulate",
            "config": {"workload": "one pair per call through gorio_apd_set_target / _set_source (48-byte PointXYZINormal stride) + gorio_apd_align; LM, trans-eps 0.1, rot-eps 2e-3; "
                                   "clearTarget / clearSource before every call (nothing reused)"},
            "value": res[1]["median_ms"], "latency": res}


# ------------------------------------------------------------------------------------------------------------- reporting

def source_sha16():
    """sha256 (first 16 hex digits) over the kernel sources the counters in profiles/kernel_counters.json were collected from."""
    import hashlib

    h = hashlib.sha256()
    d = os.path.join(ROOT, "go-rio_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def load_counters():
    """profiles/kernel_counters.json: EXECUTED work per launch of every hot kernel on this workload (rocprofv3 --pmc passes summarised
    by tools/pmc_summary.py: SQ instruction counts, busy cycles, TCC fetch / write bytes; distance evaluations of the pruned search
    from a -DGORIO_STATS build, tools/search_work.py).  The counts are a property of the workload (deterministic kernels on seeded
    inputs), the durations they are divided by are measured live in this run.  The file records the hash of the kernel sources it
    was collected from: when the sources have changed since, the counters are DROPPED (every frac = null) instead of being
    divided by the time of kernels they no longer describe."""
    p = os.path.join(ROOT, "profiles", "kernel_counters.json")
    try:
        doc = json.load(open(p))
    except Exception:
        return {}
    have, want = doc.get("_source_sha16"), source_sha16()
    if have != want:
        sys.stderr.write(f"bench.py: profiles/kernel_counters.json was collected from kernel sources {have}, the tree now holds {want}: "
                         "STALE counters dropped, roofline fractions are null until tools/r03/pmc.sh is re-run\n")
        return {"_stale": True, "kernels": {}}
    return doc


def kernel_entry(counters, kernel, workload):
    """Counters of one kernel, or the sums over the kernels of a stage written as "a + b" (the k-NN stage is two launches)."""
    parts = [k.strip() for k in kernel.split(" + ")]
    es = [counters.get("kernels", {}).get(f"{k}:{workload}") for k in parts]
    if any(e is None for e in es):
        return None
    if len(es) == 1:
        return es[0]
    out = {}
    for key in ("valu_issue_slots", "SQ_INSTS_VALU", "hbm_bytes", "mfma_flops", "fetch_bytes", "write_bytes", "valu_fast_instructions", "valu_slow_instructions"):
        if all(key in e for e in es):
            out[key] = sum(e[key] for e in es)
    return out


def valu_roofline(kernel, entry, avg_s, extra_note=""):
    """Issue-slot roofline of a vector-ALU bound kernel from EXECUTED instructions: the chip has 1024 x 2.4e9 / 2 fp32 issue slots
    per second (an fp32 FMA in every one is the 157.3 TFLOP/s peak); a wave64 instruction of the slow classes (fp64, compares,
    selects, min / max, 64-bit integer) takes two of them.  achieved = slots used per second expressed in the same unit."""
    r = {"bound": "valu", "kernel": kernel, "achieved": None, "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s", "frac": None, "traffic": None,
         "avg_launch_ms": 1e3 * avg_s}
    if entry and avg_s > 0:
        slots = entry.get("valu_issue_slots", entry.get("SQ_INSTS_VALU"))
        if slots:
            r["achieved"] = slots * 128.0 / avg_s / 1e12
            r["frac"] = r["achieved"] / PEAK_FP32_TFLOPS
            r["valu_instructions_per_launch"] = entry.get("SQ_INSTS_VALU")
            r["valu_busy_under_profiler"] = entry.get("valu_busy")
            if entry.get("valu_slow_instructions") is not None and entry.get("SQ_INSTS_VALU"):
                r["slow_instruction_share"] = entry["valu_slow_instructions"] / entry["SQ_INSTS_VALU"]  # half-rate instructions / all VALU instructions
        if entry.get("distance_evaluations"):
            # how EFFICIENT, not just how busy: the distance evaluations the exact search really performs (32 per (query, tile) item;
            # counted by a -DGORIO_STATS build, tools/search_work.py) x 8 flop (3 sub, 3 mul, 2 add) / live time, against the FP32 peak
            r["useful_tflops"] = entry["distance_evaluations"] * 8.0 / avg_s / 1e12
            r["useful_frac"] = r["useful_tflops"] / PEAK_FP32_TFLOPS
            r["distance_evaluations_per_launch"] = entry["distance_evaluations"]
        hb = entry.get("hbm_bytes")
        if hb is not None:
            r["traffic"] = hb
            r["hbm_gbs"] = hb / avg_s / 1e9
            r["hbm_frac"] = hb / avg_s / 1e9 / PEAK_HBM_GBS
    r["note"] = ("vector-ALU issue bound: achieved = EXECUTED wave64 VALU issue slots per launch (SQ instruction counters priced at the measured gfx950 issue rates: fp32 add/mul/fma and "
                 "int32 = 1 slot of 2 cycles, fp64 / compare / select / min / max / 64-bit = 2 slots; profiles/kernel_counters.json) x 64 lanes x 2 flop / live launch time; "
                 "peak = 157.3 TFLOP/s (an fp32 FMA in every slot), so frac is the share of the chip's VALU issue time the kernel fills" + extra_note)
    return r


def report(args, world, n_pairs, n, m, resident, units, wins, dt, stage_s, stage_n, ugpm_stage, ugpm_count, phase, brute):
    wl = args.workload
    out = {
        "metric": "APD-GICP GN iters/sec on 16k-pt scans + GP-preint windows/sec",
        "value": units / dt,
        "unit": "linearisations/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32 search / f64 accumulate",
        "data": "synthetic",
        "config": {
            "workload": {"c4": "C4: 64 scan pairs 16384x16384 + 64 GP windows 1 s @ 200 Hz per GPU, k-NN covariances + 20 fixed GN iterations per pair",
                         "c3": "C3: 16384-pt scan vs 100000-pt local map, 20 fixed GN iterations",
                         "c5": f"C5, one rank's share: {n_pairs} scans of {n} points against ONE shared {m}-point map resident on the GPU "
                               "(source k-NN covariances + 20 fixed GN iterations per scan; map index and covariances are setup)"}[wl],
            "pairs_per_gpu": n_pairs, "source_points": n, "target_points": m, "iterations": args.iters if args.optimizer == "gn" else "until converged (<= 64)",
            "optimizer": "GN (convergence test disabled)" if args.optimizer == "gn" else "LM, shipped tolerances (trans-eps 0.1, rot-eps 2e-3)",
            "search": args.search, "parallelism": f"batch shard x{world} (no collective)"},
        "gp_windows_per_s": (wins / dt) if wins else None,
        "aligns_per_s": n_pairs * world * args.steps / dt,
        "host_phase_seconds": phase,
    }
    if not args.full:
        return out
    counters = load_counters()
    steps = args.steps
    knn_name = "knn_kth_kernel<20> + knn_collect_kernel<20>" if args.search == "pruned" else "knn_partial_kernel<20> + cov_finalize_kernel<20>"
    nn_name = "nn_search_pruned_kernel" if args.search == "pruned" else "nn_search_kernel"
    avg = lambda s, c: s / max(c, 1)  # noqa: E731
    # per-stage device time of the timed region (HIP events on the launch streams), per step
    per_step = {
        "knn_cov": stage_s[0] / steps, "index_build": stage_s[4] / steps, "nn_search": stage_s[1] / steps, "linearize": stage_s[2] / steps, "solve": stage_s[3] / steps,
    }
    for k, v in ugpm_stage.items():
        per_step["ugpm_" + k] = v / steps
    # dominant kernel of the timed region BY TIME
    cand = {
        knn_name: (stage_s[0], stage_n[0]),
        nn_name: (stage_s[1], stage_n[1]),
        "linearize_kernel": (stage_s[2], stage_n[2]),
        "lm_solve_kernel": (stage_s[3], stage_n[3]),
    }
    if ugpm_stage:
        cand["ata_kernel<4, 16, 24>"] = (ugpm_stage.get("ata_lm", 0.0), ugpm_count.get("ata_lm", 0))
        cand["ata_kernel<8, 16, 48>"] = (ugpm_stage.get("ata_corr", 0.0), ugpm_count.get("ata_corr", 0))
    dom = max(cand, key=lambda k: cand[k][0])
    dom_avg = avg(*cand[dom])
    flops_exh = 8.0 * sum(r["n"] * r["m"] for r in resident)  # 8 N M per linearisation, summed over the batch
    if dom.startswith("ata_kernel"):
        roof = mfma_roofline(dom, kernel_entry(counters, dom, wl), dom_avg)
    else:
        roof = valu_roofline(dom, kernel_entry(counters, dom, wl), dom_avg)
    roof["share_of_step_time"] = cand[dom][0] / dt if dt > 0 else None
    kernels = {}
    for k, (s, c) in cand.items():
        if c == 0:
            continue
        e = kernel_entry(counters, k, wl)
        kernels[k] = (mfma_roofline if k.startswith("ata_kernel") else valu_roofline)(k, e, avg(s, c))
        kernels[k].pop("note", None)
        kernels[k]["ms_per_step"] = 1e3 * s / steps
    if counters.get("_stale"):
        roof["note"] = "STALE: profiles/kernel_counters.json was collected from other kernel sources; " + roof.get("note", "")
    out.update({
        "device_ms_per_step": {k: 1e3 * v for k, v in per_step.items()},
        "stage_launches": {"knn_cov": stage_n[0], "index_build": stage_n[4], "nn_search": stage_n[1], "linearize": stage_n[2], "solve": stage_n[3]},
        "roofline": roof,
        "kernels": kernels,
    })
    # what the exact pruning saves against the exhaustive search it replaces: a ratio of algorithmic work rates, NOT a roofline
    if args.search == "pruned" and stage_n[1]:
        nn_avg = avg(stage_s[1], stage_n[1])
        out["pruning_speedup"] = {"algorithmic_tflops_of_exhaustive_search": flops_exh / nn_avg / 1e12,
                                  "vs_exhaustive_kernel": (brute / nn_avg) if brute else None,
                                  "note": "identical correspondences (exact branch and bound); the pruned kernel does not execute the 8 N M flop it is credited with here"}
    if brute:
        b_ach = flops_exh / brute / 1e12
        e = kernel_entry(counters, "nn_search_kernel", wl)
        out["roofline_exhaustive"] = {"bound": "valu", "kernel": "nn_search_kernel", "achieved": b_ach, "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
                                      "frac": b_ach / PEAK_FP32_TFLOPS, "avg_launch_ms": 1e3 * brute, "traffic": (e or {}).get("hbm_bytes"),
                                      "note": "the north star's brute-force search on the same resident batch (one extra untimed step): executed == algorithmic work, 8 flop per point pair"}
    # whole-step HBM traffic against the 8 TB/s roofline (what the north star asks to be reported): sum over the hot kernels
    tot = 0.0
    have = False
    for k, (s, c) in cand.items():
        e = kernel_entry(counters, k, wl)
        if e and e.get("hbm_bytes") is not None:
            tot += e["hbm_bytes"] * c / steps
            have = True
    if have:
        out["hbm"] = {"bytes_per_step": tot, "gbs": tot / (dt / steps) / 1e9, "frac_of_peak": tot / (dt / steps) / 1e9 / PEAK_HBM_GBS,
                      "note": "TCC fetch + write bytes of the hot kernels (profiles/kernel_counters.json) per step / measured step time; the working set is L2 / MALL resident, the path is not HBM bound"}
    return out


def mfma_roofline(kernel, entry, avg_s):
    r = {"bound": "mfma", "kernel": kernel, "achieved": None, "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s", "frac": None, "traffic": None, "avg_launch_ms": 1e3 * avg_s}
    if entry and avg_s > 0:
        fl = entry.get("mfma_flops")
        if fl:
            r["achieved"] = fl / avg_s / 1e12
            r["frac"] = r["mfma_util"] = r["achieved"] / PEAK_FP64_TFLOPS
        hb = entry.get("hbm_bytes")
        if hb is not None:
            r["traffic"] = hb
            r["hbm_gbs"] = hb / avg_s / 1e9
            r["hbm_frac"] = hb / avg_s / 1e9 / PEAK_HBM_GBS
    r["note"] = "fp64 matrix cores: achieved = EXECUTED v_mfma_f64_16x16x4_f64 flop per launch (SQ_INSTS_VALU_MFMA_MOPS_F64; symmetric tiles only) / live launch time; peak 78.6 TFLOP/s"
    return r


def usable_cores():
    """Host cores this process may actually use: the cgroup CPU quota when there is one (the GPU box grants 16 of 256), else
    the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def _pose_err(Ta, Tb):
    d = np.linalg.inv(np.asarray(Ta, float)) @ np.asarray(Tb, float)
    R = d[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.linalg.norm(d[:3, 3])), float(np.arctan2(np.linalg.norm(v), (np.trace(R) - 1.0) / 2.0))


def _oracle_params(oa, args):
    if args.optimizer == "lm":
        return oa.launch_params(search=1)  # the shipped launch values
    return oa.launch_params(max_iterations=args.iters, optimizer=oa.OPT_GN, rotation_epsilon=0.0, transformation_epsilon=0.0, search=1)


def check_against_oracle(args, pairs, windows, timed_T, timed_rec):
    """Results of the LAST TIMED step against the CPU oracle (the checker, never the thing measured): pair 0 -- pose within 1e-4 m /
    1e-4 rad after the same fixed iterations -- and window 0 -- delta_R 1e-4 rad, delta_p 1e-4 m (the gates of BASELINE.json)."""
    import oracle
    from oracle import apd as oa

    oracle.build()
    p = _oracle_params(oa, args)
    p.num_threads = usable_cores()
    sx, sl, tx, tl = pairs[0][:4]
    guess = np.asarray(pairs[0][5], float) if len(pairs[0]) > 5 else np.eye(4)
    cs, ct = oa.calculate_covariances(sx, p), oa.calculate_covariances(tx, p)
    ro = oa.align(guess, sx, sl, tx, tl, cs, ct, p)
    te, re = _pose_err(ro["T"], timed_T[0])
    out = {"pair0_translation_err_m": te, "pair0_rotation_err_rad": re, "pair0_linearisations": ro["n_linearize"]}
    ok = te < 1e-4 and re < 1e-4 and np.all(np.isfinite(np.asarray(timed_T)))
    if windows is not None and timed_rec is not None:
        from oracle import ugpm as ou

        mo = ou.preintegrate(windows[0])[0][0]
        rec = timed_rec[0]
        dR = mo["delta_R"].T @ rec[0:9].reshape(3, 3)
        ang = float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
        pe = float(np.linalg.norm(rec[9:12] - mo["delta_p"]))
        out.update(window0_rotation_err_rad=ang, window0_position_err_m=pe)
        ok = ok and ang < 1e-4 and pe < 1e-4 and bool(np.all(np.isfinite(timed_rec)))
    out["ok"] = bool(ok)
    return out, None


def cpu_baseline(sample_pairs, args, windows=None):
    """The oracle (a port: the reference itself cannot be compiled here) timed on the host cores of this box on a bounded sample of
    the same workload: k-NN covariances + the same fixed-iteration GN loop for `len(sample_pairs)` pairs, through an exact kd-tree
    (what the reference's pcl::search::KdTree path does) with OpenMP over all granted cores; plus a few GP windows single-threaded
    (+1 helper thread) as the reference runs them (preint.h:939, 944)."""
    import oracle
    from oracle import apd as oa

    oracle.build()
    cores = usable_cores()
    p = _oracle_params(oa, args)
    p.num_threads = cores
    shared_ct = oa.calculate_covariances(sample_pairs[0][2], p) if args.workload == "c5" else None  # the shared map: setup, as on the GPU
    t0 = time.perf_counter()
    units = 0
    reps = 0
    while time.perf_counter() - t0 < 8.0:  # repeat the sample until ~8 s of CPU work have been spent
        for pr in sample_pairs:
            sx, sl, tx, tl = pr[:4]
            cs = oa.calculate_covariances(sx, p)
            ct = shared_ct if shared_ct is not None else oa.calculate_covariances(tx, p)
            r = oa.align(np.asarray(pr[5], float) if len(pr) > 5 else np.eye(4), sx, sl, tx, tl, cs, ct, p)
            units += r["n_linearize"]
        reps += 1
    dt = time.perf_counter() - t0
    out = {"value": units / dt, "unit": "linearisations/s", "cores": cores, "kind": "port",
           "sample": f"{len(sample_pairs)} pair(s) of the same workload ({sample_pairs[0][0].shape[0]} x {sample_pairs[0][2].shape[0]} points) x {reps} repetitions: "
                     f"covariances + {'%d GN iterations' % args.iters if args.optimizer == 'gn' else 'an LM align'} each, exact kd-tree search, OpenMP on {cores} threads, {dt:.1f} s"}
    if windows:
        from oracle import ugpm as ou

        t0 = time.perf_counter()
        nwin = 0
        while time.perf_counter() - t0 < 4.0:
            ou.preintegrate(windows[nwin % len(windows)])
            nwin += 1
        dtw = time.perf_counter() - t0
        out["gp_windows_per_s"] = nwin / dtw
        out["gp_sample"] = f"{nwin} windows (1 s @ 200 Hz), 1 solver thread + 1 helper thread as in the reference, {dtw:.1f} s"
    return out


if __name__ == "__main__":
    main()
