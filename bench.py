#!/usr/bin/env python
"""bench.py - MSCKF(+plane) update-step time and features/s on MI355X (BASELINE.json metric).

A "step" is one full UpdaterMSCKF::update downstream of triangulation (update/UpdaterMSCKF.cpp:411-814) over one synthetic
frame: host -> device copy of the feature batch, the sequential per-plane loop (point-on-plane Jacobians, projection, plane-level
chi2 gate, EKF update per plane), then the point-feature update on the features no accepted plane consumed (Jacobians,
nullspace projection, per-feature chi2 gate, compression, EKF update), results (dx, accept masks, chi2) back on the host.  The
covariance and the pose tables are resident in HBM; every step starts from the same prior (restored device-to-device).

  --gpus 1  (default): BASELINE.json configs[2] - 30 clones, 2000 features of which 1000 lie on 20 planes (10 of them state
             variables, N = 240).  This is the configuration the metric's target is quoted on; configs[1] (2000 point features,
             0 planes) is reported beside it as `point_config`, configs[3] on one GPU as `config4_1gpu`, the headline frame with
             its feature batch uploaded once outside the timed steps as `inputs_resident` (`value` itself carries the H2D).
  --gpus N>1: BASELINE.json configs[3] - 30 clones, 8000 features of which 2500 lie on 50 planes (N = 285), STRONG scaling: the
             plane loop is sequential across planes, so every rank runs it on the whole frame (identical replicas, no
             collective); the free points are sharded over the ranks, ONE RCCL all-reduce sums the information pairs, every
             rank applies the identical update.  `python bench.py --gpus N` starts its N ranks itself (torch.distributed.run).
             `--workload config2 --gpus N` strong-scales the shape without planes (2000 point features split over the ranks) -
             the part of the path that shards; the line carries the RCCL rank count and rank 0's time per stage.

A plain run sets up, settles, warms up, times exactly --steps steps and prints the headline.  Everything else the bench measures
or checks - the second timed window, the per-kernel HIP-event passes and the roofline, the device clock of the two halves of a
step, the side figures (point_config, config4_1gpu, inputs_resident, euroc_like_frame, propagation), the CPU baseline with the
accept-set comparison on the timed frame, and with several ranks the stage pass and the strong-scaling references - runs only
with --full.  --dump-outputs DIR writes what the last timed step handed its caller (rank 0) as DIR/<name>.npy in float64.

Prints ONE JSON line on rank 0."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

_ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _ROOT)

import numpy as np  # noqa: E402

PMC_TRAFFIC_FILE = "r06_final_hbm_traffic_pmc.json"  # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/prof_round.sh, tools/pmc_summary.py); quoted only when its source_hash is the running tree's
F64_PEAK_TFLOPS = 78.6  # MI355X dense FP64 (vector == matrix) peak, AMD datasheet; see DESIGN.md §6, NOTES.md §5
WORKLOADS = {
    "config2": dict(C=30, F=2000, n_planes=0, feats_per_plane=0),
    "config3": dict(C=30, F=2000, n_planes=20, feats_per_plane=50),
    "config4": dict(C=30, F=8000, n_planes=50, feats_per_plane=50),
    "points8000": dict(C=30, F=8000, n_planes=0, feats_per_plane=0),   # config 4 without its planes: the part of the path that shards
}


def algorithmic_flops_per_feature(m: int, calib: bool = True) -> float:
    """reference-algorithm FLOPs of build + projection + gate for one feature with m observations."""
    c = 6 * m + (14 if calib else 0)
    q = 2 * m - 3
    return 400.0 * m + 12.0 * (2 * m) * (c + 1) + 2.0 * q * c * c + 2.0 * q * q * c + q**3 / 3.0 + 2.0 * q * q


def executed_flops_per_feature(m: int) -> float:
    """FLOPs the structured feature kernel issues per feature (NOTES.md §4)."""
    n = 2 * m
    return 450.0 * n + n * (14 * 6 + 14 * 14) * 2.0 + n * m * 2 * (36 + 2 * 34) + (64**3 / 3.0 * 2.0 * (n / 64.0) + 4 * n * 64.0) + 64.0 * 93 * 2


def chol2_flops(n: int, n_inv: int) -> float:
    """FLOPs of one k_chol2 launch of the plane loop: Cholesky of the (n+1)-dimensional bordered T and of the (n_inv+1)-dimensional
    bordered normalised Gram (k^3 / 3 each), back substitution and dx = L0 y (n^2 each, only on accepted planes - not counted)."""
    return (n + 1) ** 3 / 3.0 + (n_inv + 1) ** 3 / 3.0


def pmc_traffic(kernel_substr, name, world):
    """HBM bytes per launch of a kernel from the committed rocprofv3 PMC passes (counters cannot be read from inside this process;
    quoted only for the workload the passes were taken on): 2 x FETCH_SIZE + WRITE_SIZE - the guide's gfx950 correction (wide
    coalesced reads are tallied at half their bytes) applied as the upper bound, WRITE_SIZE as reported.
    The file records the hash of the kernel sources it was taken on (ov_plane_amd/build.py: source_tree_hash); when that is not
    the running tree's the number is NOT quoted: (None, why)."""
    tp = os.path.join(_ROOT, "profiles", PMC_TRAFFIC_FILE)
    if name != "config3" or world != 1:
        return None, "counter passes exist for the config-3 step on one GPU only"
    if not os.path.exists(tp):
        return None, "profiles/%s not found" % PMC_TRAFFIC_FILE
    with open(tp) as fh:
        doc = json.load(fh)
    from ov_plane_amd.build import source_tree_hash

    here, there = source_tree_hash(), doc.get("source_hash")
    if there != here:
        return None, ("profiles/%s was taken on kernel sources %s, the running tree is %s: stale counters are not quoted "
                      "(tools/prof_round.sh retakes them)" % (PMC_TRAFFIC_FILE, there, here))
    hit = [v for k, v in doc["kernels"].items() if kernel_substr in k]
    if not hit or "FETCH_SIZE_KB_avg_per_launch" not in hit[0]:
        return None, "kernel not in profiles/%s" % PMC_TRAFFIC_FILE
    b = (2.0 * hit[0]["FETCH_SIZE_KB_avg_per_launch"] + hit[0].get("WRITE_SIZE_KB_avg_per_launch", 0.0)) * 1024.0
    return b, "2 x FETCH_SIZE + WRITE_SIZE per launch from profiles/%s (separate rocprofv3 --pmc passes over the same step, kernel sources %s)" % (PMC_TRAFFIC_FILE, here)


SQ_COUNTER_FILE = "r06_final_sq_counters_pmc.json"   # rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES ... pass of the same command
KERNEL_STATS_FILE = "r06_final_kernel_stats.csv"      # rocprofv3 --kernel-trace --stats of the same command


def mfma_utilisation(name, world):
    """MFMA busy fraction of the kernels that run on the matrix cores - the covariance GEMMs (k_gemm4, k_plane_dT), the information
    pair's SYRK (k_gram_pair) - from the committed rocprofv3 passes of the config-3 step: SQ_VALU_MFMA_BUSY_CYCLES per launch (cycles,
    summed over the SIMDs that ran the kernel) / (average launch duration x 2.4 GHz x 1024 SIMDs).  Quoted only when both files were
    taken on the running tree's kernel sources (source_hash)."""
    if name != "config3" or world != 1:
        return None
    from ov_plane_amd.build import source_tree_hash

    here = source_tree_hash()
    pc, ks = os.path.join(_ROOT, "profiles", SQ_COUNTER_FILE), os.path.join(_ROOT, "profiles", KERNEL_STATS_FILE)
    if not (os.path.exists(pc) and os.path.exists(ks)):
        return {"note": "profiles/%s or profiles/%s not found" % (SQ_COUNTER_FILE, KERNEL_STATS_FILE)}
    with open(pc) as fh:
        doc = json.load(fh)
    with open(ks) as fh:
        first = fh.readline()
        import csv

        rows = list(csv.reader(fh))
    there = (doc.get("source_hash"), first.split()[2] if first.startswith("# source_hash") else None)
    if there != (here, here):
        return {"note": "committed SQ counters / kernel statistics were taken on kernel sources %s / %s, the running tree is %s: not quoted" % (there[0], there[1], here)}
    dur = {r[0]: float(r[3]) for r in rows[1:] if len(r) > 3}
    out = {}
    for kname, v in doc["kernels"].items():
        busy = v.get("SQ_VALU_MFMA_BUSY_CYCLES_avg_per_launch", 0.0)
        if busy <= 0 or kname not in dur:
            continue
        short = kname.split("(")[0].replace("void ", "").replace("ovp::", "")
        out[short] = {"mfma_busy_cycles_per_launch": busy, "avg_launch_us": dur[kname],
                      "busy_fraction_of_chip": busy / (dur[kname] * 2400.0 * 1024.0)}
    return {"kernels": out, "clock_ghz_assumed": 2.4, "simds": 1024,
            "note": "f64 MFMA busy cycles / (launch duration x clock x SIMDs of the chip), per launch, from profiles/%s and profiles/%s "
                    "(kernel sources %s).  The covariance GEMMs (k_gemm4: W = A L0, T, P+ = V^T V at N <= 240; k_plane_dT) are 20-27 MFLOP "
                    "launches of 5-6 us: latency-bound at this size, the north star's 40 %% needs a GEMM that lasts longer than its own "
                    "launch" % (SQ_COUNTER_FILE, KERNEL_STATS_FILE, here)}


def make_workload(name, seed=0, feat_seed=None, chi2_mult=1.0):
    from ov_plane_amd.synth import make_scene

    w = WORKLOADS[name]
    kw = dict(C=w["C"], F=w["F"], seed=seed, chi2_mult=chi2_mult)
    if feat_seed is not None:
        kw["feat_seed"] = feat_seed
    if w["n_planes"]:
        kw.update(n_planes=w["n_planes"], feats_per_plane=w["feats_per_plane"], planes_in_state_frac=0.5)
    return make_scene(**kw)


def describe(name, sc):
    w = WORKLOADS[name]
    if w["n_planes"]:
        return "%d clones, %d feats of which %d on %d planes (%d of them in the state), calib on (N=%d)" % (
            sc.C, sc.F, int((np.asarray(sc.plane_id) > 0).sum()), int(sc.cp.shape[0]), int((np.asarray(sc.plane_state_id) >= 0).sum()), sc.N)
    return "%d clones, %d MSCKF point feats, 0 planes, calib on (N=%d)" % (sc.C, sc.F, sc.N)


class HipBackend:
    """What bench.py's rank code path needs from the machine: the product backend (one MI355X per rank, RCCL).  The path itself -
    launcher, process group, communicator id exchange, collective settle decision, timed windows, max over ranks, rank-0-only JSON
    line - is written against this object so that tests/test_bench_rank_path_cpu.py can run THE SAME main() on two gloo ranks
    with a stand-in (tests/bench_standin.py, test infrastructure built on the oracle; selected with --standin, never the default,
    and a line produced that way says so in `data` and carries no `value`)."""

    name = "hip"
    dist_backend = "nccl"
    data = "synthetic"

    def __init__(self, torch):
        self.torch = torch
        from ov_plane_amd import capi

        self.capi = capi

    def available(self):
        return self.torch.cuda.is_available()

    def set_device(self, local_rank):
        self.torch.cuda.set_device(local_rank)

    @property
    def device(self):
        return "cuda"

    def synchronize(self):
        self.torch.cuda.synchronize()

    def stream_ctx(self, run):
        return self.torch.cuda.stream(run.stream)

    def make_workload(self, name):
        return make_workload(name)

    def make_runner(self, sc, local_rank):
        return StepRunner(self.capi, self.torch, sc, local_rank)

    # communicator of the C entry ovp_msckf_update_sharded (the library's own RCCL binding)
    def unique_id(self):
        return self.capi.rccl_unique_id()

    def comm_preflight(self, local_rank):
        """Raises when this rank could not enter ncclCommInitRank: binds RCCL (dlopen inside ovp_rccl_unique_id; the id is dropped)
        and touches the device."""
        self.capi.rccl_unique_id()
        self.torch.zeros(1, device="cuda:%d" % local_rank)

    def comm_create(self, uid, rank, world, local_rank):
        return self.capi.rccl_comm_create(uid, rank, world, local_rank)

    def comm_destroy(self, comm):
        self.capi.rccl_comm_destroy(comm)


def load_backend(torch, standin):
    if not standin:
        return HipBackend(torch)
    import importlib

    return importlib.import_module(standin).make_backend(torch, sys.modules[__name__])


def create_native_comm(be, dist, rank, world, local_rank):
    """Communicator for the C entry, created so that a failure on ANY rank cannot leave the others inside ncclCommInitRank: rank 0
    draws the id (or fails) and broadcasts id-or-None - everybody sees the same thing and skips together; the collective
    ncclCommInitRank is entered by all ranks or by none; afterwards a MIN over the ranks decides whether all of them got one.
    Returns (comm or None, reason when None)."""
    torch = be.torch
    uid, why = [None], [None]
    if rank == 0:
        try:
            uid[0] = be.unique_id()
        except Exception as e:  # noqa: BLE001
            why[0] = "ncclGetUniqueId on rank 0: %r" % (e,)
    box = [uid[0], why[0]]
    dist.broadcast_object_list(box, src=0)
    if box[0] is None:
        return None, box[1]
    # everything a rank can fail at BEFORE it would enter the collective ncclCommInitRank (RCCL not loadable, device not usable)
    # is probed and agreed on first: a rank that cannot go in must keep the others out
    comm, err = None, None
    try:
        be.comm_preflight(local_rank)
    except Exception as e:  # noqa: BLE001
        err = "preflight on rank %d: %r" % (rank, e)
    ready = torch.tensor([0 if err else 1], dtype=torch.int32, device=be.device)
    dist.all_reduce(ready, op=dist.ReduceOp.MIN)
    if not bool(ready.item()):
        return None, err or "another rank is not able to create a communicator"
    try:
        comm = be.comm_create(box[0], rank, world, local_rank)
    except Exception as e:  # noqa: BLE001
        err = "ncclCommInitRank on rank %d: %r" % (rank, e)
    ok = torch.tensor([1 if comm else 0], dtype=torch.int32, device=be.device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if bool(ok.item()):
        return comm, None
    if comm:
        try:
            be.comm_destroy(comm)
        except Exception:  # noqa: BLE001
            pass
    return None, err or "another rank could not create its communicator"


class StepRunner:
    """One filter on one GPU: the step of the docstring, for scenes with or without planes."""

    def __init__(self, capi, torch, sc, device, feats_max=None):
        self.capi, self.torch, self.sc = capi, torch, sc
        self.ctx = capi.Context(sc.N, sc.C, feats_max or sc.F, device=device)
        self.stream = torch.cuda.ExternalStream(self.ctx.stream_handle(), device=torch.device("cuda", device))
        self.P0 = torch.from_numpy(np.ascontiguousarray(sc.P)).to("cuda:%d" % device)
        self.opts = capi.opts_from_scene(sc)
        self.opts_pts = capi.opts_from_scene(sc)
        self.has_planes = sc.cp.shape[0] > 0
        self.opts_pts.skip_plane_used = 1 if self.has_planes else 0
        # the frame's C-ABI arguments and output arrays, marshalled once: the timed step is the library's calls, not ctypes struct
        # building and numpy allocations (~70 us per config-3 step through the convenience wrappers of capi.Context)
        self.frame = self.ctx.prepared_frame(sc, self.opts, self.opts_pts)
        self._P0_ptr = self.P0.data_ptr()
        self._lib = capi.lib()

    def step(self):
        """Single GPU: restore of the prior, H2D of the pose tables and of the feature batch, plane loop, point update on the
        rest (device-side mask), results on the host - five C-ABI calls."""
        sc, fr = self.sc, self.frame
        self._lib.ovp_cov_set_device(self.ctx._h, self._P0_ptr, sc.N, sc.N)
        fr.upload()
        if self.has_planes:
            fr.plane_update()
        fr.point_update()
        return self  # (the outputs live in the prepared frame: results())

    def step_resident(self):
        """The same step with the feature batch already resident (uploaded once, outside): restore of the prior and of the pose
        tables, plane loop, point update, results on the host.  Side figure `inputs_resident`, never `value`."""
        sc, fr = self.sc, self.frame
        self._lib.ovp_cov_set_device(self.ctx._h, self._P0_ptr, sc.N, sc.N)
        fr.upload_state()
        if self.has_planes:
            fr.plane_update()
        fr.point_update()
        return self

    def results(self):
        pl, pt = self.frame.results()
        return (pl, self._sharded_pt) if getattr(self, "_sharded_pt", None) is not None else (pl, pt)

    def step_sharded_native(self, comm, rank, world, timing=None):
        """Feature-sharded step through the C-ABI alone: replicated plane loop, then ovp_msckf_update_sharded (this
        rank's index range of the resident frame -> pair -> ncclAllReduce on the context's stream -> update).  torch is not on
        this path (it only started the ranks and carried the communicator id)."""
        import time as _t

        sc, ctx, fr = self.sc, self.ctx, self.frame
        self._lib.ovp_cov_set_device(ctx._h, self._P0_ptr, sc.N, sc.N)
        fr.upload()
        t0 = _t.perf_counter()
        if self.has_planes:
            fr.plane_update()
            if timing is not None:
                timing["plane_loop_ms"] = timing.get("plane_loop_ms", 0.0) + 1e3 * (_t.perf_counter() - t0)
        o = self.opts_pts if self.has_planes else self.opts
        if timing is None:
            pt = ctx.msckf_update_sharded(o, comm, rank, world)
        else:
            # the same stages one by one with a host synchronisation behind each (diagnostic pass)
            from ov_plane_amd.dist import leftover_range, shard_bounds

            if self.has_planes:
                lo, hi, _ = leftover_range(fr.pl_used[: sc.F] != 0, rank, world)
            else:
                lo, hi = shard_bounds(sc.F, rank, world)
            t1 = _t.perf_counter()
            ctx.batch_set_range(lo, hi)
            ctx.build_gate_gram_async(o)
            ctx.sync()
            t2 = _t.perf_counter()
            if comm:
                ctx.rccl_allreduce_gram(comm)
                ctx.sync()
            t3 = _t.perf_counter()
            ctx.ekf_update_from_gram_async()
            pt = ctx.fetch_results()
            ctx.batch_set_range(-1, -1)
            t4 = _t.perf_counter()
            pt["shard"] = (lo, hi)
            for k, v in (("points_build_ms", t2 - t1), ("allreduce_ms", t3 - t2), ("update_ms", t4 - t3)):
                timing[k] = timing.get(k, 0.0) + 1e3 * v
        lo, hi = pt["shard"]
        self.shard_size = int((fr.pl_used[lo:hi] == 0).sum()) if self.has_planes else hi - lo
        self._sharded_pt = pt
        return self  # (results(): the plane outputs live in the prepared frame)

    def step_sharded(self, rank, world, timing=None):
        """The same step through the functions of ov_plane_amd.dist that the gloo tests drive (torch.distributed carries the
        all-reduce): the reference implementation of the split, and the fallback when the native communicator cannot be created."""
        from ov_plane_amd.dist import shard_bounds, sharded_plane_then_point_update, sharded_update

        sc, ctx = self.sc, self.ctx
        ctx.cov_set_device(self.P0.data_ptr(), sc.N, sc.N)
        ctx.state_upload(sc)
        if self.has_planes:
            pl, pt, mine = sharded_plane_then_point_update(
                ctx, self.opts, lambda idx: ctx.batch_upload_scene(sc, idx), sc.F,
                (sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id), rank=rank, world=world, timing=timing)
            self.shard_size = len(mine)
            return pl, pt
        lo, hi = shard_bounds(sc.F, rank, world)
        ctx.batch_upload_scene(sc, np.arange(lo, hi))
        self.shard_size = hi - lo
        return None, sharded_update(ctx, self.opts, timing=timing)

    def close(self):
        self.ctx.close()


PREWARM_MIN_STEPS = 100   # untimed: a fresh box runs its first steps at ramping clocks (3.5 against 3.15 ms per config-3 step)
PREWARM_BLOCK = 25
PREWARM_MAX_S = 6.0       # the untimed settling phase ends when two consecutive blocks agree to 2 % (or after this many seconds)


class GcWatch:
    """Pauses of the Python garbage collector (gc.callbacks): with torch imported the heap holds ~1e6 objects and a generation-2
    collection is a pause of tens of milliseconds in the middle of whichever step triggers it."""

    def __init__(self):
        self.events, self._t0 = [], None

    def __call__(self, phase, info):
        if phase == "start":
            self._t0 = time.perf_counter()
        elif self._t0 is not None:
            self.events.append((int(info.get("generation", -1)), 1e3 * (time.perf_counter() - self._t0)))

    def take(self):
        ev, self.events = self.events, []
        return {"collections": len(ev), "total_ms": round(sum(e[1] for e in ev), 3),
                "longest": [list(map(lambda x: round(x, 3), e)) for e in sorted(ev, key=lambda e: -e[1])[:3]]}


def run_block(fn, steps):
    """`steps` calls of fn; every step ends in a host-visible completion (results read from the pinned block), so the wall time
    of each one is free.  Returns (per-step seconds, last output)."""
    ts, out = [], None
    t_prev = time.perf_counter()
    for _ in range(steps):
        out = fn()
        t = time.perf_counter()
        ts.append(t - t_prev)
        t_prev = t
    return ts, out


def settle(be, fn, dist=None):
    """Untimed steps until the step time has settled: blocks of PREWARM_BLOCK steps until the medians of two consecutive blocks
    agree to 2 %, at least PREWARM_MIN_STEPS, at most PREWARM_MAX_S seconds.  With several ranks the decision to go on is taken
    collectively (every step holds a collective: all ranks must take the same number)."""
    n_done, prev, t0, blocks = 0, None, time.perf_counter(), []
    while True:
        ts, _ = run_block(fn, PREWARM_BLOCK)
        n_done += PREWARM_BLOCK
        med = sorted(ts)[len(ts) // 2]
        blocks.append(1e3 * med)
        settled = prev is not None and abs(med - prev) <= 0.02 * prev and n_done >= PREWARM_MIN_STEPS
        go_on = (not settled) and (time.perf_counter() - t0 < PREWARM_MAX_S)
        if dist is not None:
            flag = be.torch.tensor([1 if go_on else 0], dtype=be.torch.int32, device=be.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            go_on = bool(flag.item())
        if not go_on:
            return n_done, blocks
        prev = med


def time_steps(be, fn, steps, warmup, barrier=None):
    """`warmup` untimed steps, then EXACTLY `steps` timed ones between barrier + synchronize on both sides.
    Returns (elapsed seconds, last output, per-step seconds)."""
    out = None
    for _ in range(warmup):
        out = fn()
    be.synchronize()
    if barrier:
        barrier()
    t0 = time.perf_counter()
    ts, out2 = run_block(fn, steps)
    be.synchronize()
    if barrier:
        barrier()
    return time.perf_counter() - t0, (out2 if steps else out), ts


def step_stats(ts):
    """Distribution of the per-step wall times of a timed window (ms) and the steps that stand out."""
    a = sorted(ts)
    n = len(a)
    med = a[n // 2]
    slow = [[i, round(1e3 * t, 3)] for i, t in enumerate(ts) if t > 1.5 * med]
    return {"median_ms": 1e3 * med, "p90_ms": 1e3 * a[min(n - 1, int(0.9 * n))], "min_ms": 1e3 * a[0], "max_ms": 1e3 * a[-1],
            "mean_ms": 1e3 * sum(ts) / n, "steps_over_1p5x_median": slow,
            "excess_over_median_ms": 1e3 * sum(t - med for t in ts if t > 1.5 * med)}


def dump_outputs(out_dir, pl, pt, P):
    """--dump-outputs: what the last timed step handed its caller - every array of the point update's results (dx, accept mask,
    chi2) as point_<key>, of the plane loop's (per-plane dx, decisions, chi2, rows, consumed-feature mask) as plane_<key>, and the
    covariance it left on the device - as float64 .npy files (under 1 MB for the largest workload), so that two builds can be
    compared output for output (the frame is seeded: same arguments, same inputs)."""
    os.makedirs(out_dir, exist_ok=True)
    arrs = {"covariance": P} if P is not None else {}
    for prefix, res in (("plane", pl), ("point", pt)):
        arrs.update(("%s_%s" % (prefix, k), v) for k, v in (res or {}).items() if isinstance(v, np.ndarray))
    for k, v in arrs.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.asarray(v, dtype=np.float64))


CPU_BASELINE_RUNS = 3  # 3.7 s (one core) + 1.4 s (all cores) per run of the config-3 frame: ~15 s of CPU work in a --full bench


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sc, name, budget_feats=None):
    """The oracle (oracle/ovp_oracle.c: the reference's algorithm in its own loop order, one thread) on the same frame: plane loop
    on every plane, point update on ALL the features the planes did not consume (a bounded prefix only when budget_feats is set).
    Returns the bench object and the oracle's outputs (for the accept-set comparison)."""
    from oracle import pyoracle
    from ov_plane_amd.synth import Scene

    pyoracle.build()
    runs = []
    for _rep in range(CPU_BASELINE_RUNS):  # median of the runs (same inputs, same outputs every time)
        t0 = time.perf_counter()
        pl = None
        if sc.cp.shape[0] > 0:
            pl = pyoracle.msckf_plane_update(sc)
            sc2 = Scene(sc)
            for k in ("P", "clone_q", "clone_p", "calib_q", "calib_p", "intr", "cp"):
                sc2[k] = pl[k]
            rest = np.where(~pl["used"])[0]
            n_used = int(pl["used"].sum())
        else:
            sc2, rest, n_used = sc, np.arange(sc.F), 0
        t1 = time.perf_counter()
        sample = rest if budget_feats is None else rest[:budget_feats]
        pt = pyoracle.msckf_point_update(sc2, feats=sample)
        t2 = time.perf_counter()
        runs.append((t2 - t0, t1 - t0, t2 - t1))
    runs.sort()
    _, t_plane, t_pts = runs[len(runs) // 2]
    # point part scaled to the whole rest only when a prefix was asked for (it is linear in the feature count up to the final update)
    t_full = t_plane + t_pts * (len(rest) / max(len(sample), 1))
    # all-cores ceiling of the same step (BASELINE.md "CPU-omp"): point update spread over the host cores (OpenMP over the features,
    # TSQR compression), plane loop unchanged - it is sequential across planes and its retained rows decide its gate
    omp = None
    try:
        tt = []
        for _rep in range(CPU_BASELINE_RUNS):
            t3 = time.perf_counter()
            po = pyoracle.msckf_point_update_omp(sc2, feats=sample)
            tt.append(time.perf_counter() - t3)
        t3, t4 = 0.0, sorted(tt)[len(tt) // 2]
        omp = dict(runs=len(tt), threads=int(po["threads"]), point_update_ms=1e3 * (t4 - t3), ms_per_step=1e3 * (t_plane + (t4 - t3) * (len(rest) / max(len(sample), 1))),
                   same_accept_set=bool((po["accepted"] == pt["accepted"]).all()),
                   dx_diff_vs_1_thread=float(np.abs(po["dx"] - pt["dx"]).max()),
                   note="oracle/ovp_oracle_omp.c: per-feature stage as an OpenMP loop, compression as a two-level Householder TSQR; "
                        "plane loop on one thread (sequential by definition)")
    except Exception as e:  # noqa: BLE001
        print("all-cores CPU leg skipped: %r" % (e,), file=sys.stderr)
    obj = dict(
        value=sc.F / t_full, unit="features/s", cores=1, kind="port", runs=len(runs), runs_ms=[round(1e3 * r[0], 1) for r in runs],
        timing="median of %d runs" % len(runs), cpu=cpu_model(), host_cores=os.cpu_count(), all_cores=omp,
        sample="oracle/ovp_oracle.c (reference loop order, 1 thread) on the %s frame: plane loop over all planes %.2f s (%d features "
               "consumed, %d planes accepted), point update on %d of the %d remaining features %.2f s (feat system %.2f s, "
               "compression %.2f s, update %.3f s)%s" % (name, t_plane, n_used, int(pl["plane_ok"].sum()) if pl else 0, len(sample),
                                                        len(rest), t_pts, pt["timings"][0], pt["timings"][1], pt["timings"][2],
                                                        "" if len(sample) == len(rest) else "; scaled linearly to the whole frame"),
        ms_per_step=1e3 * t_full)
    return obj, dict(plane=pl, point=pt, rest=rest, sample=sample)


def interbuild_band():
    """Largest distance between two builds of the oracle on the plane-level statistic (tools/plane_gate_agreement.py, committed)."""
    for f in ("r06_plane_gate_agreement.json", "r04_plane_gate_agreement.json", "r03_plane_gate_agreement.json"):
        p = os.path.join(_ROOT, "profiles", f)
        if os.path.exists(p):
            with open(p) as fh:
                return json.load(fh).get("interbuild_band")
    return None


def accept_set_report(run, sc, dev_pl, dev_pt, ora):
    """Device decisions on the timed frame against the oracle's (accept sets compared on the bench frame itself).
    Plane gate: decision per plane, and for every differing plane both statistics and the threshold.  Then the device step is
    repeated with the oracle's plane decisions imposed (ovp_plane_batch::force_decision) so that both sides hand the same state to
    the point update: per-feature accept sets must then be identical, corrections and covariance agree to the path's tolerance."""
    rep = {}
    opl, opt = ora["plane"], ora["point"]
    thr_of = lambda dof: run.opts.chi2_multiplier * run.capi.lib().ovp_chi2_quantile_095(int(dof))  # noqa: E731
    force = None
    if opl is not None and dev_pl is not None:
        ok_d, ok_o = np.asarray(dev_pl["ok"]).astype(bool), np.asarray(opl["plane_ok"]).astype(bool)
        rep["plane_accept_set_equal"] = bool((ok_d == ok_o).all())
        rep["planes_accepted_device"] = int(ok_d.sum())
        rep["planes_accepted_oracle"] = int(ok_o.sum())
        # statistics compared on the common prefix of decisions only (afterwards the two loops see different states)
        diff = []
        first = None
        for k in range(len(ok_o)):
            if ok_d[k] != ok_o[k]:
                first = k if first is None else first
                if k == first:
                    thr = float(thr_of(opl["plane_rows"][k]))
                    diff.append(dict(plane=k, chi2_device=float(dev_pl["chi2"][k]), chi2_oracle=float(opl["plane_chi2"][k]), thr=thr,
                                     oracle_margin=abs(float(opl["plane_chi2"][k]) - thr)))
        rep["first_differing_plane"] = diff
        band = interbuild_band()
        rep["interbuild_band"] = band
        if diff and band is not None:
            rep["difference_inside_interbuild_band"] = bool(diff[0]["oracle_margin"] <= band)
        force = ok_o.astype(np.uint8)
    # same plane decisions on both sides -> identical inputs of the point update
    sc_, ctx = sc, run.ctx
    ctx.cov_set_device(run.P0.data_ptr(), sc_.N, sc_.N)
    ctx.state_upload(sc_)
    ctx.batch_upload_scene(sc_)
    if force is not None:
        ctx.plane_update(run.opts, sc_.plane_id, sc_.cp, sc_.cp_fej, sc_.plane_state_id, force_decision=force)
    pt = ctx.msckf_update(run.opts_pts)
    P = ctx.cov_download()
    sample = ora["sample"]
    acc_d = np.asarray(pt["accepted"]).astype(bool)[sample]
    acc_o = np.asarray(opt["accepted"]).astype(bool)
    rep["point_accept_set_equal_under_oracle_plane_decisions"] = bool((acc_d == acc_o).all()) if len(sample) == len(ora["rest"]) else None
    rep["points_accepted_device"] = int(acc_d.sum())
    rep["points_accepted_oracle"] = int(acc_o.sum())
    if len(sample) == len(ora["rest"]):
        d = np.sqrt(np.abs(np.diag(opt["P"])))
        rep["cov_rel_err_vs_oracle"] = float((np.abs(P - opt["P"]) / np.outer(d, d)).max())
        rep["dx_abs_err_vs_oracle"] = float(np.abs(np.asarray(pt["dx"])[:sc_.N] - opt["dx"]).max())
    rep["accept_set_equal"] = bool(rep.get("plane_accept_set_equal", True) and rep["point_accept_set_equal_under_oracle_plane_decisions"])
    return rep


def reexec_under_torchrun(n):
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execvp(cmd[0], cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", choices=["auto", "config2", "config3", "config4", "points8000"], default="auto")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline (module docstring): second window, kernel-timer passes and "
                         "roofline, device clock, side figures, CPU baseline and accept-set comparison, multi-rank stage pass")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the outputs of the last timed step (rank 0) to DIR/<name>.npy, float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the side figures (point_config, config4_1gpu, propagation)")
    ap.add_argument("--cpu-sample-feats", type=int, default=0, help="0 = the oracle runs every feature of the frame")
    ap.add_argument("--python-gc", choices=["off", "on"], default="off",
                    help="off (default): the Python collector is disabled inside the timed windows (the harness is Python, the path "
                         "under test is a C library: a generation-2 collection of the torch-sized heap is a ~40 ms pause that lands "
                         "in one step); on: left running, its pauses are reported")
    ap.add_argument("--collective", choices=["native", "torch"], default="native",
                    help="multi-GPU step: native = the C entry ovp_msckf_update_sharded on an RCCL communicator of the library's own "
                         "binding (default); torch = ov_plane_amd.dist over torch.distributed (the gloo-tested reference of the split)")
    ap.add_argument("--standin", default="", metavar="MODULE",
                    help="TEST HARNESS ONLY (tests/test_bench_rank_path_cpu.py): run this file's rank code path - launcher, process "
                         "group, communicator id exchange, collective settle decision, max over ranks, rank-0 JSON - on a machine "
                         "without a GPU, with MODULE.make_backend() in place of the HIP backend.  The line then says so in `data` "
                         "and carries value = null: nothing measured that way is a result")
    ap.add_argument("--sharded-path", action="store_true",
                    help="with --gpus 1: take the multi-GPU code path (process group of one rank, dist.sharded_* functions, RCCL "
                         "all-reduce, stage timing) - a smoke test of it on a one-GPU box")
    args = ap.parse_args()

    world_env = int(os.environ.get("WORLD_SIZE", "0"))
    if args.gpus > 1 and world_env == 0:
        reexec_under_torchrun(args.gpus)  # does not return
    import torch

    be = load_backend(torch, args.standin)
    capi = getattr(be, "capi", None)
    world = max(world_env, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not be.available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d" % (args.gpus, world))
    be.set_device(local_rank)
    dist = None
    sharded = world > 1 or args.sharded_path
    real_stdout = None
    if sharded:
        # RCCL writes a version banner to stdout: everything but the JSON line goes to stderr from here on
        sys.stdout.flush()
        real_stdout = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", "29571")
        dist.init_process_group(backend=be.dist_backend, rank=rank, world_size=world)
        assert dist.get_world_size() == args.gpus
    # the product path of a multi-GPU step is the C entry (ovp_msckf_update_sharded) on a communicator created through the library's
    # own RCCL binding; torch.distributed only carries the 128-byte id to the ranks.  --collective torch (or a failure to create the
    # communicator on any rank, agreed on collectively and reported in the line) takes ov_plane_amd.dist instead
    native_comm, collective, comm_note = None, "none", None
    if sharded:
        collective = "torch.distributed"
        if args.collective == "native":
            native_comm, comm_note = create_native_comm(be, dist, rank, world, local_rank)
            if native_comm:
                collective = "rccl-native (ovp_msckf_update_sharded)"
            else:
                print("native RCCL communicator not created (%s): falling back to torch.distributed" % comm_note, file=sys.stderr)
    name = args.workload if args.workload != "auto" else ("config4" if sharded else "config3")
    sc = be.make_workload(name)
    run = be.make_runner(sc, local_rank)
    barrier = (lambda: dist.barrier()) if sharded else None
    with be.stream_ctx(run):
        if sharded:
            sharded_step = (lambda r, timing=None: r.step_sharded_native(native_comm, rank, world, timing)) if native_comm else \
                           (lambda r, timing=None: r.step_sharded(rank, world, timing))
            fn = lambda: sharded_step(run)  # noqa: E731
        else:
            fn = run.step
        import gc

        gcw = GcWatch()
        gc.callbacks.append(gcw)
        n_prewarm, prewarm_blocks = settle(be, fn, dist if sharded else None)
        gc_prewarm = gcw.take()
        if args.python_gc == "off":
            gc.collect()
            gc.disable()
            gcw.take()  # (the collection just asked for)
        run.ctx.host_timing(reset=True)
        elapsed, last, per_step = time_steps(be, fn, args.steps, args.warmup, barrier)
        pl, pt = last.results() if hasattr(last, "results") else last
        host_acc = run.ctx.host_timing(reset=True)
        gc_w1 = gcw.take()
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, pl, pt, run.ctx.cov_download() if hasattr(run.ctx, "cov_download") else None)
        per_step2, gc_w2, k1_n, c2_n, dev_ms, stages = None, None, 0, 0, None, None
        if args.full:
            # a second window of the same length right behind the first (reported beside it, never `value`)
            elapsed2, _, per_step2 = time_steps(be, fn, args.steps, 0, barrier)
            gc_w2 = gcw.take()
        gc.enable()
        gc.callbacks.remove(gcw)
        if args.full:
            # dominant-kernel launch times with HIP events, in a pass of their own (events between dependent launches cost
            # microseconds each, they must not sit in the timed region above)
            run.ctx.kernel_timer(enable=True, reset=True)
            run.ctx.plane_kernel_timer(enable=1, reset=True)
            time_steps(be, fn, max(5, min(args.steps, 20)), 0, barrier)
            k1_ms, k1_n = run.ctx.kernel_timer(enable=False, reset=False)
            c2_ms, c2_n = run.ctx.plane_kernel_timer(enable=0, reset=False)
        # device clock of the two halves of a step (a pass of its own: one event pair around the plane loop, K1 start .. last
        # kernel of the point update) - what the step would take with a host that is never late
        if args.full and not sharded:
            n_ev = max(5, min(args.steps, 20))
            run.ctx.kernel_timer(enable=True, reset=True)
            run.ctx.plane_kernel_timer(enable=2, reset=True)
            run.ctx.host_timing(reset=True)
            pt_ms = []
            for _ in range(n_ev):
                fn()
                pt_ms.append(float(run.ctx.timings_ms()[3]))
            acc = run.ctx.host_timing(reset=True)
            run.ctx.kernel_timer(enable=False, reset=False)
            run.ctx.plane_kernel_timer(enable=0, reset=False)
            dev_ms = {"plane_loop_ms": acc["plane_loop_device_ms"] / n_ev if run.has_planes else 0.0,
                      "point_update_ms": sorted(pt_ms)[len(pt_ms) // 2], "steps": n_ev}
            dev_ms["sum_ms"] = dev_ms["plane_loop_ms"] + dev_ms["point_update_ms"]
        if args.full and sharded:
            # where a multi-GPU step spends its time (a pass of its own: the stages are separated by host synchronisations)
            stages = {}
            n_diag = 5
            for _ in range(n_diag):
                sharded_step(run, stages)
            stages = {k: v / n_diag for k, v in stages.items()}

    # the same workload on ONE GPU, measured by rank 0 of this very job (the others wait): the driver's N = 1 line is the headline
    # configuration (config 3), not this one, so the line carries its own strong-scaling reference
    one_gpu = None
    if args.full and sharded:
        if rank == 0:
            with be.stream_ctx(run):
                els = []
                for blk in range(3):
                    el_b, _, _ = time_steps(be, run.step, 10, 3 if blk == 0 else 0)
                    els.append(el_b / 10)
            one_gpu = {"ms_per_step": 1e3 * sorted(els)[1], "timing": "median of 3 blocks of 10 unsharded steps on rank 0 while the other ranks wait"}
        dist.barrier()
    point_only = None
    if args.full and sharded and name not in ("config2", "points8000"):
        # the part of the path that shards, on the same ranks: config 4's 8000 features WITHOUT its planes, strong-scaled, with its
        # own one-GPU reference (rank 0, unsharded, while the others wait)
        sc2 = be.make_workload("points8000")
        r2 = be.make_runner(sc2, local_rank)
        with be.stream_ctx(r2):
            blocks = []
            for blk in range(5):
                el_b, _, _ = time_steps(be, lambda: sharded_step(r2), 10, 3 if blk == 0 else 0, barrier)
                blocks.append(el_b / 10)
        tb = torch.tensor(blocks, dtype=torch.float64, device=be.device)
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)
        med = float(sorted(tb.tolist())[2])
        ref1 = None
        if rank == 0:
            with be.stream_ctx(r2):
                els = []
                for blk in range(3):
                    el_b, _, _ = time_steps(be, r2.step, 10, 3 if blk == 0 else 0)
                    els.append(el_b / 10)
            ref1 = sorted(els)[1]
        dist.barrier()
        point_only = {"workload": describe("points8000", sc2), "ms_per_step": 1e3 * med, "features_per_s": sc2.F / med,
                      "rank0_point_shard": int(r2.shard_size),
                      "one_gpu_ms_per_step": 1e3 * ref1 if ref1 else None, "speedup_vs_one_gpu": (ref1 / med) if ref1 else None,
                      "timing": "median of 5 blocks of 10 steps, max over ranks per block; one-GPU reference: median of 3 blocks of 10 "
                                "unsharded steps on rank 0"}
        r2.close()
    if sharded:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=be.device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    ms_per_step = 1e3 * elapsed / args.steps
    value = sc.F * args.steps / elapsed

    if rank == 0:
        C = sc.C
        n_pts_done = int(run.shard_size) if sharded else int((~pl["used"]).sum()) if pl is not None else sc.F
        line = {
            "metric": "MSCKF+plane update-step features/sec at %d clones" % C,
            "value": value if be.name == "hip" else None,
            "unit": "features/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "prewarm_steps": n_prewarm,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": be.data,
            "source_hash": __import__("ov_plane_amd.build", fromlist=["source_tree_hash"]).source_tree_hash(),
            "config": {"workload": describe(name, sc), "baseline_config": name, "clones": C, "feats": int(sc.F),
                       "state_dim": int(sc.N), "planes": int(sc.cp.shape[0]),
                       "planes_accepted": int(pl["ok"].sum()) if pl is not None else 0,
                       "points_accepted": int(pt["accepted"].sum()),
                       "parallelism": "1 GPU" if not sharded else "plane loop replicated, free points sharded x%d (RCCL ranks: %d)"
                                      % (world, dist.get_world_size()),
                       "timed_region": "H2D feature batch + plane loop + point update + D2H results; covariance and pose tables "
                                       "resident (restored on the device at the start of every step)"},
        }
        # ---- where the wall time of the timed window went ----
        st1 = step_stats(per_step)
        line["step_times"] = dict(st1, note="wall time of each of the timed steps (every step ends in a host-visible completion); "
                                            "ms_per_step above is total / steps and includes the closing synchronize + barrier")
        if per_step2 is not None:
            line["second_window"] = dict(step_stats(per_step2), ms_per_step=1e3 * elapsed2 / args.steps,
                                         note="the same number of steps timed again right behind the first window")
        line["prewarm"] = {"steps": n_prewarm, "block_medians_ms": [round(b, 4) for b in prewarm_blocks],
                           "rule": "blocks of %d untimed steps until two consecutive block medians agree to 2 %% (>= %d steps, <= %.0f s)"
                                   % (PREWARM_BLOCK, PREWARM_MIN_STEPS, PREWARM_MAX_S)}
        line["python_gc"] = {"inside_timed_windows": args.python_gc, "prewarm": gc_prewarm, "window_1_incl_warmup": gc_w1, "window_2": gc_w2,
                             "note": "pauses of the harness's garbage collector (gc.callbacks); `off` = gc.collect() + gc.disable() in "
                                     "front of the warm-up steps, re-enabled behind the timed window(s); window_2 only with --full"}
        kp, kq = max(host_acc["plane_calls"], 1), max(host_acc["point_calls"], 1)  # (the accumulators also cover the warm-up steps)
        line["host"] = {
            "plane_pre_launch_ms": host_acc["plane_pre_ms"] / kp, "plane_enqueue_ms": host_acc["plane_enqueue_ms"] / kp,
            "plane_wait_ms": host_acc["plane_wait_ms"] / kp, "point_enqueue_ms": host_acc["point_enqueue_ms"] / kq,
            "point_wait_ms": host_acc["point_wait_ms"] / kq, "plane_calls": host_acc["plane_calls"], "point_calls": host_acc["point_calls"],
            "note": "host clock inside the two update entry points per CALL: plane loop entry -> first launch (grouping, staging "
                    "tables), entry -> last launch enqueued, wait for the device; point update enqueue, wait for the published results"}
        if dev_ms is not None:
            line["device_clock"] = dict(dev_ms, step_median_minus_device_ms=st1["median_ms"] - dev_ms["sum_ms"],
                                        note="HIP events in a pass of their own: plane loop (first launch .. covariance product) and "
                                             "point update (feature kernel .. last kernel); the rest of a step is the H2D of the frame, "
                                             "the restore of the prior and the host turn-around")
        # ---- roofline of the dominant kernel ----
        if run.has_planes and c2_n:
            # per plane: the update part factorizes the leading block of the loop's column order (clones + calibration + the own
            # columns of the planes processed so far, NOTES.md section 3b), the range part the plane's involved columns
            base = 6 * C + 14
            in_state = (np.asarray(sc.plane_state_id) >= 0).astype(int)
            nl = base + 3 * np.cumsum(in_state)
            n_inv = base + 3 * in_state
            fl = float(np.mean([chol2_flops(int(a), int(b)) for a, b in zip(nl, n_inv)]))
            n_inv_avg, nl_avg = float(n_inv.mean()), float(nl.mean())
            ks = c2_ms * 1e-3
            line["roofline"] = {
                "bound": "mfma",
                "kernel": "k_chol2 (one launch per plane: bordered tile Cholesky of the leading block of T = I + L0^T A L0 and of the "
                          "normalised Gram side by side on two CUs, gate, back substitution, dx, commit) - a latency-bound serial "
                          "chain, the plane loop is %d of these in sequence" % int(sc.cp.shape[0]),
                "achieved": fl / ks / 1e12, "peak": F64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": fl / ks / 1e12 / F64_PEAK_TFLOPS,
                "traffic": pmc_traffic("k_chol2", name, world)[0], "traffic_note": pmc_traffic("k_chol2", name, world)[1],
                "algorithmic_bytes_per_launch": 8.0 * ((nl_avg + 1) ** 2 / 2 + (n_inv_avg + 1) ** 2 / 2 + sc.N * nl_avg - nl_avg ** 2 / 2),
                "leading_block_avg": nl_avg,
                "avg_launch_ms": c2_ms, "launches_timed": c2_n, "algorithmic_flops_per_launch": fl,
                "share_of_step": c2_ms * int(sc.cp.shape[0]) / ms_per_step,
                "cus_occupied": 2, "frac_of_occupied_cus": fl / ks / 1e12 / (F64_PEAK_TFLOPS * 2.0 / 256.0),
                "note": "f64 MFMA + DPP-broadcast FMA chains on 2 of 256 CUs: the fraction of the chip's peak is by construction "
                        "tiny; what bounds the kernel is the dependent pivot chain (n sequential pivots) and the f64 pipe of one "
                        "CU (NOTES.md section 4)",
            }
        if k1_n:
            m = C
            per_launch = sc.F  # features the launch walks (skipped / other ranks' ones exit early)
            alg = algorithmic_flops_per_feature(m) * n_pts_done
            exe = executed_flops_per_feature(m) * n_pts_done
            ks = max(k1_ms, 1e-9) * 1e-3
            line["roofline_point_kernel"] = {
                "bound": "mfma",
                "kernel": "k_feat_chol (per-feature build + nullspace projection + chi2 gate of the point update; chol(P) rides "
                          "on one CU of the same launch, or runs beside it as k_chol2 on a side stream up to 1976 features)",
                "achieved": exe / ks / 1e12, "peak": F64_PEAK_TFLOPS, "peak_measured": 59.5, "unit": "TFLOP/s",
                "frac": exe / ks / 1e12 / F64_PEAK_TFLOPS, "traffic": pmc_traffic("k_feat_chol", name, world)[0],
                "traffic_source": pmc_traffic("k_feat_chol", name, world)[1],
                "traffic_note": "of which the kernel's OUTPUTS to K2: rec[C][F][2][21] %.1f MB + G[3F][ldg] %.1f MB (zeros for rejected / "
                                "plane-consumed features included); B = H_x P H_x^T + I never leaves the CU since round 5" % (
                                    C * sc.F * 2 * 21 * 8 / 1e6, 3 * sc.F * (((sc.N + 4 + 15) // 16) * 16) * 8 / 1e6),
                "avg_launch_ms": k1_ms, "launches_timed": k1_n,
                "features_gated_per_launch": n_pts_done, "features_walked_per_launch": per_launch,
                "executed_flops_per_launch": exe, "reference_algorithm_flops_per_launch": alg,
                "reference_algorithm_rate": alg / ks / 1e12,
                "note": "frac = executed FLOPs of the Gram-form kernel / launch time / f64 peak; the SURVEY 8(d) reference-"
                        "algorithm figure (5.77 MFLOP per feature, 9x more than executed) is carried separately",
            }
            if "roofline" not in line:
                line["roofline"] = line["roofline_point_kernel"]
        mu = mfma_utilisation(name, world) if args.full else None
        if mu is not None:
            line["mfma_utilisation"] = mu
        if sharded:
            line["multi_gpu"] = {
                "rccl_ranks": int(dist.get_world_size()), "backend": dist.get_backend(), "collective": collective,
                "collective_note": comm_note, "rank0_point_shard": int(run.shard_size)}
        if stages is not None:
            tot_st = sum(stages.values()) or 1.0
            line["multi_gpu"].update({
                "rank0_stage_ms": stages,
                "serial_fraction": stages.get("plane_loop_ms", 0.0) / tot_st,
                "serial_fraction_note": "plane loop (replicated on every rank, sequential across planes: update/UpdaterMSCKF.cpp:413-649) / "
                                        "sum of rank 0's stages; Amdahl bound of the step at this rank count = 1 / (s + (1 - s) / N)",
                "amdahl_bound_speedup": 1.0 / (stages.get("plane_loop_ms", 0.0) / tot_st + (1.0 - stages.get("plane_loop_ms", 0.0) / tot_st) / world),
                "amdahl_bound_speedup_at_8_ranks": 1.0 / (stages.get("plane_loop_ms", 0.0) / tot_st + (1.0 - stages.get("plane_loop_ms", 0.0) / tot_st) / 8.0),
                "one_gpu_same_workload": one_gpu,
                "speedup_vs_one_gpu_same_workload": (one_gpu["ms_per_step"] / ms_per_step) if one_gpu else None,
                "point_only_scaling": point_only,
                "note": "stage times of rank 0 from a separate pass with a host synchronisation behind every stage (plane loop "
                        "replicated on every rank; points_build = feature kernel + information pair of the rank's shard; "
                        "allreduce = one RCCL all-reduce of (N+1) x ld f64; update = EKF update from the summed pair + results)"})
        if args.full and not sharded and not args.no_extras:
            extras(line, be, capi, torch, args, local_rank, name)
        if args.full and not sharded and not args.no_cpu_baseline:
            try:
                line["cpu_baseline"], ora = cpu_baseline(sc, name, args.cpu_sample_feats if args.cpu_sample_feats > 0 else None)
                line["speedup_vs_cpu_baseline"] = line["cpu_baseline"]["ms_per_step"] / ms_per_step
                with be.stream_ctx(run):
                    line["parity_on_timed_frame"] = accept_set_report(run, sc, pl, pt, ora)
            except Exception as e:  # noqa: BLE001
                line.setdefault("cpu_baseline", None)
                print("cpu baseline / accept-set comparison skipped: %r" % (e,), file=sys.stderr)
        out_line = json.dumps(line)
    else:
        out_line = None
    run.close()
    if native_comm:
        be.comm_destroy(native_comm)
    if sharded:
        dist.barrier()
        dist.destroy_process_group()
    if out_line is not None:
        if real_stdout is not None:
            real_stdout.write(out_line + "\n")
            real_stdout.flush()
        else:
            print(out_line)


def extras(line, be, capi, torch, args, device, headline):
    """Side figures, measured after the timed region, never `value`."""
    # the headline frame with its feature batch resident in HBM before the timed region starts (the headline's step carries the H2D of
    # the batch - the boundary hands over host buffers, so `value` is the PCIe-inclusive rate, the stricter of the two)
    try:
        sc = make_workload(headline)
        r = StepRunner(capi, torch, sc, device)
        with torch.cuda.stream(r.stream):
            r.step()  # uploads the batch
            els = []
            for blk in range(5):
                el_b, last, _ = time_steps(be, r.step_resident, 10, 3 if blk == 0 else 0)
                els.append(el_b / 10)
            pl, pt = last.results()
            el = sorted(els)[2]
        line["inputs_resident"] = {"workload": describe(headline, sc), "ms_per_step": 1e3 * el, "features_per_s": sc.F / el,
                                   "timing": "median of 5 blocks of 10 steps (blocks, ms/step: %s)" % ", ".join("%.3f" % (1e3 * e) for e in els),
                                   "planes_accepted": int(pl["ok"].sum()) if pl is not None else 0,
                                   "points_accepted": int(pt["accepted"].sum()),
                                   "note": "feature batch uploaded once outside the timed steps; the prior and the pose tables are restored "
                                           "inside every step as in the headline"}
        r.close()
    except Exception as e:  # noqa: BLE001
        line["inputs_resident"] = None
        print("inputs_resident skipped: %r" % (e,), file=sys.stderr)
    for key, wname in (("point_config", "config2"), ("config4_1gpu", "config4")):
        if wname == headline:
            continue
        try:
            sc = make_workload(wname)
            r = StepRunner(capi, torch, sc, device)
            with torch.cuda.stream(r.stream):
                # median of five blocks of ten steps: one stray host stall (a page fault, a clock ramp) in a block of a side
                # figure would otherwise be its whole value
                els = []
                for blk in range(5):
                    el_b, last, _ = time_steps(be, r.step, 10, 3 if blk == 0 else 0)
                    pl, pt = last.results()
                    els.append(el_b / 10)
                el = 20 * sorted(els)[2]
            line[key] = {"workload": describe(wname, sc), "ms_per_step": 1e3 * el / 20, "features_per_s": sc.F * 20 / el,
                         "timing": "median of 5 blocks of 10 steps (blocks, ms/step: %s)" % ", ".join("%.3f" % (1e3 * e) for e in els),
                         "planes_accepted": int(pl["ok"].sum()) if pl is not None else 0,
                         "points_accepted": int(pt["accepted"].sum())}
            r.close()
        except Exception as e:  # noqa: BLE001  (the headline must not depend on an extra)
            line[key] = None
            print("%s skipped: %r" % (key, e), file=sys.stderr)
    # small-batch latency at the sizes of the real-data configuration (11 + 1 clones, <= 20 features, gate at multiplier 1): the
    # frames of tests/golden/trace_euroc_like.ovptrc (recorded closed loop, stand-in for BASELINE config 5) through the C-ABI -
    # upload of state / covariance / batch, update, results - next to the oracle on the same frames
    try:
        from ov_plane_amd import trace

        frames = trace.read_frames(os.path.join(_ROOT, "tests", "golden", "trace_euroc_like.ovptrc"))
        scs = [trace.scene_from_frame(f) for f in frames]
        ctx = capi.Context(max(s_.N for s_ in scs), max(s_.C for s_ in scs), 32, device=device)

        Pd = [torch.from_numpy(np.ascontiguousarray(s_.P)).to("cuda:%d" % device) for s_ in scs]
        st = torch.cuda.ExternalStream(ctx.stream_handle(), device=torch.device("cuda", device))

        def one(k):
            s_ = scs[k]
            ctx.cov_set_device(Pd[k].data_ptr(), s_.N, s_.N)   # the covariance is resident in a running filter
            ctx.state_upload(s_)
            ctx.batch_upload_scene(s_)
            return ctx.msckf_update(capi.opts_from_scene(s_))

        with torch.cuda.stream(st):
            for k in range(len(scs)):
                one(k)
            torch.cuda.synchronize()
            blocks = []
            for _ in range(9):  # median over nine passes of the trace
                t0 = time.perf_counter()
                for k in range(len(scs)):
                    one(k)
                blocks.append(1e6 * (time.perf_counter() - t0) / len(scs))
            dev_us = sorted(blocks)[4]
        ctx.close()
        from oracle import pyoracle

        pyoracle.build()
        t0 = time.perf_counter()
        for s_ in scs:
            pyoracle.msckf_point_update(s_)
        cpu_us = 1e6 * (time.perf_counter() - t0) / len(scs)
        line["euroc_like_frame"] = {
            "workload": "%d recorded point updates, 12 clones, %d-%d MSCKF features, chi2_multipler 1 (tests/golden/trace_euroc_like.ovptrc)"
                        % (len(scs), min(s_.F for s_ in scs), max(s_.F for s_ in scs)),
            "device_us_per_update": dev_us, "device_us_per_update_passes": [round(b, 1) for b in blocks],
            "oracle_us_per_update_1_core": cpu_us,
            "note": "host call to completion: pose tables and batch uploaded per update, covariance (N = 102) restored on the device; "
                    "at this size the step is launch and transfer latency, not arithmetic"}
    except Exception as e:  # noqa: BLE001
        line["euroc_like_frame"] = None
        print("euroc-like frame timing skipped: %r" % (e,), file=sys.stderr)
    # second figure of SURVEY 8(d): StateHelper::EKFPropagation of the IMU block (k = 15) on the resident covariance
    try:
        sc = make_workload("config2")
        ctx = capi.Context(sc.N, sc.C, 16, device=device)
        rng = np.random.default_rng(1)
        Phi = np.eye(15) + 1e-3 * rng.standard_normal((15, 15))
        Qd = 1e-8 * np.eye(15)
        ctx.cov_upload(sc.P)
        for _ in range(5):
            ctx.cov_propagate(0, [0], [15], Phi, Qd)
        t0 = time.perf_counter()
        for _ in range(50):
            ctx.cov_propagate(0, [0], [15], Phi, Qd)
        line["propagation_cov_step_us"] = 1e6 * (time.perf_counter() - t0) / 50
        ctx.close()
    except Exception as e:  # noqa: BLE001
        line["propagation_cov_step_us"] = None
        print("propagation timing skipped: %r" % (e,), file=sys.stderr)


if __name__ == "__main__":
    main()
