"""Worker of test_two_processes_on_one_gpu_reduce_through_the_hook: ranks of WORLD_SIZE, ALL on GPU 0, each holding its time shard of
a problem and running oicc_optimize with an all-reduce hook that stages through host memory and gloo (RCCL refuses two ranks on
one device; the hook is the product path under test, the transport is not).  One process hosts the ranks listed in RANKS (default:
RANK), each in a thread of its own with its own problem, stream and gloo group: more ranks than GPU processes the machine allows.
usage: python mp_shard_worker.py <cfg> <flags> <iterations> <bounds_line_search> <out.json> [inner_iterations] [owner_computes]   (RANK(S) / WORLD_SIZE / MASTER_* from the env;
{rank} in <out.json> is replaced by the rank)
owner_computes = 1: the round-4 exchange (oicc_set_shard): halo rows to their owners, gather of the owned band ranges, all-reduce of
the arrow corner only -- through the transport hooks (oicc_set_exchange: gloo send / recv / broadcast staged through host memory).
With inner_iterations = 1 every rank also builds the WHOLE problem on the device and hands it to its shard as the source of the
inner-iteration sweeps (oicc_set_inner_iteration_source): the reference's solver configuration on time-sharded ranks.
OICC_TEST_SEQUENCE: the public calls every rank makes, in this order (default: optimize), comma-separated --
  optimize[:iterations]  time_exchange  time_linear_solve  evaluate  evaluate_cost  evaluate_entries  solver_profile
  set_option:<name>:<value>
evaluate_entries reads the (2, n) int32 array [rows; cols] of OICC_TEST_ENTRIES (.npy).  Each call's results (npz next to <out.json>)
and oicc_debug_dist_solve_info behind it are listed under "steps"; the top-level fields are those of the LAST optimize (its
dist_solves: the distributed solves it ran).  time_exchange is a collective of sharded ranks: skipped on one process.
OICC_TEST_RANK_OPTIONS="<rank>:<name>:<value>;...": options set on that rank only (ranks whose options differ)."""
import ctypes, datetime, json, os, sys, threading, traceback
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openimucameracalibrator_amd import _lib, synthetic, estimator as E


def run_rank(rank, world, cfg, flags, iters, ls, out, inner, owner):
    store = dist.TCPStore(os.environ["MASTER_ADDR"], int(os.environ["MASTER_PORT"]), is_master=False, timeout=datetime.timedelta(seconds=300))
    pg = dist.ProcessGroupGloo(dist.PrefixStore("shards", store), rank, world, datetime.timedelta(seconds=300))
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    calls = {"n": 0, "doubles": 0, "max": 0}

    def allreduce(ptr, count, strm):
        assert hip.hipStreamSynchronize(strm) == 0
        buf = torch.empty(count, dtype=torch.float64)
        assert hip.hipMemcpy(buf.data_ptr(), ptr, count * 8, 2) == 0      # device -> host
        pg.allreduce([buf]).wait()                                          # (SUM)
        assert hip.hipMemcpy(ptr, buf.data_ptr(), count * 8, 1) == 0      # host -> device
        calls["n"] += 1; calls["doubles"] += count; calls["max"] = max(calls["max"], count)

    xch = {"sendrecv": 0, "broadcast": 0, "doubles": 0, "max_broadcast": 0}

    def exchange(op, sp, sc, rp, rc, peer, strm):
        assert hip.hipStreamSynchronize(strm) == 0
        if op == 0:      # send sc doubles to `peer`, receive rc doubles from it: the lower rank of the pair sends first
            sb = torch.empty(max(sc, 1), dtype=torch.float64); rb = torch.empty(max(rc, 1), dtype=torch.float64)
            if sc: assert hip.hipMemcpy(sb.data_ptr(), sp, sc * 8, 2) == 0
            for turn in (0, 1):
                if (turn == 0) == (rank < peer):
                    if sc: pg.send([sb[:sc]], peer, 0).wait()
                elif rc: pg.recv([rb[:rc]], peer, 0).wait()
            if rc: assert hip.hipMemcpy(rp, rb.data_ptr(), rc * 8, 1) == 0
            xch["sendrecv"] += 1; xch["doubles"] += sc + rc
        else:            # `peer` holds sc doubles at sp; everybody receives them in place
            b = torch.empty(sc, dtype=torch.float64)
            if rank == peer: assert hip.hipMemcpy(b.data_ptr(), sp, sc * 8, 2) == 0
            o = dist.BroadcastOptions(); o.rootRank = peer
            pg.broadcast([b], o).wait()
            if rank != peer: assert hip.hipMemcpy(rp, b.data_ptr(), sc * 8, 1) == 0
            xch["broadcast"] += 1; xch["doubles"] += sc if rank != peer else 0; xch["max_broadcast"] = max(xch["max_broadcast"], sc)

    ds = synthetic.make_config(cfg)
    cal = E.ImuCameraCalibrator().BatchInitSpline(ds, shard=(rank, world) if world > 1 else None, owner_computes=bool(owner))
    tr = cal.trajectory_
    tr.SetOption("bounds_line_search", ls); tr.SetOption("inner_iterations", inner)
    if os.environ.get("OICC_TEST_RADIUS") is not None: tr.SetOption("initial_trust_region_radius", float(os.environ["OICC_TEST_RADIUS"]))
    if os.environ.get("OICC_TEST_DISTRIBUTED_SOLVE") is not None: tr.SetOption("distributed_solve", int(os.environ["OICC_TEST_DISTRIBUTED_SOLVE"]))
    shared_launch = os.environ.get("OICC_TEST_SHARED_LAUNCH_SLOTS")     # (tests: the shared blocks of the sweeps as a sequence of launches at any size)
    if shared_launch is not None: tr.SetOption("inner_shared_launch_slots", int(shared_launch))
    for item in filter(None, os.environ.get("OICC_TEST_RANK_OPTIONS", "").split(";")):
        r_, name, value = item.split(":")
        if int(r_) == rank and world > 1: tr.SetOption(name, float(value))
    if world > 1:
        tr.SetAllReduce(allreduce)
        if owner: tr.SetExchange(exchange)
        if inner:
            whole = E.ImuCameraCalibrator().BatchInitSpline(ds)
            # (the plan of the sweeps belongs to the source problem; oicc_optimize forwards the shard's plan options to it: round 6)
            tr.SetInnerIterationSource(whole.trajectory_)
    tr._b.lib.oicc_debug_dist_solve_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]

    def dist_info():
        info = (ctypes.c_int64 * 4)()
        assert tr._b.lib.oicc_debug_dist_solve_info(tr._h, info) == 0
        return [int(v) for v in info]
    steps, s, solves_of_last = [], None, 0
    for k, call in enumerate(os.environ.get("OICC_TEST_SEQUENCE", "optimize").split(",")):
        op, *args = call.split(":")
        before, arrays, step = dist_info(), None, dict(op=call)
        if op == "optimize":
            s = tr.Optimize(int(args[0]) if args else iters, flags)
            step.update(final_cost=s["final_cost"], iterations=len(tr.GetIterations()))
        elif op == "time_exchange":
            if world == 1: step["skipped"] = True
            else: tr.TimeExchange(flags, repeats=1)
        elif op == "time_linear_solve":
            tr.TimeLinearSolve(flags, repeats=1)
        elif op == "evaluate":
            c, H, g = tr.Evaluate(flags)
            arrays = dict(cost=c, H=H, g=g)
        elif op == "evaluate_cost":
            step["cost"] = tr.EvaluateCost(flags)
        elif op == "evaluate_entries":
            rc_ = np.load(os.environ["OICC_TEST_ENTRIES"])
            arrays = dict(values=tr.EvaluateEntries(flags, rc_[0], rc_[1]))
        elif op == "solver_profile":
            fn = tr._b.lib.oicc_debug_solver_profile
            fn.restype = ctypes.c_int; fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_longlong)]
            cycles = (ctypes.c_longlong * 12)()
            step["rc"] = int(fn(tr._h, flags, cycles)); step["cycles"] = [int(v) for v in cycles]
        elif op == "set_option":
            tr.SetOption(args[0], float(args[1]))
        else:
            raise ValueError("unknown call in OICC_TEST_SEQUENCE: " + call)
        step["info"] = dist_info()
        if op == "optimize": solves_of_last = step["info"][0] - before[0]
        if arrays is not None:
            step["file"] = out.format(rank=rank) + ".%d.npz" % k
            np.savez(step["file"], **arrays)
        steps.append(step)
    assert s is not None, "OICC_TEST_SEQUENCE without an optimize"
    it = tr.GetIterations()
    info = dist_info()
    res = dict(rejected=int(s["num_unsuccessful_steps"]), dist_solves=solves_of_last, dist_first_block=int(info[1]), dist_blocks=int(info[2]), dist_ranks=int(info[3]), steps=steps, band_row_doubles=int(s["half_bandwidth"]) + 1 + int(s["arrow_dim"]) + 1, band_dim=int(s["band_dim"]), rank=rank, blocks=cal.num_blocks, iterations=[dict(cost=i["cost"], ok=i["step_is_successful"], gmax=i["gradient_max_norm"]) for i in it],
               final_cost=s["final_cost"], inner_sweeps=s["inner_sweeps"], inner_lm_iterations=s["inner_lm_iterations"], T_i_c=[float(v) for v in tr.GetT_i_c()], hook_calls=calls["n"], hook_doubles=calls["doubles"], hook_max_doubles=calls["max"], P=int(s["num_parameters_tangent"]), exchange=xch)
    json.dump(res, open(out.format(rank=rank), "w"))
    pg.barrier().wait()


def main():
    cfg, flags, iters, ls, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    inner = int(sys.argv[6]) if len(sys.argv) > 6 else 0
    owner = int(sys.argv[7]) if len(sys.argv) > 7 else 0
    world = int(os.environ["WORLD_SIZE"])
    ranks = [int(r) for r in os.environ.get("RANKS", os.environ.get("RANK", "0")).split(",")]
    # the process that hosts rank 0 serves the rendezvous store; it lives until every rank of this process is done
    master = dist.TCPStore(os.environ["MASTER_ADDR"], int(os.environ["MASTER_PORT"]), is_master=True, wait_for_workers=False) if 0 in ranks else None
    _lib.load()     # (bound once, before the rank threads)
    failed = []

    def body(rank):
        try:
            run_rank(rank, world, cfg, flags, iters, ls, out, inner, owner)
        except BaseException:
            traceback.print_exc(); failed.append(rank)
    threads = [threading.Thread(target=body, args=(r,)) for r in ranks]
    for t in threads: t.start()
    for t in threads: t.join()
    del master
    if failed:
        raise SystemExit("ranks %s failed" % failed)


if __name__ == "__main__":
    main()
