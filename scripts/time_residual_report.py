"""Residual report and corner gate (GPU box): python scripts/time_residual_report.py [CFG ...] [--runs 3] [--repeats 20]
Per configuration (default C2 C5), `runs` times over: the report's device time (HIP events around its three kernels, ms_device of
oicc_residual_info) and the whole call on the host clock (it ends in a device synchronise: kernels + read-back + median), against the
only other route to the same numbers -- oicc_evaluate_blocks(kind 0, 1, 2; no Jacobians), a residual dump through three full
evaluation passes, host clock around the three calls (each ends in a synchronise) -- alternating the two inside every run; and one
oicc_gate_corners at 5 sigma_px followed by what it makes the next pass redo: upload + layout + tiles (oicc_get_tangent_layout) and the
set-up of a following solve with the reference's options (the inner-iteration plan), next to the same calls on the ungated problem."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openimucameracalibrator_amd import synthetic, estimator as E

ap = argparse.ArgumentParser()
ap.add_argument("cfgs", nargs="*", default=["C2", "C5"])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--repeats", type=int, default=20)
a = ap.parse_args()
F = E.SPLINE | E.T_I_C | E.GRAVITY_DIR


def wall(fn):
    t = time.perf_counter(); r = fn(); return 1e3 * (time.perf_counter() - t), r


for cfg in a.cfgs:
    ds = synthetic.make_config(cfg)
    cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
    tr = cal.trajectory_
    tr.Optimize(3, F)                                       # a point a user would look at; also lays the problem out for F
    nrows = {0: 2 * cal.num_corners, 1: 3 * int(cal.accl_accepted.sum()), 2: 3 * int(cal.gyro_accepted.sum())}
    dump = lambda: [tr.EvaluateBlocks(F, k, nrows[k], False) for k in (0, 1, 2)]
    for _ in range(3):                                      # warm-up of both routes
        tr.ResidualReport(); dump()
    for run in range(a.runs):
        dev, rep, dmp = [], [], []
        for _ in range(a.repeats):
            ms, info = wall(tr.ResidualReport); rep.append(ms); dev.append(info["ms_device"])
            dmp.append(wall(dump)[0])
        print("%s run %d: report device %.3f ms (min %.3f), report call %.3f ms, three dump passes %.3f ms  [medians of %d; %d corners, %d + %d samples]"
              % (cfg, run, np.median(dev), min(dev), np.median(rep), np.median(dmp), a.repeats, info["num_corners"], info["num_accl"], info["num_gyro"]), flush=True)
    # the gate: the call itself, then what the next pass redoes because the measurements changed
    tr.UseReferenceSolverOptions()
    for run in range(a.runs):
        tr.GateCorners(0.0)
        tr.Optimize(1, F)                                   # everything current, plan included
        base_layout = wall(lambda: tr.GetTangentLayout(F))[0]
        base_setup = 1e3 * tr.Optimize(1, F)["seconds_setup"]
        info = tr.ResidualReport()
        gate_ms, n = wall(lambda: tr.GateCorners(5.0 * info["sigma_px"]))
        if n == 0:                                          # clean synthetic data: gate the worst corner so that the weights do change
            gate_ms, n = wall(lambda: tr.GateCorners(0.999999 * info["max_px"]))
        layout_ms = wall(lambda: tr.GetTangentLayout(F))[0]
        tr.GateCorners(0.0)                                 # (dirty again: the solve's own set-up redoes upload, tiles and plan)
        tr.ResidualReport(); tr.GateCorners(0.999999 * info["max_px"])
        setup_ms = 1e3 * tr.Optimize(1, F)["seconds_setup"]
        print("%s run %d: gate call %.3f ms (%d gated); next layout + tiles %.3f ms (current: %.3f ms); set-up of the next solve with the plan %.3f ms (current: %.3f ms)"
              % (cfg, run, gate_ms, n, layout_ms, base_layout, setup_ms, base_setup), flush=True)
