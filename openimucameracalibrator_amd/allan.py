"""IMU noise characterisation: host-side mirror of the reference's applications/fit_allan_variance.cc and
core::AllanVarianceFitter (src/core/allan_variance_fitter.cc:12-128) over the C-ABI entries oicc_allan_*.
The Allan variance of all six channels runs on the MI355X in one call; the factor list and the noise-model fit run on
the host inside the library.  There is no CPU fallback."""
import argparse
import ctypes as C
import json

import numpy as np

from . import _lib
from . import io_files

GYRO, ACC = 0, 1
GYRO_SCALE = 57.3 * 3600          # AllanGyr::pushRadPerSec (allan_gyr.cc:20-23): rad/s -> deg/h
AXES = ("acc_x", "acc_y", "acc_z", "gyr_x", "gyr_y", "gyr_z")

_i32p = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def allan_factors(n, num_clusters=10000, backend=None):
    """AllanGyr::initStrides: the cluster sizes (in samples) for n samples."""
    b = backend if backend is not None else _lib.load_allan()
    out = np.zeros(num_clusters, dtype=np.int32)
    nf = C.c_int32()
    rc = b.factors(int(n), int(num_clusters), _p(out, _i32p), C.byref(nf))
    if rc != 0:
        raise ValueError("oicc_allan_factors failed with status %d" % rc)
    return out[:nf.value].copy()


def allan_variance(samples, t_s, scale, num_clusters=10000, device=0, backend=None):
    """Overlapping Allan variance of every row of samples [channels][n] (raw units; scale[c] is applied per sample).
    Returns dict(factors, taus, sigma2 [channels][num_factors], freq, period, mean [channels], device_ms)."""
    b = backend if backend is not None else _lib.load_allan()
    w = np.ascontiguousarray(np.atleast_2d(np.asarray(samples, dtype=np.float64)))
    t = np.ascontiguousarray(np.asarray(t_s, dtype=np.float64).ravel())
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (w.shape[0],)))
    ch, n = w.shape
    if t.shape[0] != n:
        raise ValueError("times and samples differ in length")
    factors = np.zeros(num_clusters, dtype=np.int32)
    taus = np.zeros(num_clusters)
    s2 = np.zeros(ch * num_clusters)
    mean = np.zeros(ch)
    nf, freq, period, ms = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
    rc = b.variance(int(device), ch, n, _p(w), _p(t), _p(sc), int(num_clusters), C.byref(nf), _p(factors, _i32p), _p(taus), _p(s2),
                    C.byref(freq), C.byref(period), _p(mean), C.byref(ms))
    if rc != 0:
        raise RuntimeError("oicc_allan_variance failed with status %d" % rc)
    k = nf.value
    return dict(factors=factors[:k].copy(), taus=taus[:k].copy(), sigma2=s2[:ch * k].reshape(ch, k).copy(),
                freq=freq.value, period=period.value, mean=mean, device_ms=ms.value)


def allan_fit(kind, taus, sigma2, freq, backend=None):
    """FitAllanGyr (kind GYRO) / FitAllanAcc (kind ACC) on one axis; sigma2 in the units the variance was computed in."""
    b = backend if backend is not None else _lib.load_allan()
    t = np.ascontiguousarray(np.asarray(taus, dtype=np.float64))
    s = np.ascontiguousarray(np.asarray(sigma2, dtype=np.float64))
    params, init, rep = np.zeros(5), np.zeros(5), np.zeros(6)
    used, iters = C.c_int32(), C.c_int32()
    rc = b.fit(int(kind), len(t), _p(t), _p(s), float(freq), _p(params), _p(init), _p(rep), C.byref(used), C.byref(iters))
    if rc != 0:
        raise RuntimeError("oicc_allan_fit failed with status %d" % rc)
    return dict(params=params, init=init, bias_instability=rep[0], tau_at_min=rep[1], white_noise=rep[2],
                bias_instability_B=rep[3], white_noise_N=rep[4], cost=rep[5], num_used=used.value, iterations=iters.value)


class AllanVarianceFitter:
    """core::AllanVarianceFitter(telemetry, nr_clusters).RunFit().  telemetry: dict with timestamps_ns[n],
    accelerometer[n][3] (m/s^2), gyroscope[n][3] (rad/s), as the telemetry JSON holds them."""

    def __init__(self, telemetry, nr_clusters=10000, device=0, backend=None):
        self.nr_clusters = int(nr_clusters)
        self.device = device
        self.backend = backend
        self.t_s = np.asarray(telemetry["timestamps_ns"], dtype=np.float64).ravel() * 1e-9   # read_telemetry.cc: timestamp_s
        acc = np.asarray(telemetry["accelerometer"], dtype=np.float64).reshape(-1, 3)
        gyr = np.asarray(telemetry["gyroscope"], dtype=np.float64).reshape(-1, 3)
        self.samples = np.concatenate([acc.T, gyr.T], axis=0)       # AXES order
        self.scale = np.array([1.0, 1.0, 1.0, GYRO_SCALE, GYRO_SCALE, GYRO_SCALE])

    def RunFit(self):
        v = allan_variance(self.samples, self.t_s, self.scale, self.nr_clusters, device=self.device, backend=self.backend)
        res = dict(n=int(self.samples.shape[1]), freq=v["freq"], period=v["period"], factors=v["factors"], taus=v["taus"],
                   device_ms=v["device_ms"], axes={})
        for c, name in enumerate(AXES):
            kind = GYRO if name.startswith("gyr") else ACC
            s2 = v["sigma2"][c]
            fit = allan_fit(kind, v["taus"], s2, v["freq"], backend=self.backend)
            ax = dict(sigma2=s2, deviation=np.sqrt(s2), fit=fit, mean=v["mean"][c])
            if kind == GYRO:
                ax["bias"] = v["mean"][c] / 3600          # allan_variance_fitter.cc: getAvgValue() / 3600, degree/s
            res["axes"][name] = ax
        return res


def result_lines(res):
    """The reference's result lines (allan_variance_fitter.cc:56-125, fitallan_gyr.cc:49-60, fitallan_acc.cc:52-56)."""
    out = []
    for name, title in (("gyr_x", "Gyro X "), ("gyr_y", "Gyro y "), ("gyr_z", "Gyro z "), ("acc_x", "acc X "), ("acc_y", "acc y "), ("acc_z", "acc z ")):
        a = res["axes"][name]; f = a["fit"]
        out.append(title)
        out.append("C " + " ".join("%.6g" % x for x in f["init"]))
        if name.startswith("gyr"):
            out.append(" Bias Instability %.6g rad/s" % f["bias_instability_B"])
            out.append(" Bias Instability %.6g rad/s, at %.6g s" % (f["bias_instability"], f["tau_at_min"]))
            out.append(" White Noise %.6g rad/s" % f["white_noise_N"])
            out.append(" White Noise %.6g rad/s" % f["white_noise"])
            out.append("  bias %.6g degree/s" % a["bias"])
        else:
            out.append(" Bias Instability %.6g m/s^2" % f["bias_instability"])
            out.append(" White Noise %.6g m/s^2" % f["white_noise"])
        out.append("-------------------")
    return out


def result_json(res):
    """The --result_output_json document (the C++ application writes the same keys)."""
    doc = dict(num_samples=res["n"], freq=res["freq"], period=res["period"], num_factors=int(len(res["factors"])), axes={})
    for name, a in res["axes"].items():
        f = a["fit"]
        d = dict(Q=f["params"][0], N=f["params"][1], B=f["params"][2], K=f["params"][3], R=f["params"][4],
                 bias_instability=f["bias_instability"], tau_at_min=f["tau_at_min"], white_noise=f["white_noise"],
                 bias_instability_B=f["bias_instability_B"], white_noise_N=f["white_noise_N"], num_used=f["num_used"],
                 iterations=f["iterations"], final_cost=f["cost"])
        if "bias" in a:
            d["bias"] = a["bias"]
        doc["axes"][name] = {k: (float(v) if not isinstance(v, int) else v) for k, v in d.items()}
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description="IMU noise parameters from a still recording (fit_allan_variance)")
    ap.add_argument("--telemetry_json", default="", help="Path to the telemetry json.")
    ap.add_argument("--verbose", action="store_true", help="If more stuff should be printed")
    ap.add_argument("--result_output_json", default="", help="write the fitted values here")
    ap.add_argument("--nr_clusters", default=10000, type=int)
    ap.add_argument("--device", default=0, type=int)
    args = io_files.parse_reference_flags(ap, argv)
    with open(args.telemetry_json) as f:
        tel = json.load(f)
    res = AllanVarianceFitter(tel, args.nr_clusters, device=args.device).RunFit()
    for line in result_lines(res):
        print(line)
    if args.result_output_json:
        with open(args.result_output_json, "w") as f:
            json.dump(result_json(res), f, indent=2)


if __name__ == "__main__":
    main()
