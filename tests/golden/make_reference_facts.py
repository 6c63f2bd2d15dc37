"""Regenerates the fixtures that let the tests compare this repository with the reference WITHOUT the reference tree:

  reference_facts.json   names the reference's interface and file formats use (gflags of the four applications, flags its
                         python/run_*.py drivers pass, public methods of the mirrored classes, JSON keys of the io layer) and
                         outputs of its python/ modules (sew.py on 60 seeded signals, get_sew_for_dataset.py on the C1 telemetry)
  ref_json_cases.json    the reference's JSON library (oracle/_ref/ref_json_tool, `make -C oracle ref REF=<tree>`) on the
                         documents of test_ref_json_fixture.py: to_ubjson of 150 property-test documents, from_ubjson of this
                         repository's encoder output

usage: python tests/golden/make_reference_facts.py <reference tree>
The reference is run only here (its Python modules in a child interpreter that writes no bytecode into its tree); the tests read
only the committed files."""
import glob
import hashlib
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
APPS = ("continuous_time_imu_to_camera_calibration", "estimate_imu_to_camera_rotation", "calibrate_camera",
        "estimate_camera_poses_from_checkerboard")


def telemetry_digest(tel):
    return hashlib.sha256(json.dumps(tel, sort_keys=True).encode()).hexdigest()


def sew_case_c1(tmp):
    """The telemetry file of test_sew.test_twin_application_writes_what_the_reference_script_writes."""
    from openimucameracalibrator_amd import synthetic, io_files
    ds = synthetic.make_config("C1", camera="gopro9_division")
    files = io_files.write_dataset_files(ds, tmp)
    tel = json.load(open(files["telemetry_json"]))
    tel["camera_fps"] = 59.94                                   # read_generic_json requires the key (telemetry_converter.py:237)
    json.dump(tel, open(files["telemetry_json"], "w"))
    return files["telemetry_json"], tel


def sew_signal(seed):
    """Signal `seed` of test_sew.test_oracle_matches_the_reference_module_on_many_random_signals."""
    import numpy as np
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(400, 3000)); axes = 1 if seed % 5 == 0 else 3
    rate = float(rng.choice([100.0, 200.0, 400.0]))
    t = np.arange(n) / rate
    sig = np.cumsum(rng.standard_normal((axes, n)), axis=1) * rng.uniform(0.002, 0.05) + rng.uniform(0.0, 0.3) * rng.standard_normal((axes, n))
    for k in range(3):
        sig += rng.uniform(0.1, 1.0) * np.sin(2 * np.pi * rng.uniform(0.2, 15.0) * t + rng.uniform(0, 6.28))
    q = float(rng.choice([0.9, 0.96, 0.99, 0.999])); lo = float(rng.choice([0.005, 0.01, 0.02])); hi = float(rng.choice([0.1, 0.15, 0.4]))
    return sig, t, q, lo, hi


def child(code, ref, *args):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", REF_PYTHON=os.path.join(ref, "python"), REPO=ROOT)
    return subprocess.check_output([sys.executable, "-c", code] + list(args), env=env).decode()


def facts(ref):
    out = {}
    out["gflags"] = {app: sorted(set(re.findall(r"DEFINE_\w+\(\s*(\w+)", open(os.path.join(ref, "applications", app + ".cc")).read())))
                     for app in APPS}
    used = {a: set() for a in APPS}
    for f in glob.glob(os.path.join(ref, "python", "run_*.py")):
        for m in re.finditer(r"Popen\(\[pjoin\(bin_path,\s*['\"](\w+)['\"]\)(.*?)\]\)", open(f).read(), flags=re.S):
            if m.group(1) in used:
                used[m.group(1)] |= set(re.findall(r"--(\w+)", m.group(2)))
    out["driver_flags"] = {a: sorted(used[a]) for a in APPS}
    core = os.path.join(ref, "include", "OpenCameraCalibrator", "core")
    hdr = open(os.path.join(core, "spline_trajectory_estimator.h")).read()
    pub = hdr[hdr.index("public:"):hdr.index("private:")]
    out["spline_trajectory_estimator_public"] = sorted(set(re.findall(r"\b([A-Z][A-Za-z0-9_]+)\s*\(", pub)) - {"SplineTrajectoryEstimator", "EIGEN_MAKE_ALIGNED_OPERATOR_NEW"})
    hdr = open(os.path.join(core, "imu_camera_calibrator.h")).read()
    out["imu_camera_calibrator_names"] = sorted(set(re.findall(r"\b([A-Z][A-Za-z0-9_]+)\s*\(", hdr[hdr.index("class ImuCameraCalibrator"):])) - {"ImuCameraCalibrator"})

    def public_methods(header, cls):
        h = open(os.path.join(core, header)).read()
        body = h[h.index("class " + cls):]
        body = body[body.index("public:"):body.index("private:")]
        return sorted(set(re.findall(r"\b([A-Z][A-Za-z0-9_]+)\s*\(", body)) - {cls, "EIGEN_MAKE_ALIGNED_OPERATOR_NEW"})
    out["public_methods"] = {"CameraCalibrator": public_methods("camera_calibrator.h", "CameraCalibrator"),
                             "PoseEstimator": public_methods("pose_estimator.h", "PoseEstimator"),
                             "ImuToCameraRotationEstimator": public_methods("imu_to_camera_rotation_estimator.h", "ImuToCameraRotationEstimator")}
    files = glob.glob(os.path.join(ref, "src", "io", "*.cc")) + [os.path.join(ref, "applications", a + ".cc") for a in APPS] + \
        [os.path.join(ref, "src", "core", f) for f in ("board_extractor.cc", "camera_calibrator.cc", "pose_estimator.cc")]
    keys = set()
    for f in files:
        keys |= set(re.findall(r'\[\s*"([A-Za-z0-9_ /]+)"\s*\]', open(f).read()))
    out["io_json_keys"] = sorted(keys)

    # python/sew.py on the 60 seeded signals (knot spacing, variance)
    code = r'''
import sys, os, json
sys.dont_write_bytecode = True
sys.path.insert(0, os.environ["REF_PYTHON"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tests", "golden"))
import sew
from make_reference_facts import sew_signal
out = []
for seed in range(60):
    sig, t, q, lo, hi = sew_signal(seed)
    dt, var = sew.knot_spacing_and_variance(sig, t, q, min_dt=lo, max_dt=hi)
    out.append(dict(seed=seed, dt=float(dt), var=float(var)))
print(json.dumps(out))
'''
    out["sew_random_signals"] = json.loads(child(code, ref).splitlines()[-1])

    # python/get_sew_for_dataset.py itself on the C1 telemetry (its unused imports cv2 / matplotlib / natsort stubbed)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        tel_path, tel = sew_case_c1(tmp)
        out_ref = os.path.join(tmp, "sew_ref.json")
        code = r'''
import sys, os, types
sys.dont_write_bytecode = True
for name in ("cv2", "matplotlib", "matplotlib.pyplot", "natsort"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.path.insert(0, os.environ["REF_PYTHON"])
sys.argv = ["get_sew_for_dataset.py", "--input_json_path", sys.argv[1], "--output_path", sys.argv[2]]
import get_sew_for_dataset
get_sew_for_dataset.main()
'''
        child(code, ref, tel_path, out_ref)
        out["sew_for_dataset_C1"] = dict(telemetry_sha256=telemetry_digest(tel), output=json.load(open(out_ref)))
    return out


def json_cases(ref):
    import tempfile
    from openimucameracalibrator_amd import io_files, camera_calibrator as CC
    import test_ba_applications as T
    from test_ref_json_fixture import _documents
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref", "-s", "REF=" + ref])
    tool = os.path.join(ROOT, "oracle", "_ref", "ref_json_tool")
    assert os.path.exists(tool), "the reference's JSON library did not build"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        # from_ubjson of the encoder's bytes for the synthetic corner file of test_reference_library_reads_what_this_repository_writes
        sc = T.scene_of(CC.make_calibration_dataset("pinhole", num_views=4, corners_per_view=12, seed=5))
        raw = io_files.ubjson_encode(sc)
        open(a, "wb").write(raw)
        subprocess.check_call([tool, "from_ubjson", a, b])
        out["scene"] = dict(encoder_ubjson=raw.hex(), reference_reads=json.load(open(b)))
        # the property-test documents (hypothesis, derandomized): to_ubjson of the JSON text, from_ubjson of the encoder's bytes
        from hypothesis import given, settings, HealthCheck
        docs = []

        @settings(max_examples=150, derandomize=True, deadline=None, suppress_health_check=list(HealthCheck), database=None)
        @given(_documents())
        def collect(doc):
            docs.append({"doc": doc})
        collect()
        cases = []
        for doc in docs:
            text = json.dumps(doc)
            open(a, "w").write(text)
            subprocess.check_call([tool, "to_ubjson", a, b])
            ref_bytes = open(b, "rb").read()
            mine = io_files.ubjson_encode(doc)
            open(a, "wb").write(mine)
            subprocess.check_call([tool, "from_ubjson", a, b])
            cases.append(dict(json=text, reference_ubjson=ref_bytes.hex(), encoder_ubjson=mine.hex(), reference_reads_encoder=json.load(open(b))))
        out["documents"] = cases
    return out


def main():
    ref = os.path.abspath(sys.argv[1])
    json.dump(facts(ref), open(os.path.join(HERE, "reference_facts.json"), "w"), indent=1, sort_keys=True)
    json.dump(json_cases(ref), open(os.path.join(HERE, "ref_json_cases.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
