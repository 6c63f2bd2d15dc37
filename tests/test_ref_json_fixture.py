"""File formats pinned by the REFERENCE's own JSON library: tests/golden/ref_corners.* were written by
oracle/_ref/ref_json_tool (= include/OpenCameraCalibrator/utils/json.h of the reference, nlohmann::json 3.7.0, built from
the reference tree by `make -C oracle ref`; tests/golden/make_ubjson_golden.py), tests/golden/ref_json_cases.json holds what the
same tool made of the documents below (tests/golden/make_reference_facts.py).  The corner file is the input of the
whole chain (src/io/read_scene.cc:25-41), so its reader must agree with the reference's serializer byte for byte."""
import json
import os
import subprocess

import numpy as np
import pytest

from openimucameracalibrator_amd import io_files, planar_init, camera_calibrator as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
CASES = os.path.join(G, "ref_json_cases.json")


def _sorted(o):
    if isinstance(o, dict):
        return {k: _sorted(o[k]) for k in sorted(o)}      # nlohmann's object type is a std::map
    if isinstance(o, list):
        return [_sorted(x) for x in o]
    return o


def test_python_decoder_and_encoder_match_the_reference_serializer():
    src = json.load(open(os.path.join(G, "ref_corners.json")))
    raw = open(os.path.join(G, "ref_corners.uson"), "rb").read()
    assert io_files.ubjson_decode(raw) == src
    assert io_files.read_scene_bson(os.path.join(G, "ref_corners.uson")) == src
    assert io_files.ubjson_encode(_sorted(src)) == raw            # byte for byte, every integer width included
    assert json.load(open(os.path.join(G, "ref_roundtrip.json"))) == src


def test_cpp_reader_parses_the_reference_bytes():
    """calibrate_camera --dry_run on the reference-made corner file: host/json_min.hpp's UbjsonReader feeds the same
    start values as the Python path computes from the decoded scene."""
    if not os.path.exists(os.path.join(CSRC, "calibrate_camera")):
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    r = subprocess.run([os.path.join(CSRC, "calibrate_camera"), "--input_corners=" + os.path.join(G, "ref_corners.uson"),
                        "--camera_model_to_calibrate=DIVISION_UNDISTORTION", "--dry_run"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    sc = json.load(open(os.path.join(G, "ref_corners.json")))
    pts = np.array([[*sc["scene_pts"][str(i)], 1.0] for i in range(len(sc["scene_pts"]))])
    w, h = sc["image_width"], sc["image_height"]
    fs, views = [], []
    for key in sorted(sc["views"]):
        ip = sc["views"][key]["image_points"]
        pid = np.array([int(k) for k in sorted(ip)], dtype=np.int32)
        uv = np.array([ip[k] for k in sorted(ip)])
        ok, R, C, f = planar_init.initialize_view(pts, pid, uv - [w / 2, h / 2])
        if ok:
            fs.append(f); views.append((key, pid, uv))
    f0 = float(np.median(fs))
    assert abs(out["focal_length"] - f0) < 1e-6 * f0 and sorted(out["poses"]) == sorted(k for k, _, _ in views)
    for key, pid, uv in views:
        ok, R, C, _ = planar_init.initialize_view(pts, pid, uv - [w / 2, h / 2], focal=f0)
        got = np.array(out["poses"][key])
        assert np.abs(got[:3] - C).max() < 1e-7 and np.abs(got[3:] - CC.rotation_to_angle_axis(R)).max() < 1e-7


def test_reference_library_reads_what_this_repository_writes():
    """files of io_files.ubjson_encode (synthetic corner files of the tests) through the reference's from_ubjson: the encoder still
    writes the bytes the reference read, and what it read is the scene."""
    ds = CC.make_calibration_dataset("pinhole", num_views=4, corners_per_view=12, seed=5)
    import test_ba_applications as T
    sc = T.scene_of(ds)
    case = json.load(open(CASES))["scene"]
    assert io_files.ubjson_encode(sc) == bytes.fromhex(case["encoder_ubjson"])
    assert case["reference_reads"] == json.loads(json.dumps(sc))


def test_cpp_reader_and_writer_reproduce_the_reference_dump(tmp_path):
    """host/json_min.hpp: UBJSON in, JSON text out with indent 4 -- the same text nlohmann::json prints for the same bytes
    (key order, layout, integers, exponents); the only differences are doubles where nlohmann 3.7.0's Grisu2 does not find
    the SHORTEST round-tripping decimal (a handful per thousand) and json_min prints the shortest: same value."""
    exe = str(tmp_path / "json_roundtrip")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "host", "json_roundtrip.cpp"), "-o", exe])
    out = str(tmp_path / "mine.json")
    subprocess.check_call([exe, os.path.join(G, "ref_corners.uson"), out, "4"])
    mine = open(out).read().splitlines(); ref = open(os.path.join(G, "ref_roundtrip.json")).read().splitlines()
    assert len(mine) == len(ref) > 1000
    diff = [(a, b) for a, b in zip(mine, ref) if a != b]
    assert len(diff) <= len(ref) // 200
    for a, b in diff:
        assert float(a.strip().rstrip(",")) == float(b.strip().rstrip(",")) and len(a) < len(b)
    # text JSON in: the parser reads the reference's own dump back to the same document
    subprocess.check_call([exe, os.path.join(G, "ref_roundtrip.json"), out, "4"])
    assert json.load(open(out)) == json.load(open(os.path.join(G, "ref_corners.json")))


def _documents():
    from hypothesis import strategies as st
    keys = st.text(alphabet="abcdefghijklmnopqrstuvwxyz0123456789_", min_size=1, max_size=8)
    ints = st.one_of(st.integers(-2**63, 2**63 - 1), st.sampled_from([0, 127, 128, 255, 256, -128, -129, 32767, 32768, -32768, -32769,
                                                                        2**31 - 1, 2**31, -2**31, -2**31 - 1]))
    texts = st.text(alphabet=st.characters(blacklist_categories=("Cs",)), max_size=12)      # any unicode incl. controls, quotes, astral
    leaves = st.one_of(st.none(), st.booleans(), ints, st.floats(allow_nan=False, allow_infinity=False), keys, texts)
    return st.recursive(leaves, lambda c: st.one_of(st.lists(c, max_size=5), st.dictionaries(st.one_of(keys, texts), c, max_size=5)), max_leaves=25)


def test_random_documents_against_the_reference_serializer(tmp_path):
    """property test with the reference library as the judge: for random documents (the 150 derandomized examples of
    _documents(), recorded with the reference's answers) the encoder's bytes equal nlohmann::json::to_ubjson's, the Python and
    C++ decoders read the reference's bytes, from_ubjson reads the encoder's."""
    a, b, c = str(tmp_path / "d.json"), str(tmp_path / "d.uson"), str(tmp_path / "back.json")
    exe = str(tmp_path / "json_roundtrip")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "host", "json_roundtrip.cpp"), "-o", exe])
    cases = json.load(open(CASES))["documents"]
    assert len(cases) == 150
    for case in cases:
        doc = json.loads(case["json"])
        open(a, "w").write(case["json"])
        raw = bytes.fromhex(case["reference_ubjson"])                 # to_ubjson of the JSON text
        open(b, "wb").write(raw)
        assert io_files.ubjson_encode(_sorted(doc)) == raw
        assert io_files.ubjson_decode(raw) == doc
        subprocess.check_call([exe, b, c, "2"])                      # the C++ reader (host/json_min.hpp) on the reference's bytes
        assert json.load(open(c)) == doc
        subprocess.check_call([exe, a, c, "0"])                      # ... and its text parser on the JSON text
        assert json.load(open(c)) == doc
        assert io_files.ubjson_encode(doc) == bytes.fromhex(case["encoder_ubjson"])   # the bytes from_ubjson was given ...
        assert case["reference_reads_encoder"] == doc                                 # ... and what it read


def test_every_json_key_of_the_reference_io_layer_is_known_to_the_host_code():
    """Drop-in at the file level: every JSON key the reference's readers / writers of this path use (string literals in
    json["..."] accesses of src/io/*.cc, the three applications' mains and the calibrator / pose estimator sources) appears in
    this repository's host code (C++ applications + Python twins).  Out of scope, listed: the raw GoPro telemetry importer
    (vendor format) and two board-description fields only the board extractor writes."""
    import glob
    import re
    keys = set(json.load(open(os.path.join(G, "reference_facts.json")))["io_json_keys"])    # (recorded by tests/golden/make_reference_facts.py)
    mine = ""
    for f in glob.glob(os.path.join(CSRC, "host", "*")) + glob.glob(os.path.join(ROOT, "openimucameracalibrator_amd", "*.py")):
        mine += open(f).read()
    literals = set(re.findall(r'"([A-Za-z0-9_ /]+)"', mine))
    out_of_scope = {"ACCL", "CORI", "GPS5", "GYRO", "cts", "precision", "samples", "streams", "value",      # read_gopro_imu_json.cc
                    "calibration_board_type", "square_size_meter"}                                               # board_extractor.cc
    assert len(keys) > 50
    assert keys - literals == out_of_scope
