"""The slot rotation of the frame entries (csrc/frame_batches.h) on the host alone: tests/frame_batches_driver.cpp drives it with
recording callables, plain and under the address and undefined-behaviour sanitizers.  No device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ((1, 1), (1, 4), (2, 1), (3, 1), (3, 3), (4, 2), (5, 2), (7, 3))      # (num_frames, batch), as in the driver


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "address-undefined"))
def test_batches_rotate_through_two_slots_in_order(tmp_path, sanitize):
    """Every frame enqueued once and in ascending order, completions in enqueue order, at most two batches in flight, slot 1 idle when
    one batch covers all frames, a slot enqueued again only after its own completion, and the first non-zero code of the n-th
    enqueue or completion returned with no call behind it: the driver checks each of these and counts what fails."""
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    exe = str(tmp_path / "frame_batches_driver")
    csrc = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", csrc] + extra + [os.path.join(ROOT, "tests", "frame_batches_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l for l in lines if l[0] == "FAILED"] == []
    assert [(int(l[1]), int(l[2]), int(l[4])) for l in lines if l[0] == "pair"] == [(n, b, -(-n // min(n, b))) for n, b in PAIRS]
    assert lines[-1] == ["failures", "0"]
