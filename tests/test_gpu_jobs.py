"""GPU: the coalescer's two job kernels on batches whose shape the test chose.

tests/cxx/test_jobs_gpu.cc hands the battery of tests/cxx/jobs_battery.h
straight to net2_launch_jobs (job_kernel and job_wave_kernel of
ilias_net2_amd/csrc/sha2_kernels.hip, linked from the library's own kernel
object), with no coalescer and no thread timing in between: 1 / 63 / 64 / 65 /
130 jobs per family in the lane form (a second wave, its `j >= n` guard, a
SHA-512 family starting at a job index that is no multiple of 64), lanes that
differ in block count (0 to 70), in kind (IV / state / HMAC) and in SHA-384
against SHA-512, the lane form's split of a job in 128- and 4,096-byte pieces,
the wave form at 0 / 1 / 63 / 64 / 65 / 128 / 129 / 1,024 blocks, and the
coalescer's pair of launches (long jobs a wave each, 70 small ones a lane
each) on one stream and one counter; every case with the staging copied to
device memory and read through a mapped host buffer.  Checked per case: all
eight raw state words of every job against the oracle's block transforms
(which the battery itself checks against the oracle's one-shot digest / HMAC
of the unpadded message), the canary in bytes 32-63 of SHA-256 slots and in
the slots past the last job, and the completion counter advancing by exactly
one per job (wave form) or one per 64 jobs of a family (lane form) -- what
csrc/sha2_coalesce.cpp waits for.

Measured on an MI355X: 2,422 jobs in 0.30 s inside the program.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cxx", "test_jobs_gpu")


@pytest.mark.gpu
def test_job_kernels_on_hand_built_batches():
    r = subprocess.run([BIN], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "test_jobs_gpu: ok" in r.stdout
