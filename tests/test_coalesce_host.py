"""CPU: the request coalescer and the streaming contexts under the sanitizers.

ilias_net2_amd/csrc/sha2_coalesce.cpp and csrc/sha2_stream.cpp compile
unchanged against a host-only stand-in for the HIP runtime
(tests/cxx/hipstub: streams are worker threads with a FIFO, events mark a
position in a stream, allocations are recorded) and a stand-in
net2_launch_jobs that runs the staged jobs on the stream's thread as the
kernels' contract says, after checking every range of the launch against the
recorded allocations (inside its buffer, 64-byte aligned, disjoint).
tests/cxx/test_coalesce_host.cc drives them: built here twice, with
-fsanitize=thread and with -fsanitize=address,undefined (only the oracle's
compression arithmetic is left uninstrumented), and run as child processes,
one per run and setting, because the coalescer reads its environment once.

  battery  the stand-in against tests/cxx/jobs_battery.h, the battery the real
           kernels pass in tests/test_gpu_jobs.py: what the coalescer runs on
           here meets the contract the kernels are held to
  stress   32 threads x 300 requests (digest / HMAC / blocks from a state, all
           three rows, two-segment iovecs, 0 to 5,000 bytes), every result
           against the oracle; default settings, 1 slot, 2 slots with a 500 us
           window, 16 slots with no window, the copy mode with the lane form
  sizes    up to 400 KB from a quarter of 16 threads (the 1 MiB staging
           fills: "no room, join the next batch", grow_stage) and four
           requests of 17-20 MiB (staging past the retained 16 MiB, which
           the next small batch on the slot gives back: the page-locked
           bytes are counted)
  stream   SHA*Init / Update / Final from 8 threads at the lengths and split
           points of test_streaming_matches_oracle_call_by_call, the context
           bytes against the oracle's after every call, Pad, Final(NULL) and
           SHA-384's zeroing
  gate     a held launch keeps the device busy while 40 requests arrive:
           every request runs in exactly one launch, 41 calls in the
           statistics, every launch ordered SHA-256 first, then SHA-384/512,
           longest first within each, no job of 1,024 blocks on a lane
           (also with the lane form forced)
  fail     one failure each of stream and event creation, every hipHostMalloc
           and hipHostGetDevicePointer, hipMalloc and the H2D copy (copy
           mode), a lone launch, the first and the second launch of a
           lane-form pair, hipEventRecord, hipEventSynchronize: the callers
           of the batch get ENOMEM / EIO, nobody hangs, and the next 200
           requests on the coalescer succeed (the counter base is
           resynchronised)

A wrong result is a message and exit status 1, a sanitizer report ends the
process (halt_on_error=1), a hang ends at the program's own alarm.

Measured on a CPU-only build machine, seconds per child process as pytest
times them, TSan / ASan+UBSan: stress 1.4-1.5 / 0.3-0.9 per setting, sizes
2.9 / 0.9, stream 1.1 / 0.04, gate 1.1 / 0.1, fail 2.5 / 0.5, battery 0.3 /
0.2 after a build of about 3 s each (TSan's own exit adds about a second to
every child); the module 28 s.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"             # the compiler of tests/test_work_pool.py
CSRC = os.path.join(ROOT, "ilias_net2_amd", "csrc")
TCXX = os.path.join(ROOT, "tests", "cxx")
SOURCES = [os.path.join(TCXX, "test_coalesce_host.cc"),
           os.path.join(TCXX, "jobs_battery.cc"),
           os.path.join(TCXX, "hipstub", "hip_stub.cc"),
           os.path.join(CSRC, "sha2_coalesce.cpp"),
           os.path.join(CSRC, "sha2_stream.cpp")]
# the stand-in's hip/hip_runtime.h first on the include path
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread",
         "-I", os.path.join(TCXX, "hipstub"), "-I", CSRC, "-I", TCXX]
SANITIZERS = {
    "tsan": (["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1"}),
    "asan": (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
             # the coalescer keeps its streams for the life of the process
             {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=0",
              "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}),
}
RUNS = {
    "battery": ("battery", {}),
    "stress": ("stress", {}),
    "stress-1slot": ("stress", {"NET2_COALESCE_SLOTS": "1"}),
    "stress-2slots-500us": ("stress", {"NET2_COALESCE_SLOTS": "2",
                                       "NET2_COALESCE_WINDOW_US": "500"}),
    "stress-16slots-0us": ("stress", {"NET2_COALESCE_SLOTS": "16",
                                      "NET2_COALESCE_WINDOW_US": "0"}),
    "stress-copy-lane": ("stress", {"NET2_COALESCE_ZEROCOPY": "0",
                                    "NET2_COALESCE_JOBMODE": "2"}),
    "sizes": ("sizes", {}),
    "stream": ("stream", {}),
    # a long window: the requests behind the held launch share batches
    "gate": ("gate", {"NET2_COALESCE_WINDOW_US": "100000"}),
    "gate-lane": ("gate", {"NET2_COALESCE_WINDOW_US": "100000",
                           "NET2_COALESCE_JOBMODE": "2"}),
    "fail": ("fail", {}),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built with each sanitizer, on first use."""
    built = {}

    def get(san):
        if san in built:
            return built[san]
        clang, clangxx = os.path.join(LLVM, "clang"), os.path.join(LLVM, "clang++")
        if not os.path.exists(clangxx):
            pytest.skip("ROCm clang not present")
        out = tmp_path_factory.mktemp("coalesce_host_" + san)
        flags = SANITIZERS[san][0]
        objs = [str(out / "sha2_oracle.o")]
        # the compression arithmetic alone is not instrumented
        jobs = [subprocess.Popen([clang, "-O2", "-c", "-o", objs[0],
                                  os.path.join(ROOT, "oracle", "sha2_oracle.c")],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                 text=True)]
        for src in SOURCES:
            objs.append(str(out / (os.path.basename(src) + ".o")))
            jobs.append(subprocess.Popen([clangxx, *FLAGS, *flags, "-c", "-o",
                                          objs[-1], src], stdout=subprocess.PIPE,
                                         stderr=subprocess.STDOUT, text=True))
        for j in jobs:
            log = j.communicate()[0]
            assert j.returncode == 0, log[-3000:]
        exe = out / "test_coalesce_host"
        link = subprocess.run([clangxx, *flags, "-pthread", "-o", str(exe), *objs],
                              capture_output=True, text=True)
        assert link.returncode == 0, link.stderr[-3000:]
        built[san] = str(exe)
        return built[san]
    return get


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("san", list(SANITIZERS))
def test_coalescer_on_the_host_runtime(driver, san, run, tmp_path):
    exe = driver(san)
    arg, settings = RUNS[run]
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("NET2_", "TSAN_", "ASAN_", "UBSAN_"))}
    env.update(SANITIZERS[san][1])
    env.update(settings)
    r = subprocess.run([exe, arg], cwd=tmp_path, capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, (r.stderr + r.stdout)[-4000:]
    assert f"test_coalesce_host: {arg}: ok" in r.stdout
