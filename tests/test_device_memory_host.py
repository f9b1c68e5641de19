"""The owner of the library's device and pinned memory (sdrreceiver_amd/csrc/sdrx_mem.h) where its failure paths can be
reached: host/mem_check.cpp drives it with a fake allocator that fails on request, under AddressSanitizer (leak check on) and
UndefinedBehaviorSanitizer.  A stand-alone program in a child process: no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_owner_is_sound_with_a_failing_allocator(tmp_path):
    exe = tmp_path / "mem_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-o", str(exe), os.path.join(ROOT, "host", "mem_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stderr == "" and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    assert r.stdout.startswith("mem_check ok")
