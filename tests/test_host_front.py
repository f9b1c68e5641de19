"""The front stage's host arithmetic (sdrreceiver_amd/csrc/sdrx_front.h: frame lengths per stage, windows per tile, the LDS slots
of every read, the design) at real sizes: host/front_check.cpp under AddressSanitizer and UndefinedBehaviorSanitizer.  A
stand-alone program in a child process: no GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frames_windows_and_reads_at_real_sizes(tmp_path):
    exe = tmp_path / "front_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-o", str(exe), os.path.join(ROOT, "host", "front_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == "" and "runtime error" not in r.stdout and "Sanitizer" not in r.stdout
    assert r.stdout.startswith("front_check ok")
