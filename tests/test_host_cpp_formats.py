"""host/sdrx_demo --format: the C++ host layer's sdrj::demodSamples (host/sdrx_host.hpp) fed the demo's LCG stream as int8 and
as int16 samples.  The stream's components are -8 ... 8, so c, and 256 c, are the images of the byte c + 127: the same
sample values, hence the same messages as the dongle-byte run."""
import os
import subprocess

import pytest

from test_topology import INI_25E_LIKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "host", "sdrx_demo")

pytestmark = pytest.mark.gpu


def _run(profile, *extra):
    return subprocess.check_output([DEMO, str(profile), "--frames", "3", *extra], text=True).splitlines()


@pytest.fixture(scope="module")
def profile(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")], stdout=subprocess.DEVNULL)
    usage = subprocess.run([DEMO], capture_output=True, text=True)
    assert usage.returncode == 2 and "--format cu8|cs8|cs16" in usage.stderr  # (a demo without the flag would ignore it)
    p = tmp_path_factory.mktemp("formats") / "profile.ini"
    p.write_text(INI_25E_LIKE)
    return p


@pytest.fixture(scope="module")
def cu8_run(profile):
    """The default integer run: dongle bytes (--format cu8), which must itself be the --u8 run."""
    lines = _run(profile, "--format", "cu8")
    assert len(lines) >= 6 and lines == _run(profile, "--u8")
    return lines


@pytest.mark.parametrize("fmt", ["cs16", "cs8"])
def test_demo_prints_the_same_message_hashes_for_signed_samples(profile, cu8_run, fmt):
    assert _run(profile, "--format", fmt) == cu8_run


def test_demo_formats_on_several_devices(profile, cu8_run):
    """sdrx_group_process_fmt behind demodSamples: three shards on one GPU, the same messages in the same order."""
    assert _run(profile, "--format", "cs16", "--devices", "0,0,0") == cu8_run


def test_demo_refuses_an_unknown_format(profile):
    r = subprocess.run([DEMO, str(profile), "--frames", "1", "--format", "cf32"], capture_output=True, text=True)
    assert r.returncode == 1 and "cu8, cs8 or cs16" in r.stderr
