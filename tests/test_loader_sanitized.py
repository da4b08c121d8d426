"""The native loader (tf_kaldi_speaker_amd/csrc/xv_loader.cpp) under the host sanitizers: tests/host_san/loader_san.cpp is compiled
TOGETHER with the loader's source into a stand-alone program, once with the address + undefined-behaviour instrumentation and once
with the thread one, the runtimes linked statically (no library load order, no environment variable), and every scenario of every
flavour runs as a child process: exit status 0, and nothing from a sanitizer on stderr.

CPU only, on the build machine: the module skips itself where a GPU is visible.  The language and codec flags come from the
library's own rule (csrc/Makefile, print-io-flags), so the instrumented code is the code the shared library is built from.

Time limits: ten times the slowest run measured on an 8-CPU build host, rounded up to whole seconds.  Measured (seconds):
    asan_ubsan   codec 0.03   hostile 0.51   create_leaks 0.04   stream 2.17
    tsan         codec 0.04   hostile 2.26   create_leaks 0.09   stream 4.08
"""
import os
import shutil
import subprocess

import pytest

from tests.kaldi_fixture import make_data_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tf_kaldi_speaker_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_san", "loader_san.cpp")

FLAVOURS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
    "tsan": ["-fsanitize=thread", "-static-libtsan"],
}
# seconds: ten times the measured run time (module docstring), rounded up
LIMITS = {
    ("asan_ubsan", "codec"): 1, ("asan_ubsan", "hostile"): 6, ("asan_ubsan", "create_leaks"): 1, ("asan_ubsan", "stream"): 22,
    ("tsan", "codec"): 1, ("tsan", "hostile"): 23, ("tsan", "create_leaks"): 1, ("tsan", "stream"): 41,
}
SCENARIOS = ["codec", "hostile", "create_leaks", "stream"]


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = pytest.mark.skipif(_gpu_visible(), reason="sanitizer programs run on the build machine, not where a GPU is visible")


def _io_flags():
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "print-io-flags"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, check=True).stdout
    flags = out.split()
    assert "-std=c++17" in flags and "-ffp-contract=off" in flags and "-pthread" in flags, flags
    return flags


@pytest.fixture(scope="session")
def san_programs(tmp_path_factory):
    """{flavour: program path, or the compiler's message when this compiler cannot link that flavour at all}"""
    out_dir = tmp_path_factory.mktemp("host_san")
    cxx = os.environ.get("CXX") or "g++"
    assert shutil.which(cxx), "no C++ compiler (%s)" % cxx
    base = [cxx] + _io_flags() + ["-O1", "-g", "-Wall"]
    probe = out_dir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    programs, builds = {}, {}
    for flavour, san in FLAVOURS.items():
        p = subprocess.run(base + san + [str(probe), "-o", str(out_dir / ("probe_" + flavour))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True)
        if p.returncode != 0:
            programs[flavour] = (None, "this compiler does not link %s: %s" % (" ".join(san), p.stdout.strip()[-600:]))
            continue
        exe = str(out_dir / ("loader_san_" + flavour))
        builds[flavour] = (exe, subprocess.Popen(base + san + ["-I", os.path.join(ROOT, "include"), HARNESS, os.path.join(CSRC, "xv_loader.cpp"), "-o", exe],
                                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True))
    for flavour, (exe, p) in builds.items():             # the flavours compile side by side
        log = p.communicate()[0]
        assert p.returncode == 0, "the %s program does not build:\n%s" % (flavour, log[-4000:])
        programs[flavour] = (exe, None)
    return programs


@pytest.fixture(scope="session")
def stream_data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kaldi_san"))
    return make_data_dir(root, num_spk=8, utts_per_spk=4, dim=30, min_frames=70, max_frames=160, seed=3)[0]


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_loader_scenario(flavour, scenario, san_programs, stream_data, tmp_path):
    exe, why_not = san_programs[flavour]
    if exe is None:
        pytest.skip(why_not)
    env = {k: v for k, v in os.environ.items() if k != "XVIO_NO_MMAP"}
    cmd = [exe, scenario, str(tmp_path / "work")] + ([stream_data] if scenario == "stream" else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=LIMITS[flavour, scenario])
    tail = "\n".join((p.stdout + "\n" + p.stderr).splitlines()[-60:])
    assert p.returncode == 0, "%s %s ended with status %d:\n%s" % (flavour, scenario, p.returncode, tail)
    assert "Sanitizer" not in p.stderr and "runtime error:" not in p.stderr, tail
    assert ("ok [%s]" % scenario) in p.stdout, tail
