"""The whole-batch calls under AddressSanitizer and UBSan, host only: tests/cpp/host_batch_sanitized.cpp (its own main) linked with the
product's host sources compiled against the wave emulator, as tests/emu/Makefile compiles them.  Nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "manta_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")


def test_batch_calls_under_address_and_ub_sanitizers():
    exe = os.path.join(CPP, "host_batch_sanitized")
    sources = [os.path.join(CPP, "host_batch_sanitized.cpp"), os.path.join(CSRC, "api_unity.cpp")]
    deps = sources + [os.path.join(EMU, "wave_emu.hpp"), os.path.join(ROOT, "include", "manta_amd.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".cpp"))]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer", "-DMANTA_WAVE_EMU", "-I" + EMU, "-I" + CSRC] + sources + ["-o", exe, "-lpthread"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0 and "host_batch_sanitized ok" in out.stdout, out.stdout[-4000:]
