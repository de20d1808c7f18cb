"""HostPool (manta_amd/csrc/host_pool.hpp: the helper threads of the host loops over a whole batch): exceptions in a helper's part."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_host_pool_rethrows_helper_exceptions():
    exe = os.path.join(CPP, "host_pool_throw")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "manta_amd", "csrc"),
                           os.path.join(CPP, "host_pool_throw.cpp"), "-o", exe, "-lpthread"])
    subprocess.check_call([exe])
