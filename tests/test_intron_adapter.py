"""manta_amd::GlobalJumpIntronAligner<int> of manta_amd/host/manta_amd.hpp (the reference's constructor and align() signature over
manta_align_intron_batch): the 16 vectors of the reference's own test file, against the recorded reference output."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "intron_aligner_reference_tests.json")))


def _run(lib_dir, lib_name, out):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(CPP, "host_intron_capi.cpp"), "-L" + lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir])
    text = "".join("%s %d %d %d %d %d %d %s %s %s\n" % (" ".join(str(v) for v in c["scores"][:5]), c["jump"], c["intron_open"], c["intron_off_edge"],
                                                       c["ref1_fw"], c["ref2_fw"], c["stranded"], c["query"], c["ref1"], c["ref2"]) for c in CASES)
    got = subprocess.run([out], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(CASES) == 16 and len(got) == len(CASES), got
    for c, line in zip(CASES, got):
        assert line == c["ref_text"], c["name"]


def test_intron_adapter_on_emulator(emu):
    _run(os.path.join(ROOT, "tests", "emu"), "manta_amd_emu", os.path.join(CPP, "host_intron_emu"))


@pytest.mark.gpu
def test_intron_adapter_on_gpu(gpu):
    _run(os.path.join(ROOT, "manta_amd"), "manta_amd", os.path.join(CPP, "host_intron_gpu"))
