"""GlobalJumpIntronAligner on the device (manta_align_intron_batch, align_kernel<3, E>) against recorded outputs of the reference.

tests/golden/intron_aligner_reference_tests.json: the 16 cases of the reference's alignment/test/GlobalJumpIntronAlignerTest.cpp with the
expectations that file asserts and the reference's full output (ScoreType int).  tests/golden/intron_aligner_cases.json.xz: generated cases,
stored as seed + shape + scores + output text; tests/intron_cases.py regenerates the sequences (a digest per case guards the generator).
Both were written by tests/golden/make_intron_golden.py.  Every comparison is on the whole result as text: score, both begin:cigar pairs,
jumpInsertSize, jumpRange.  The CPU tier runs the kernels on the wave emulator and leaves out only the cases marked tier "gpu" (RNA-sized
windows of up to 50 000 bases each); `-m gpu` runs every stored case on the device."""
import json
import lzma
import os

import pytest

import intron_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TESTS = json.load(open(os.path.join(GOLDEN, "intron_aligner_reference_tests.json")))
with lzma.open(os.path.join(GOLDEN, "intron_aligner_cases.json.xz"), "rt") as _f:
    CASES = json.load(_f)
RNA = ([2, -8, -19, -1, -1, 0], -100, -15, -1)


def _problem(c, seqs):
    return (seqs[0], seqs[1], seqs[2], c["ref1_fw"], c["ref2_fw"], c["stranded"])


def _fields(text):
    w = text.split()
    assert w[0::2][:5] == ["score", "align1", "align2", "jumpInsertSize", "jumpRange"], text
    b1, c1 = w[3].split(":")
    b2, c2 = w[5].split(":")
    return dict(score=int(w[1]), begin1=int(b1), cigar1=c1, begin2=int(b2), cigar2=c2, jumpInsertSize=int(w[7]), jumpRange=int(w[9]))


def test_stored_reference_output_satisfies_the_reference_tests_own_expectations():
    assert len(TESTS) == 16
    n = 0
    for c in TESTS:
        got = _fields(c["ref_text"])
        assert c["expect"], c["name"]
        for key, want in c["expect"].items():
            assert got[key] == want, (c["name"], key, got[key], want)
            n += 1
        assert "ref_text_short" not in c  # int (Manta's instantiation) and short (the test file's) agree on all 16
    assert n == sum(len(c["expect"]) for c in TESTS) and n == 48  # every BOOST_REQUIRE_EQUAL of the test file


def test_stored_cases_cover_the_families():
    fam = {}
    for c in CASES:
        fam.setdefault(c["family"], []).append(c)
    assert sorted(fam) == ["a", "b", "c", "d", "e", "f", "rows"]
    assert all(any("N" in c["ref_text"] for c in v) for v in fam.values())
    assert all(sum(c["lens"][1:]) > 65536 and c["tier"] == "cpu" for c in fam["rows"])
    assert sum(c["tier"] == "cpu" for c in fam["f"]) == 2
    big = [c for c in fam["f"] if c["tier"] == "gpu"]
    assert len(big) >= 8 and all(150 <= c["lens"][0] <= 600 and 5000 <= min(c["lens"][1:]) and max(c["lens"][1:]) <= 50000 for c in big)
    qlens = [c["lens"][0] for c in fam["e"]]  # (the generator's indels move a length by a few bases)
    assert min(qlens) > 64 and any(q <= 128 for q in qlens) and sum(128 < q <= 420 for q in qlens) >= 4 and sum(q > 2048 for q in qlens) >= 2
    for name in "abcd":  # every strand mode, ref1Fw != ref2Fw among them
        modes = {(c["ref1_fw"], c["ref2_fw"], c["stranded"]) for c in fam[name]}
        assert {(True, True, True), (False, False, True), (True, True, False), (True, False, True), (False, True, True)} <= modes


def _run_reference_tests(lib):
    for c in TESTS:
        r = lib.align_intron_batch(c["scores"], c["jump"], c["intron_open"], c["intron_off_edge"], [_problem(c, (c["query"], c["ref1"], c["ref2"]))])[0]
        assert r["status"] == 0 and ic.result_text(r) == c["ref_text"], c["name"]


def _run_cases(lib, tiers):
    """-> number of stored cases compared; cases that share their scores go to the device in one batch"""
    groups = {}
    for i, c in enumerate(CASES):
        if c["tier"] in tiers:
            groups.setdefault((tuple(c["scores"]), c["jump"], c["intron_open"], c["intron_off_edge"]), []).append(i)
    compared = 0
    for (scores, jump, iopen, ioff), idx in groups.items():
        for at in range(0, len(idx), 64):
            part = idx[at:at + 64]
            probs = []
            for i in part:
                seqs = ic.make_case(CASES[i]["spec"])
                assert [len(s) for s in seqs] == CASES[i]["lens"] and ic.digest(*seqs) == CASES[i]["digest"], "tests/intron_cases.py changed"
                probs.append(_problem(CASES[i], seqs))
            res = lib.align_intron_batch(list(scores), jump, iopen, ioff, probs)
            for i, r in zip(part, res):
                assert r["status"] == 0, CASES[i]["spec"]
                assert ic.result_text(r) == CASES[i]["ref_text"], (CASES[i]["family"], CASES[i]["spec"], scores, jump, iopen, ioff)
                compared += 1
    return compared


def _status_codes(lib):
    from manta_amd._capi import AlignResult, AlignScores, AlignTask, MantaError
    import ctypes
    sc, jump, iopen, ioff = RNA
    # empty query / ref1 / ref2: MANTA_E_EMPTY_SEQ (-4) for that task, the others are still aligned
    probs = [("ACGT", "ACGT", "ACGT", 1, 1, 1), ("", "ACGT", "ACGT", 1, 1, 1), ("ACGT", "", "ACGT", 1, 1, 1), ("ACGT", "ACGT", "", 1, 1, 1)]
    with pytest.raises(MantaError) as e:
        lib.align_intron_batch(sc, jump, iopen, ioff, probs)
    assert e.value.code == -4
    res = lib.align_intron_batch(sc, jump, iopen, ioff, probs, strict=False)
    assert [r["status"] for r in res] == [0, -4, -4, -4] and res[0]["cigar1"] + res[0]["cigar2"] == "4="
    # is_allow_edge_insertion is refused (GlobalJumpIntronAligner.hpp: the constructor's assert)
    with pytest.raises(MantaError) as e:
        lib.align_intron_batch(sc[:5] + [1], jump, iopen, ioff, probs[:1])
    assert e.value.code == -1
    # flag bits other than ref1Fw / ref2Fw / isStranded are refused
    f = lib.lib.manta_align_intron_batch
    task = AlignTask(0, 4, 8, 4, 4, 4, 8)
    res, cig, used, s = AlignResult(), (ctypes.c_uint32 * 32)(), ctypes.c_uint64(0), AlignScores(*sc)
    arena = ctypes.create_string_buffer(b"ACGTACGTACGT")
    args = lambda: (lib.ctx, ctypes.cast(ctypes.pointer(s), ctypes.c_void_p), jump, iopen, ioff, 1, ctypes.cast(ctypes.pointer(task), ctypes.c_void_p),
                    ctypes.cast(arena, ctypes.c_void_p), 12, ctypes.cast(ctypes.pointer(res), ctypes.c_void_p), ctypes.cast(cig, ctypes.c_void_p), 32,
                    ctypes.cast(ctypes.pointer(used), ctypes.c_void_p))
    assert f(*args()) == -1
    task.reserved = 7
    assert f(*args()) == 0 and res.status == 0 and res.score == 8
    # manta_align_batch cannot carry the intron scores: kind 3 stays an invalid argument there
    with pytest.raises(MantaError) as e:
        lib.align_batch(3, sc, jump, [("ACGT", "ACGT", "ACGT")])
    assert e.value.code == -1


def test_reference_vectors_on_emulator(emu):
    _run_reference_tests(emu)


def test_stored_cases_on_emulator(emu):
    compared = _run_cases(emu, ("cpu",))
    assert compared == sum(c["tier"] == "cpu" for c in CASES) and compared == len(CASES) - sum(c["tier"] == "gpu" for c in CASES)


def test_status_codes_on_emulator(emu):
    _status_codes(emu)


@pytest.mark.gpu
def test_reference_vectors_on_gpu(gpu):
    _run_reference_tests(gpu)


@pytest.mark.gpu
def test_every_stored_case_on_gpu(gpu):
    compared = _run_cases(gpu, ("cpu", "gpu"))
    assert compared == len(CASES)


@pytest.mark.gpu
def test_status_codes_on_gpu(gpu):
    _status_codes(gpu)
