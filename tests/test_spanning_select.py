"""Spanning jump-alignment QC and contig selection on the device (manta_amd/csrc/spanning_select_kernels.hpp):
manta_spanning_select_batch, the staged opt-in (manta_spanning_set_select / manta_spanning_download_select), the host adapter
selectJumpContigBatch and the refiner's setDeviceSpanningSelect switch.

Pinned on the host restatement (manta_amd/host/refiner_util.hpp through tests/cpp/host_refiner_span_capi.cpp) and, wherever
oracle/_ref/libmanta_ref_refiner.so exists, live on the UNMODIFIED reference's statics.  Every test runs on the wave emulator (CPU tier)
and on the device (gpu marker)."""
import ctypes
import os
import random
import subprocess

import pytest

from refiner_cases import HelperLib, make_cases, path_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmanta_ref_refiner.so")
SEED = 20261021       # of the random paths: the class counts of test_random_verdicts' docstring
PILE_SEED = 20261021  # of the read piles
FILTER = [2, -8, -12, 0, -1, 0]  # SVRefinerOptions::contigFilterScores of the spanning path
E_INVALID_ARG, E_EMPTY_SEQ, E_UNSUPPORTED, E_DEVICE_FAULT = -1, -4, -5, -7
DNA_SPANS, RNA_SPANS = (75, 100, 200), (36, 75, 100)


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    return request.getfixturevalue(request.param)


def build_driver(lib, tag):
    lib_dir = os.path.dirname(lib.path)
    name = os.path.basename(lib.path)[3:-3]
    so = os.path.join(CPP, "libhost_refiner_span_%s.so" % tag)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "manta_amd", "host"), os.path.join(CPP, "host_refiner_span_capi.cpp"), "-o", so,
                           "-L" + lib_dir, "-l" + name, "-Wl,-rpath," + lib_dir])
    return so


@pytest.fixture(scope="module")
def driver(dev):
    from refiner_loci import RefinerLib
    return RefinerLib(build_driver(dev, "emu" if "emu" in os.path.basename(dev.path) else "gpu"), "mine")


@pytest.fixture(scope="module")
def ref_statics():
    """the reference statics where they can be had; None elsewhere"""
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    return HelperLib(REF_SO, "ref") if os.path.exists(REF_SO) else None


# ---------------------------------------------------------------------------------------------------------------------
# host side: the restatement through the driver, the reference's statics, and the two selection rules in plain Python
# ---------------------------------------------------------------------------------------------------------------------
VERDICT_FIELDS = ("qc_fail", "ref_length1", "ref_length2", "read_length1", "read_length2", "span_low", "low1", "low2")


def host_verdict(driver, scores, c1, c2, rna):
    """isJumpAlignmentQCFail / isLowQualityJumpAlignment of the host restatement, verdict by verdict -> dict (+ `low`: the static's value)"""
    out = (ctypes.c_int * 8)()
    f = driver.lib.mine_jump_contig_verdict
    f.restype = ctypes.c_int
    low = f((ctypes.c_int32 * 6)(*scores), c1.encode(), c2.encode(), int(rna), out)
    d = dict(zip(VERDICT_FIELDS, [int(v) for v in out]))
    d["low"] = int(low)
    return d


def ref_verdict(ref_statics, scores, c1, c2, rna):
    """the same from the unmodified reference: is_low_quality_jump_alignment, and is_low_quality_spanning span by span"""
    sc = (ctypes.c_int32 * 6)(*scores)
    low = ref_statics._is_low_quality_jump_alignment(sc, 0, c1.encode(), 0, c2.encode(), 0, int(rna))
    bits = 0
    for s, span in enumerate(RNA_SPANS if rna else DNA_SPANS):
        spliced = lambda c: sum(n for n, op in segments(c) if op == "N") if rna else 0
        if ref_statics._is_low_quality_spanning(span + spliced(c1), sc, 1, int(rna), c1.encode()):
            bits |= 1 << s
        if ref_statics._is_low_quality_spanning(span + spliced(c2), sc, 0, int(rna), c2.encode()):
            bits |= 8 << s
    return dict(low=int(low), span_low=bits)


def segments(cigar):
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    return out


def qc_fail_of(c1, c2):
    """isJumpAlignmentQCFail from apath_ref_length alone"""
    return int(c1 == "" or c2 == "" or path_lengths(c1)[1] < 20 or path_lengths(c2)[1] < 20)


def select_dna(contigs, low_of):
    """selectJumpContigDNA on (qc_fail, score) per contig and a verdict function -> (selected, best, tested index or None)"""
    best = -1
    for i, c in enumerate(contigs):
        if c["qc_fail"]:
            continue
        if best == -1 or c["score"] > contigs[best]["score"]:
            best = i
    if best == -1:
        return 0, -1, None
    return (0, -1, best) if low_of(best) else (1, best, best)


def select_rna(contigs, low_of):
    """selectJumpContigRNA -> (selected, best, max score)"""
    good = [i for i, c in enumerate(contigs) if not c["qc_fail"] and not low_of(i)]
    if not good:
        return 0, -1, 0
    max_score, sel = 0, good[0]
    for i in good:
        if contigs[i]["score"] > max_score:
            max_score, sel = contigs[i]["score"], i
    for i in good:
        if contigs[i]["score"] * 2 > max_score and len(contigs[i].get("support", [])) > len(contigs[sel].get("support", [])):
            sel = i
    return 1, sel, max_score


def loci_text(driver, scores, rna, loci_items, use_device):
    """mine_select_jump_contig_loci on loci given as Lib.spanning_select_batch takes them -> (device status, best) per locus"""
    flat = [c for it in loci_items for c in it]
    n, m = len(loci_items), max(1, len(flat))
    strs = lambda v: (ctypes.c_char_p * m)(*([x.encode() for x in v] or [b""]))
    ints = lambda v: (ctypes.c_int * max(1, len(v)))(*v)
    buf = ctypes.create_string_buffer(1 << 20)
    f = driver.lib.mine_select_jump_contig_loci
    f.restype = ctypes.c_int
    f((ctypes.c_int32 * 6)(*scores), int(rna), n, ints([len(it) for it in loci_items]), strs([c["cigar1"] for c in flat]),
      strs([c["cigar2"] for c in flat]), ints([c["score"] for c in flat]), ints([len(c.get("support", [])) for c in flat]), int(use_device),
      buf, len(buf))
    text = buf.value.decode()
    assert not text.startswith("EXCEPTION"), text[:300]
    return [tuple(int(v) for v in line.split(" ")) for line in text.splitlines()]


def check_against_host(driver, ref_statics, scores, rna, loci_items, contig_recs, locus_recs, name=""):
    """every record of a clean batch against the host restatement (and the reference's statics): the contigs' lengths and verdicts, the
    tested set, the locus' choice by the mode's rule applied to those verdicts"""
    for l, (items, crecs, lrec) in enumerate(zip(loci_items, contig_recs, locus_recs)):
        where = "%s locus %d" % (name, l)
        assert lrec["status"] == 0, where
        verdicts = [host_verdict(driver, scores, c["cigar1"], c["cigar2"], rna) for c in items]
        if ref_statics is not None:
            for c, v in zip(items, verdicts):
                if not v["qc_fail"]:  # (the reference asserts on a path without a read base)
                    r = ref_verdict(ref_statics, scores, c["cigar1"], c["cigar2"], rna)
                    assert (r["low"], r["span_low"]) == (v["low"], v["span_low"]), (where, c)
        facts = [dict(qc_fail=qc_fail_of(c["cigar1"], c["cigar2"]), score=c["score"], support=c.get("support", [])) for c in items]
        low_of = lambda i: verdicts[i]["low"]
        if rna:
            selected, best, max_score = select_rna(facts, low_of)
            tested = {i for i, f in enumerate(facts) if not f["qc_fail"]}
        else:
            selected, best, t = select_dna(facts, low_of)
            max_score, tested = 0, ({t} if t is not None else set())
        for i, (c, rec, v, f) in enumerate(zip(items, crecs, verdicts, facts)):
            assert rec["status"] == 0, (where, i)
            assert rec["qc_fail"] == f["qc_fail"] == v["qc_fail"], (where, i, c)
            for k in ("ref_length1", "ref_length2", "read_length1", "read_length2"):
                assert rec[k] == v[k], (where, i, k)
            assert rec["is_tested"] == int(i in tested), (where, i)
            if i in tested:
                assert (rec["span_low"], rec["low1"], rec["low2"]) == (v["span_low"], v["low1"], v["low2"]), (where, i, c)
                assert int(rec["low1"] or rec["low2"]) == v["low"], (where, i, c)
            else:
                assert (rec["span_low"], rec["low1"], rec["low2"]) == (0, 0, 0), (where, i)
        assert (lrec["selected"], lrec["best_contig"], lrec["max_score"]) == (selected, best, max_score), (where, items)
        assert lrec["n_qc_pass"] == sum(1 for f in facts if not f["qc_fail"]), where


# ---------------------------------------------------------------------------------------------------------------------
# 1. random verdicts, both modes
# ---------------------------------------------------------------------------------------------------------------------
def random_loci():
    """the jump cases of refiner_cases.make_cases: 1 000 contig alignments, grouped by their score set into loci of 1..10 contigs with
    scores from {40, 90, 120, 300} (ties occur) and random support sets -> {score set: [locus, ...]}"""
    rng = random.Random(SEED)
    by_scores = {}
    for c in make_cases(SEED, 9000):
        if c["kind"] == "jump":
            by_scores.setdefault(tuple(c["scores"]), []).append(
                dict(cigar1=c["c1"], cigar2=c["c2"], score=rng.choice([40, 90, 120, 300]), support=list(range(rng.randint(0, 70)))))
    out = {}
    for sc, contigs in sorted(by_scores.items()):
        loci, i = [], 0
        while i < len(contigs):
            k = rng.choice([1, 1, 2, 2, 3, 3, 4, 5, 10])
            loci.append(contigs[i:i + k])
            i += k
        out[sc] = loci
    return out


def test_random_verdicts(dev, driver, ref_statics):
    """With SEED the three statics give, over the 1 000 contigs: DNA 459 QC fail / 475 low / 66 good, RNA 459 / 437 / 104; of the 278
    loci drawn here 33 are selected in DNA mode and 86 in RNA mode."""
    groups = random_loci()
    assert sum(len(l) for loci in groups.values() for l in loci) == 1000
    assert 250 <= sum(len(loci) for loci in groups.values()) <= 400
    for rna in (0, 1):
        n_fail = n_low = n_good = n_sel = n_unsel = 0
        for sc, loci in groups.items():
            contig_recs, locus_recs = dev.spanning_select_batch(list(sc), rna, loci)
            check_against_host(driver, ref_statics, list(sc), rna, loci, contig_recs, locus_recs, "rna=%d" % rna)
            for items, lrec in zip(loci, locus_recs):
                n_sel += lrec["selected"]
                n_unsel += 1 - lrec["selected"]
                for c in items:
                    v = host_verdict(driver, list(sc), c["cigar1"], c["cigar2"], rna)
                    n_fail += v["qc_fail"]
                    n_low += (not v["qc_fail"]) and v["low"]
                    n_good += (not v["qc_fail"]) and not v["low"]
            # the adapter gives the same choice
            host = loci_text(driver, list(sc), rna, loci, 0)
            assert loci_text(driver, list(sc), rna, loci, 1) == host
            assert [(0, r["best_contig"]) for r in locus_recs] == host
        # the condition on the inputs, on the restatement's (and, above, the reference's) answers alone
        assert min(n_fail, n_low, n_good) >= 30, (rna, n_fail, n_low, n_good)
        assert n_sel >= 20 and n_unsel >= 20, (rna, n_sel, n_unsel)


# ---------------------------------------------------------------------------------------------------------------------
# 2. constructed edges
# ---------------------------------------------------------------------------------------------------------------------
GOOD = "200="  # a side that is fine at every span in both modes


def long_path(n_segs):
    """a path of exactly n_segs segments, 1=1X... with an occasional 1I / 1D"""
    segs = []
    for i in range(n_segs):
        if i % 17 == 8:
            segs.append((1, "I"))
        elif i % 23 == 11:
            segs.append((1, "D"))
        else:
            segs.append((1, "=" if i % 2 == 0 else "X"))
    return segs


def constructed_loci():
    """name -> (is_rna, [locus, ...], expectation or None).  expectation: per locus (selected, best_contig)"""
    out = {}

    def add(name, loci, rna=0, expect=None):
        out[name] = (rna, loci, expect)

    def one(c1, c2, score=100, **kw):
        return dict(cigar1=c1, cigar2=c2, score=score, **kw)

    text = lambda segs: "".join("%d%s" % s for s in segs)
    # reference length 19 and 20 on either side; empty paths; insertions and clips only
    add("ref-19-left", [[one("19=", GOOD)]], expect=[(0, -1)])
    add("ref-20-left", [[one("20=", GOOD)]], expect=[(0, -1)])   # passes the fast QC, low: 20 read bases < 30
    add("ref-19-right", [[one(GOOD, "19=")]], expect=[(0, -1)])
    add("ref-20-right", [[one(GOOD, "10=10D10=")]], expect=[(0, -1)])
    add("ref-20-rna", [[one("20=", "20=")]], rna=1, expect=[(1, 0)])
    add("empty-align1", [[one("", GOOD)]], expect=[(0, -1)])
    add("empty-align2", [[one(GOOD, "")]], expect=[(0, -1)])
    add("empty-align2-rna", [[one(GOOD, "")]], rna=1, expect=[(0, -1)])
    add("ins-clip-only", [[one("10S40I", GOOD)]], expect=[(0, -1)])
    # clipped read length 29 / 30 (DNA), 19 / 20 (RNA): a deletion keeps the reference length at 20 or above
    add("read-29", [[one("29=", GOOD)], [one(GOOD, "14=10D15=")]], expect=[(0, -1), (0, -1)])
    add("read-30", [[one("30=", GOOD)], [one(GOOD, "30=")]], expect=[(1, 0), (1, 0)])
    add("read-30-clip", [[one("5S30=", GOOD)], [one("6S29=", GOOD)], [one(GOOD, "30=7S")], [one(GOOD, "29=7S")]],
        expect=[(1, 0), (0, -1), (1, 0), (0, -1)])
    add("read-19-rna", [[one("19=5D", GOOD)], [one(GOOD, "10=9D9=")]], rna=1, expect=[(0, -1), (0, -1)])
    add("read-20-rna", [[one("20=", GOOD)], [one(GOOD, "20=")]], rna=1, expect=[(1, 0), (1, 0)])
    # scoreFrac exactly 0.75 and one step below it: match 2, mismatch -8, so m matches and x mismatches of n = m + x give
    # (2m - 8x) / 2n = 3/4 at x = n / 20
    add("frac-0.75-40", [[one("38=2X", GOOD)], [one(GOOD, "2X38=")]], expect=[(1, 0), (1, 0)])
    add("frac-below-40", [[one("37=3X", GOOD)], [one(GOOD, "37=3X")]], expect=[(0, -1), (0, -1)])
    add("frac-0.75-20-rna", [[one("19=1X", GOOD)], [one(GOOD, "1X19=")]], rna=1, expect=[(1, 0), (1, 0)])
    add("frac-below-20-rna", [[one("18=2X", GOOD)]], rna=1, expect=[(0, -1)])
    add("frac-0.75-60", [[one("57=3X", GOOD)], [one(GOOD, "56=4X")]], expect=[(1, 0), (0, -1)])
    add("frac-0.75-120", [[one("114=6X", "6X114=")], [one("113=7X", GOOD)]], expect=[(1, 0), (0, -1)])
    # ... and with the open score in it: 55= 5I is 110 - 12 = 98 of 120, 48= 12I is 96 - 12 = 84 of 120 < 90 = 0.75 x 120
    add("frac-0.75-ins", [[one("54=6I", GOOD)], [one("53=7I", GOOD)]], expect=[(1, 0), (1, 0)])  # 96 / 120, 94 / 120
    add("frac-0.75-ins-exact", [[one("51=9I", GOOD)], [one("50=10I", GOOD)]], expect=[(1, 0), (0, -1)])  # 90 / 120 == 0.75, 88 / 120
    # the cut of apath_limit_ref_length: on a boundary, inside a segment, on a D, before an I and an S (both dropped)
    add("cut-on-boundary", [[one("100=75=", GOOD)], [one(GOOD, "75=4X100=")]], expect=[(1, 0), (1, 0)])
    add("cut-inside", [[one("40X100=", GOOD)], [one(GOOD, "100=40X")]], expect=[(1, 0), (1, 0)])
    add("cut-inside-x", [[one(GOOD, "70=30X100=")]], expect=[(0, -1)])  # span 75 keeps 5X, 100 keeps 30X, 200 all of them
    add("cut-on-d", [[one(GOOD, "70=10D100=")], [one("100=10D70=", GOOD)]], expect=[(1, 0), (1, 0)])
    add("cut-before-i-s", [[one(GOOD, "200=40I30S")], [one(GOOD, "25=40I30S")]], expect=[(1, 0), (0, -1)])  # (uncut: 95 read, 65 clipped)
    add("uncut-s-h", [[one(GOOD, "30=10S5H")], [one(GOOD, "29=10S5H")], [one(GOOD, "30=10I5H")]], expect=[(1, 0), (0, -1), (0, -1)])
    # (the last two: the clip is at the breakend and counts as read length: 40 read bases score 60 of 80, 39 score 58 of 78)
    add("leading-s-align1", [[one("10S30=", GOOD)], [one("5H10S30=", GOOD)], [one("10S29=", GOOD)], [one("30=10S", GOOD)], [one("29=10S", GOOD)]],
        expect=[(1, 0), (1, 0), (0, -1), (1, 0), (0, -1)])
    # low at spans 75 and 100, fine at 200: "low at all three spans"
    # (60= 6X 9=: 90 of 150; 60= 6X 34=: 140 of 200; with 100= behind it 340 of 400)
    add("low-75-100-only", [[one(GOOD, "60=6X34=100=")], [one("100=34=6X60=", GOOD)], [one(GOOD, "60=6X34=")]],
        expect=[(1, 0), (1, 0), (0, -1)])
    # selection
    add("tie-lower-index", [[one("19=", GOOD, 500), one(GOOD, GOOD, 300), one(GOOD, GOOD, 300)]], expect=[(1, 1)])
    add("tie-lower-index-rna", [[one(GOOD, GOOD, 300), one(GOOD, GOOD, 300)]], rna=1, expect=[(1, 0)])
    add("best-is-low", [[one(GOOD, GOOD, 100), one("37=3X", GOOD, 300)]], expect=[(0, -1)])
    add("best-is-low-rna", [[one(GOOD, GOOD, 100), one("18=2X", GOOD, 300)]], rna=1, expect=[(1, 0)])
    add("negative-best", [[one(GOOD, GOOD, -7), one(GOOD, GOOD, -3)]], expect=[(1, 1)])
    add("negative-best-rna", [[one(GOOD, GOOD, -7), one(GOOD, GOOD, -3)]], rna=1, expect=[(1, 0)])  # nothing exceeds 0: the first good one
    add("zero-scores-rna", [[one("19=", GOOD, 0), one(GOOD, GOOD, 0), one(GOOD, GOOD, 0, support=[0, 1])]], rna=1, expect=[(1, 1)])
    sup = lambda n: list(range(n))
    add("rna-support-half", [[one(GOOD, GOOD, 100, support=sup(3)), one(GOOD, GOOD, 50, support=sup(9))]], rna=1, expect=[(1, 0)])
    add("rna-support-half-plus", [[one(GOOD, GOOD, 101, support=sup(3)), one(GOOD, GOOD, 51, support=sup(4))]], rna=1, expect=[(1, 1)])
    add("rna-support-equal", [[one(GOOD, GOOD, 101, support=sup(4)), one(GOOD, GOOD, 51, support=sup(4))]], rna=1, expect=[(1, 0)])
    add("rna-support-chain", [[one(GOOD, GOOD, 60, support=sup(5)), one(GOOD, GOOD, 100, support=sup(2)), one(GOOD, GOOD, 70, support=sup(4)),
                               one(GOOD, GOOD, 90, support=sup(65))]], rna=1, expect=[(1, 3)])
    add("rna-support-words", [[one(GOOD, GOOD, 100, support=[0, 63, 64, 127, 128]), one(GOOD, GOOD, 90, support=[5, 70, 129, 190, 191, 200])]],
        rna=1, expect=[(1, 1)])
    # the RNA span is lengthened by the spliced length of the WHOLE path: the N behind the first 36 reference bases matters.
    # 30=3X7= 500N 100=: spans 36 / 75 / 100 alone would all end in or before the intron with 40 read bases at 50 of 80 (low); lengthened
    # by 500, span 536 still ends inside the intron, 575 and 600 reach 35 / 60 clean bases behind it (120 of 150).
    # 16=1X 500N 100=: 17 read bases before the intron are fewer than 20; span 536 reaches 19 bases behind it (62 of 72)
    add("rna-n-outside", [[one(GOOD, "30=3X7=500N100=")], [one(GOOD, "16=1X500N100=")], [one("100=500N7=3X30=", GOOD)]], rna=1,
        expect=[(1, 0), (1, 0), (1, 0)])
    add("dna-n-not-counted", [[one(GOOD, "30=3X7=500N100=")]], expect=[(0, -1)])  # (DNA: no lengthening, every span ends inside the N)
    # long paths: the cut and the sums cross a 64-lane round
    for n in (63, 64, 65, 129, 300):
        segs = long_path(n)
        add("segs-%d" % n, [[one(text(segs), GOOD)], [one(GOOD, text(segs))], [one(text(segs), text(reversed(segs)))]])
        add("segs-%d-rna" % n, [[one(text(segs), text(segs))]], rna=1)
        clean = [(1, "=")] * (n - 2) + [(1, "X"), (1, "=")]  # (one-base segments of one type side by side are a legal path_t)
        add("segs-%d-clean" % n, [[one(text(clean), text(list(reversed(clean))))]], expect=[(1, 0)])
    # the cut (75 reference bases) in the last lane of a round and in the first lane of the next: 63 / 64 one-base segments before it
    for before in (62, 63, 64, 65):
        lead = [(1, "=")] * before
        for tail in ("12=200X", "11=200X", "12=1X200=", "150="):
            segs = lead + segments(tail)
            # (neighbouring segments of one type are legal in a path_t; the walk must not care)
            add("cut-lane-%d-%s" % (before, tail), [[one(GOOD, text(segs))], [one(text(list(reversed(segs))), GOOD)]])
    # loci of 0, 1 and 64 contigs, and beyond
    add("no-contigs", [[], [one(GOOD, GOOD)], []], expect=[(0, -1), (1, 0), (0, -1)])
    add("contigs-64", [[one("19=", GOOD, 900)] * 30 + [one(GOOD, GOOD, 10 + (i % 7)) for i in range(34)]], expect=[(1, 36)])
    add("contigs-64-rna", [[one(GOOD, GOOD, 10 + (i % 7), support=list(range(i % 5))) for i in range(64)]], rna=1)
    return out


def test_constructed_edges(dev, driver, ref_statics):
    cases = constructed_loci()
    for name, (rna, loci, expect) in cases.items():
        contig_recs, locus_recs = dev.spanning_select_batch(FILTER, rna, loci)
        check_against_host(driver, ref_statics, FILTER, rna, loci, contig_recs, locus_recs, name)
        if expect is not None:
            assert [(r["selected"], r["best_contig"]) for r in locus_recs] == expect, name
        host = loci_text(driver, FILTER, rna, loci, 0)
        assert [(0, r["best_contig"]) for r in locus_recs] == host, name
        assert loci_text(driver, FILTER, rna, loci, 1) == host, name
    # what the names promise, on the records themselves
    rec = lambda name, l=0, c=0: dev.spanning_select_batch(FILTER, cases[name][0], cases[name][1])[0][l][c]
    assert rec("low-75-100-only")["span_low"] == 0b011000 and rec("low-75-100-only", 1)["span_low"] == 0b000011
    assert rec("low-75-100-only", 2)["span_low"] == 0b111000
    assert rec("cut-inside-x")["span_low"] == 0b110000 | 0b001000
    assert rec("rna-n-outside", 0)["span_low"] == 0b001000 and rec("rna-n-outside", 1)["span_low"] == 0
    assert rec("rna-n-outside", 2)["span_low"] == 0b000001 and rec("dna-n-not-counted")["span_low"] == 0b111000
    assert rec("ref-20-left")["qc_fail"] == 0 and rec("ref-19-left")["qc_fail"] == 1


def test_more_than_64_contigs(dev, driver):
    one = dict(cigar1=GOOD, cigar2=GOOD, score=100)
    loci = [[one], [dict(one, score=i) for i in range(65)], [dict(one, cigar1="19=")], [dict(one, score=i) for i in range(64)]]
    contig_recs, locus_recs = dev.spanning_select_batch(FILTER, 0, loci)
    assert [r["status"] for r in locus_recs] == [0, E_UNSUPPORTED, 0, 0]
    assert [(r["selected"], r["best_contig"]) for r in locus_recs] == [(1, 0), (0, -1), (0, -1), (1, 63)]
    assert {r["status"] for r in contig_recs[1]} == {E_UNSUPPORTED} and len(contig_recs[1]) == 65
    assert all(r["status"] == 0 for l in (0, 2, 3) for r in contig_recs[l])
    # the adapter recomputes such a locus on the host and says so
    assert loci_text(driver, FILTER, 0, loci, 1) == [(0, 0), (E_UNSUPPORTED, 64), (0, -1), (0, 63)]


# ---------------------------------------------------------------------------------------------------------------------
# 3. per-item failures and call failures
# ---------------------------------------------------------------------------------------------------------------------
def test_per_item_failures(dev, driver):
    good = lambda s: dict(cigar1=GOOD, cigar2=GOOD, score=s)
    clean = [[good(5), good(9)], [good(4), dict(good(50), cigar1="37=3X")], [good(1)], [dict(good(3), cigar2="19=")], [good(2), good(2)]]
    for code in (E_EMPTY_SEQ, E_DEVICE_FAULT):
        for rna in (0, 1):
            want_c, want_l = dev.spanning_select_batch(FILTER, rna, clean)
            loci = [list(l) for l in clean]
            loci[1] = [dict(clean[1][0], status=code), clean[1][1]]
            loci[3] = [dict(clean[3][0], status=code)]
            with pytest.raises(Exception):
                dev.spanning_select_batch(FILTER, rna, loci, strict=True)  # the call returns the code
            got_c, got_l = dev.spanning_select_batch(FILTER, rna, loci)
            assert [r["status"] for r in got_l] == [0, code, 0, code, 0]
            assert (got_l[1]["selected"], got_l[1]["best_contig"]) == (0, -1)
            assert [r["status"] for r in got_c[1]] == [code, 0] and got_c[3][0]["status"] == code
            for l in (0, 2, 4):
                assert got_l[l] == want_l[l] and got_c[l] == want_c[l], l
            assert [(0, r["best_contig"]) for r in want_l] == loci_text(driver, FILTER, rna, clean, 0)


def raw_batch(items):
    """one locus per item list, as records and arenas -> (loci, contigs, aligns, cig, bits)"""
    import numpy as np
    from manta_amd._capi import AsmContig, AsmLocusResult, SpanningAlignment, pack_cigar
    n = sum(len(it) for it in items)
    loci, contigs, aligns = (AsmLocusResult * len(items))(), (AsmContig * n)(), (SpanningAlignment * n)()
    cig, i = [], 0
    for l, it in enumerate(items):
        loci[l].n_contigs, loci[l].first_contig, loci[l].n_words = len(it), i, 1
        for c in it:
            w1, w2 = pack_cigar(c["cigar1"]), pack_cigar(c["cigar2"])
            a = aligns[i].align
            a.score = c["score"]
            a.cigar1_off, a.cigar1_len, a.cigar2_off, a.cigar2_len = len(cig), len(w1), len(cig) + len(w1), len(w2)
            cig += w1 + w2
            contigs[i].support_off, contigs[i].reject_off = 2 * i, 2 * i + 1
            i += 1
    return loci, contigs, aligns, np.array(cig, dtype=np.uint32), np.zeros(2 * n, dtype=np.uint64)


def test_outside_the_arena(dev):
    good = dict(cigar1="100=50=", cigar2=GOOD, score=7)
    items = [[good], [good], [good, good], [good], [good]]
    loci, contigs, aligns, cig, bits = raw_batch(items)
    words = len(cig)
    aligns[1].align.cigar1_off = words - 1     # the last word is inside, the one behind it is not
    aligns[3].align.cigar2_len = 1 << 31       # the length alone leaves the arena
    aligns[4].align.cigar2_off = (1 << 64) - 1  # offset + length wraps
    cs, ls = dev.spanning_select_raw(FILTER, 0, loci, contigs, aligns, cig, None)
    assert [r["status"] for r in ls] == [0, E_INVALID_ARG, E_INVALID_ARG, E_INVALID_ARG, 0]
    assert [r["status"] for r in cs] == [0, E_INVALID_ARG, 0, E_INVALID_ARG, E_INVALID_ARG, 0]
    assert (ls[0]["selected"], ls[4]["selected"]) == (1, 1)
    # a path that ends exactly at the arena's end is inside; in RNA mode a bitset that leaves its arena is the same failure
    loci, contigs, aligns, cig, bits = raw_batch(items)
    cs, ls = dev.spanning_select_raw(FILTER, 1, loci, contigs, aligns, cig, bits)
    assert all(r["status"] == 0 and r["selected"] == 1 for r in ls)
    contigs[5].support_off = len(bits)
    cs, ls = dev.spanning_select_raw(FILTER, 1, loci, contigs, aligns, cig, bits)
    assert [r["status"] for r in ls] == [0, 0, 0, 0, E_INVALID_ARG] and cs[5]["status"] == E_INVALID_ARG


def test_call_failures_write_nothing(dev):
    from manta_amd._capi import MantaError, SpanningSelect, SpanningSelectContig
    items = [[dict(cigar1=GOOD, cigar2=GOOD, score=7)] * 2, [dict(cigar1=GOOD, cigar2="19=", score=7)]]
    loci, contigs, aligns, cig, bits = raw_batch(items)

    def attempt(scores, rna, bits_arg):
        cs, ls = (SpanningSelectContig * 3)(), (SpanningSelect * 2)()
        ctypes.memset(cs, 0xA5, ctypes.sizeof(cs))
        ctypes.memset(ls, 0xA5, ctypes.sizeof(ls))
        with pytest.raises(MantaError) as e:
            dev.spanning_select_raw(scores, rna, loci, contigs, aligns, cig, bits_arg, contig_out=cs, locus_out=ls)
        assert e.value.code == E_INVALID_ARG
        assert bytes(cs) == b"\xa5" * ctypes.sizeof(cs) and bytes(ls) == b"\xa5" * ctypes.sizeof(ls)

    attempt(FILTER, 1, None)                      # RNA mode without the bitsets
    attempt([0, -8, -12, 0, -1, 0], 0, None)      # a zero match score: the score fraction would divide by zero
    attempt([0, -8, -12, 0, -1, 0], 1, bits)
    cs, ls = dev.spanning_select_raw(FILTER, 0, loci, contigs, aligns, cig, None)  # ... and the same inputs are fine otherwise
    assert [(r["status"], r["selected"]) for r in ls] == [(0, 1), (0, 0)]


# ---------------------------------------------------------------------------------------------------------------------
# 4. staged opt-in
# ---------------------------------------------------------------------------------------------------------------------
def spanning_piles(driver, tmp_path, n):
    """the piles, windows and cuts the refiner hands to the device for n breakend pairs (its own dump hook)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay_piles
    from refiner_loci import spanning_case
    rng = random.Random(PILE_SEED)
    cases = []
    for i in range(n):
        # (every sixth pile: two reads, or an inserted sequence almost as long as a read, so that some loci assemble nothing usable)
        weak = i % 6 == 5
        cases.append(spanning_case(rng, orient=("RL", "LR", "RR", "LL")[i % 4], ins_len=(120 if weak and i % 12 == 5 else (0, 25)[(i // 4) % 2]),
                                   n_reads=(2 if weak and i % 12 == 11 else rng.randint(3, 40)), same_chrom=(i % 5 == 4)))
    path = str(tmp_path / "dump.txt")
    driver.lib.mine_set_pile_dump.restype = ctypes.c_uint64
    driver.lib.mine_set_pile_dump(path.encode())
    for c in cases:
        assert not driver.run(c).startswith("EXCEPTION")
    assert driver.lib.mine_set_pile_dump(None) == n
    recs = replay_piles.parse_dump(path)
    assert [r["kind"] for r in recs] == ["J"] * n
    return recs


def test_staged_opt_in(dev, driver, tmp_path):
    from manta_amd._capi import SpanningBatch
    piles = spanning_piles(driver, tmp_path, 24)
    opts, sc, extra = piles[0]["opt"], piles[0]["scores"], piles[0]["extra"]
    assert all(r["opt"] == opts and r["scores"] == sc and r["extra"] == extra for r in piles)
    reads = [[x.encode("latin-1") for x in r["reads"]] for r in piles]
    refs1, refs2 = [r["refs"][0] for r in piles], [r["refs"][1] for r in piles]
    cuts = [r["cuts"] for r in piles]

    def staged(with_select, unset=False):
        pipe = SpanningBatch(dev, opts, sc, extra)
        if with_select:
            pipe.set_select(FILTER)
        if unset:
            pipe.set_select(None)
        pipe.upload(reads, refs1, refs2, cuts)
        pipe.run()
        stats = pipe.stats()
        res = pipe.download()
        raw = pipe.raw
        sel = pipe.download_select() if with_select and not unset else None
        if not with_select or unset:
            with pytest.raises(Exception):
                pipe.download_select()
        pipe.close()
        return res, raw, sel, stats

    res, raw, (contig_recs, locus_recs), stats = staged(True)
    loci, contigs, aligns, seq, bits, cig = raw
    n_contigs = sum(len(r["contigs"]) for r in res)
    assert len(locus_recs) == 24
    # ... equal the stand-alone call on the downloaded output, handed back as it came
    alone_c, alone_l = dev.spanning_select_raw(FILTER, 0, loci, contigs, aligns, cig, None)
    assert alone_c[:n_contigs] == contig_recs[:n_contigs]
    assert alone_l == locus_recs
    # ... and the host restatement on the same alignments
    items = [[dict(cigar1=a["cigar1"], cigar2=a["cigar2"], score=a["score"]) for a in r["aligns"]] for r in res]
    host = loci_text(driver, FILTER, 0, items, 0)
    n_sel = sum(1 for _, best in host if best >= 0)
    assert n_sel >= 8 and len(host) - n_sel >= 2, host  # (a condition on the sample: change the sample, not this line)
    assert [(r["status"], r["best_contig"]) for r in locus_recs] == host
    per_locus, i = [], 0
    for it in items:
        per_locus.append(contig_recs[i:i + len(it)])
        i += len(it)
    check_against_host(driver, None, FILTER, 0, items, per_locus, locus_recs, "staged")
    # a second pipeline that never set the stage: the same downloads, byte for byte, and download_select refuses
    res2, raw2, _, stats2 = staged(False)
    assert res2 == res
    for a, b in zip(raw, raw2):
        assert bytes(a) == bytes(b)
    for k in ("n_align_launches", "n_alignments", "ptr_matrix_bytes", "dp_cells"):
        assert stats2[k] == stats[k], k
    # switched off again, download_select refuses and the ordinary download is unchanged
    res3, raw3, _, _ = staged(True, unset=True)
    assert res3 == res
    for a, b in zip(raw, raw3):
        assert bytes(a) == bytes(b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the refiner's switch
# ---------------------------------------------------------------------------------------------------------------------
def run_batched_select(driver, cases, device_select):
    """one getCandidateAssemblyDataBatch call on a refiner with setDeviceSpanningSelect(device_select) -> (canonical text, counters)"""
    from refiner_loci import RefineInput, fill
    keep, arr = [], (RefineInput * len(cases))()
    for i, c in enumerate(cases):
        fill(arr[i], c, keep)
    buf = ctypes.create_string_buffer(1 << 24)
    counters = (ctypes.c_uint64 * 3)()
    driver.lib.mine_get_candidate_assembly_data_batch_select(arr, len(cases), int(device_select), counters, buf, len(buf))
    return buf.value.decode(), dict(zip(("spanning", "device", "fallback"), list(counters)))


@pytest.fixture(scope="module")
def ref_refiner():
    from refiner_loci import RefinerLib
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    return RefinerLib(REF_SO, "ref") if os.path.exists(REF_SO) else None


def test_refiner_switch(driver, ref_refiner):
    from refiner_loci import complex_case, spanning_case
    rng = random.Random(PILE_SEED)
    sample = [("orient-" + o, spanning_case(rng, orient=o)) for o in ("RL", "LR", "RR", "LL")]
    sample.append(("same-chrom", spanning_case(rng, same_chrom=True)))
    sample.append(("same-chrom-near", spanning_case(rng, same_chrom=True, far=False)))
    sample.append(("insertion", spanning_case(rng, ins_len=30)))
    sample.append(("insertion-RR", spanning_case(rng, orient="RR", ins_len=12)))
    sample.append(("homology", spanning_case(rng, homology=6)))
    sample.append(("near-edge", spanning_case(rng, near_edge=True)))
    sample.append(("few-reads", spanning_case(rng, n_reads=3)))
    sample.append(("two-reads", spanning_case(rng, n_reads=2)))
    sample.append(("n-rate", spanning_case(rng, n_rate=0.02)))
    sample.append(("complex-del", complex_case(rng, "del")))
    sample.append(("complex-ins", complex_case(rng, "ins")))
    n_device = 0
    for name, c in sample:
        off, off_n = run_batched_select(driver, [c], False)
        on, on_n = run_batched_select(driver, [c], True)
        assert not off.startswith("EXCEPTION"), off[:200]
        assert on == off, name
        if ref_refiner is not None:
            assert on == (ref_refiner.run_multi([c], True) if ref_refiner.multi else ref_refiner.run(c)), name
        assert off_n["device"] == 0 and off_n["fallback"] == 0, name
        # (a close pair on one chromosome is handed to the local assembler: no spanning locus)
        assert on_n["spanning"] == off_n["spanning"] == (0 if name.startswith("complex") or name == "same-chrom-near" else 1), name
        assert on_n["fallback"] == 0 and on_n["device"] == on_n["spanning"], name
        n_device += on_n["device"]
    assert n_device == 12
    # a mixed batch: spanning and complex candidates of one chromosome set in one call
    # (as test_refiner.py mixes them: the complex candidate sits on the pair's first breakend and shares its chromosomes and pile)
    rng = random.Random(PILE_SEED + 1)
    pair = spanning_case(rng, same_chrom=True)
    cx = dict(pair)
    cx.update(state=[3, 0], begin=[pair["begin"][0] + 1] * 2, end=[pair["end"][0] - 1] * 2)
    other = dict(pair, begin=[b + 2 for b in pair["begin"]], end=[e - 2 for e in pair["end"]])
    mixed = [pair, cx, other]
    off, off_n = run_batched_select(driver, mixed, False)
    on, on_n = run_batched_select(driver, mixed, True)
    assert not off.startswith("EXCEPTION"), off[:200]
    assert on == off
    assert (off_n["spanning"], off_n["device"], off_n["fallback"]) == (2, 0, 0)
    assert (on_n["spanning"], on_n["device"], on_n["fallback"]) == (2, 2, 0)
