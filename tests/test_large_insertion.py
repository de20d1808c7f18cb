"""Small-SV large-insertion search on the device (manta_amd/csrc/smallsv_li_kernels.hpp): manta_smallsv_large_insertion_batch, the staged
opt-in (manta_smallsv_set_large_insertion / manta_smallsv_download_large_insertion), the host adapter findLargeInsertionBatch and the
refiner's setDeviceLargeInsertion switch.

Pinned on the host restatement (manta_amd/host/refiner_util.hpp through tests/cpp/host_refiner_li_capi.cpp) plus manta_align_batch and,
wherever oracle/_ref/libmanta_ref_refiner.so exists, live on the UNMODIFIED reference.  Every test runs on the wave emulator (CPU tier)
and on the device (gpu marker)."""
import ctypes
import os
import random
import subprocess

import pytest

from refiner_cases import HelperLib, make_cases, path_lengths, rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmanta_ref_refiner.so")
SEED = 20261027       # of the random paths: 167 of its 1 500 randomly limited paths are candidates by the host restatement alone
PILE_SEED = 20261021  # of the read piles
EDGE = [2, -8, -18, -1, -1, 0]       # largeInsertEdgeAlignScores (SVRefinerOptions.hpp)
COMPLETE = [2, -8, -100, 0, -1, 0]   # largeInsertCompleteAlignScores
E_INVALID_ARG, E_EMPTY_SEQ, E_UNSUPPORTED, E_DEVICE_FAULT = -1, -4, -5, -7


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    return request.getfixturevalue(request.param)


def build_driver(lib, tag):
    lib_dir = os.path.dirname(lib.path)
    name = os.path.basename(lib.path)[3:-3]
    so = os.path.join(CPP, "libhost_refiner_li_%s.so" % tag)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "manta_amd", "host"), os.path.join(CPP, "host_refiner_li_capi.cpp"), "-o", so,
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
# host side: the restatement through the driver
# ---------------------------------------------------------------------------------------------------------------------
def host_edge(driver, scores, cigar, cons):
    """isLargeInsertionEdge -> the edge record's fields"""
    out = (ctypes.c_int * 6)()
    driver.lib.mine_large_insertion_edge((ctypes.c_int32 * 6)(*scores), cigar.encode(), int(cons[0]), int(cons[1]), out)
    return dict(zip(("is_candidate", "is_left", "is_right", "contig_offset", "ref_offset", "score"), [int(v) for v in out]))


def loci_text(driver, edge_scores, complete_scores, loci_items, use_device):
    """mine_large_insertion_loci on loci given as Lib.smallsv_large_insertion_batch takes them -> one line per locus"""
    flat = [c for it in loci_items for c in it[3]]
    n, m = len(loci_items), max(1, len(flat))
    strs = lambda v, k: (ctypes.c_char_p * max(1, len(v)))(*[x.encode() for x in v]) if k else None
    ints = lambda v: (ctypes.c_int * max(1, len(v)))(*v)
    buf = ctypes.create_string_buffer(1 << 22)
    f = driver.lib.mine_large_insertion_loci
    f.restype = ctypes.c_int
    f((ctypes.c_int32 * 6)(*edge_scores), (ctypes.c_int32 * 6)(*complete_scores), n, ints([len(it[3]) for it in loci_items]),
      strs([c["seq"] for c in flat], m), ints([c["begin"] for c in flat]), strs([c["cigar"] for c in flat], m),
      ints([c["cons"][0] for c in flat]), ints([c["cons"][1] for c in flat]), strs([it[0] for it in loci_items], n),
      ints([it[1] for it in loci_items]), ints([it[2] for it in loci_items]), int(use_device), buf, len(buf))
    text = buf.value.decode()
    assert not text.startswith("EXCEPTION"), text[:300]
    return text.splitlines()


def record_text(edges, rec):
    """a locus' device records in the format of mine_large_insertion_loci"""
    cands = "".join(" %d:%d:%d:%d:%d:%d" % (i, e["is_left"], e["is_right"], e["contig_offset"], e["ref_offset"], e["score"])
                    for i, e in enumerate(edges) if e["is_candidate"])
    return "%d %d %d %d %d %d | %d %d %s | %d %d %d %d %d %d %d |%s" % (
        rec["status"], rec["has_pair"], rec["left_contig"], rec["right_contig"], rec["break_dist"], rec["break_score"], rec["score"],
        rec["begin"], rec["cigar"], rec["n_insert_segments"], rec["seg_first"], rec["seg_last"], rec["is_finished"], rec["trim_begin"],
        rec["trim_end"], rec["is_flank_ok"], cands)


# ---------------------------------------------------------------------------------------------------------------------
# 1. edge records on constructed paths
# ---------------------------------------------------------------------------------------------------------------------
def random_edge_cases():
    """the large_insert paths of refiner_cases.make_cases, each with a random conservative range and once more with the whole read
    as its range (the full-path half: what isLargeInsertAlignment alone decides)"""
    rng = random.Random(SEED)
    out = []
    for c in make_cases(SEED, 13500):
        if c["kind"] != "large_insert":
            continue
        read, _ = path_lengths(c["cigar"])
        u = rng.random()
        # (one path in nine of this generator is a candidate on its whole read: most ranges trim little, so that candidates stay frequent)
        if u < 0.9:
            cons = (rng.randint(-5, 1), read + rng.randint(-1, 5))
        elif u < 0.95:
            cons = (rng.randint(0, read // 8), rng.randint(read - read // 8, read))
        else:
            a, b = rng.randint(-5, read + 5), rng.randint(-5, read + 5)
            cons = (min(a, b), max(a, b))
        out.append(dict(scores=c["scores"], cigar=c["cigar"], cons=cons, full=False))
        out.append(dict(scores=c["scores"], cigar=c["cigar"], cons=(0, read), full=True))
    return out


def boundary_edge_cases():
    """(name, cigar, conservative range or None for the whole read, expected (is_candidate, is_left, is_right, contig_offset,
    ref_offset, score) or None), all with the edge scores"""
    out = []

    def add(name, cigar, cons=None, expect=None):
        out.append((name, cigar, cons if cons is not None else (0, path_lengths(cigar)[0]), expect))

    # thresholds 39 / 40 on refOffset, contigOffset and pathSize - contigOffset (the last is unsigned arithmetic)
    add("left-40", "40=40I", expect=(1, 1, 0, 40, 40, 80))
    add("left-ref-39", "39=41I", expect=(0, 0, 0, 0, 0, 0))
    add("left-rest-39", "41=39I", expect=(0, 0, 0, 0, 0, 0))
    add("left-contig-39", "20=21D19=60I", expect=(0, 0, 0, 0, 0, 0))  # (the max sits at 20=: refOffset 20)
    add("right-40", "40I40=", expect=(1, 0, 1, 40, 0, 80))
    add("right-ref-39", "41I39=", expect=(0, 0, 0, 0, 0, 0))
    add("right-rest-39", "39I41=", expect=(0, 0, 0, 0, 0, 0))
    # the score fraction: 2X38=40I is exactly 60 / 80 = 0.75, one more mismatch is below
    add("frac-0.75", "2X38=40I", expect=(1, 1, 0, 40, 40, 60))
    add("frac-below", "3X37=40I", expect=(0, 0, 0, 0, 0, 0))
    add("frac-0.75-right", "40I38=2X", expect=(1, 0, 1, 40, 0, 60))
    # running max: strict '>' from 0 at offsets 0; the earliest position wins ties
    add("never-positive", "4X60I", expect=(0, 0, 0, 0, 0, 0))
    add("tie-earliest", "50=1X4=60I", expect=(1, 1, 0, 50, 50, 100))  # 100 again after 1X4=
    add("tie-across-rounds", "50=" + "1X4=" * 40 + "60I")             # 100 again at segments 2, 4, ... past the first round of 64
    add("tie-right-across-rounds", "60I" + "4=1X" * 40 + "50=")
    add("max-at-round-end", "1X29=" * 32 + "60I")             # the max at segment 63
    add("max-at-round-start", "29=" + "1X29=" * 32 + "60I")   # ... at segment 64
    # soft clips are scored with offEdge here; an insertion next to a deletion pays open twice
    add("clip-lead", "10S50=60I", expect=(1, 1, 0, 60, 50, 90))
    add("clip-trail-right", "60I50=10S", expect=(1, 0, 1, 60, 0, 90))
    add("ins-del", "60=5I5D60=60I")
    add("del-at-end", "60=60I20D")
    # right candidates: read_length - off and ref_length - off of the path that was scored
    add("right-offsets", "10=50I20D60=", expect=(1, 0, 1, 60, 30, 120))
    add("right-full-vs-cons", "10=50I20D60=", cons=(12, 118))
    # apath_limit_read_length
    add("limit-same-segment", "200=", cons=(50, 150))                 # start and end in one segment: 100= left, no candidate
    add("limit-both-ends", "100=100I", cons=(10, 190))
    add("limit-start-on-boundary", "30=70=100I", cons=(30, 200))
    add("limit-end-on-boundary", "100=60I40I", cons=(0, 160))
    add("limit-begin-negative", "100=100I", cons=(-7, 200))
    add("limit-end-beyond", "100=100I", cons=(0, 1000))
    add("limit-both-negative", "100=100I", cons=(-9, -2))
    add("limit-end-never-reached", "50=20D50=100I", cons=(5, 201))
    add("limit-start-never-set", "100=100I", cons=(200, 300))
    add("limit-start-past-end", "100=100I", cons=(150, 150))
    add("limit-del-at-start", "10=20D90=100I", cons=(10, 200))        # the deletion before the start segment is dropped
    add("limit-del-at-end", "100=60I20D40I", cons=(0, 160))           # ... the one behind the end segment too
    add("limit-del-inside", "50=20D50=100I", cons=(5, 195))
    add("limit-kills-left", "100=100I", cons=(70, 200), expect=(0, 0, 0, 0, 0, 0))  # 30= left: the conservative path is no candidate
    add("limit-kills-rest", "100=100I", cons=(0, 130), expect=(0, 0, 0, 0, 0, 0))
    # a conservative-path candidate is dropped when the full path disagrees on left/right; else the offsets are the full path's
    add("disagree", "60I50=40X50=60I", cons=(0, 110), expect=(0, 0, 0, 0, 0, 0))    # conservative: right; full: neither
    add("offsets-from-full", "100=100I", cons=(20, 180), expect=(1, 1, 0, 100, 100, 160))
    add("cons-right-full-left", "50=60I50=45I", cons=(50, 205))
    # 1, 63, 64, 65, 128, 129 segments
    add("segs-1", "100=")
    for n in (63, 64, 65, 128, 129):
        body = ["1X", "29="] * (n // 2) + (["1X"] if n % 2 else [])
        body[-1] = "70I"
        add("segs-%d" % n, "".join(body))
        add("segs-%d-right" % n, "".join(reversed(body)))
        add("segs-%d-limited" % n, "".join(body), cons=(7, path_lengths("".join(body))[0] - 9))
    return out


def edge_run(lib, items):
    """items: dicts of scores, cigar, cons -> the edge record of each (one locus with one contig per item, one call per score set)"""
    rng = random.Random(3)
    groups = {}
    for i, c in enumerate(items):
        groups.setdefault(tuple(c["scores"]), []).append(i)
    out = [None] * len(items)
    for sc, idx in groups.items():
        loci = [("ACGTACGTAC", 0, 0, [dict(seq=rand_seq(rng, path_lengths(items[i]["cigar"])[0]), begin=0, cigar=items[i]["cigar"],
                                           cons=items[i]["cons"])]) for i in idx]
        edges, recs = lib.smallsv_large_insertion_batch(list(sc), COMPLETE, loci)
        for i, e, r in zip(idx, edges, recs):
            assert r["status"] == 0 and r["has_pair"] == 0
            out[i] = e[0]
    return out


def test_edge_records(dev, driver, ref_statics):
    rand = random_edge_cases()
    assert len(rand) == 3000
    named = boundary_edge_cases()
    items = rand + [dict(scores=EDGE, cigar=cigar, cons=cons) for _, cigar, cons, _ in named]
    got = edge_run(dev, items)
    kinds = set()
    n_cand = n_whole = 0
    for c, g in zip(rand, got[:len(rand)]):
        assert g.pop("status") == 0
        assert g == host_edge(driver, c["scores"], c["cigar"], c["cons"]), c
        kinds.add((g["is_candidate"], g["is_left"], g["is_right"]))
        n_cand += g["is_candidate"] and not c["full"]
        # (the whole read as the range still drops a deletion at either end of the path: only a path without one is scored as it stands)
        whole = c["full"] and c["cigar"][-1] != "D" and c["cigar"].lstrip("0123456789")[0] != "D"
        n_whole += whole
        if whole and ref_statics is not None:
            r, info = ref_statics.evaluate(dict(kind="large_insert", scores=c["scores"], cigar=c["cigar"])).split(" ")
            want = [int(v) for v in info.split(",")] if r == "1" else [0] * 5
            assert [g["is_candidate"]] + [g[k] for k in ("is_left", "is_right", "contig_offset", "ref_offset", "score")] == [int(r)] + want, c
    assert kinds == {(1, 1, 0), (1, 0, 1), (0, 0, 0)}
    assert n_whole >= 1000
    assert 10 * n_cand >= len(rand) // 2  # at least 10 % of the randomly limited cases are candidates
    for (name, cigar, cons, expect), g in zip(named, got[len(rand):]):
        assert g.pop("status") == 0, name
        assert g == host_edge(driver, EDGE, cigar, cons), name
        if expect is not None:
            assert tuple(g[k] for k in ("is_candidate", "is_left", "is_right", "contig_offset", "ref_offset", "score")) == expect, name
    by_name = {n[0]: g for n, g in zip(named, got[len(rand):])}
    assert by_name["tie-across-rounds"]["contig_offset"] == 50 and by_name["tie-right-across-rounds"]["is_right"] == 1
    assert by_name["max-at-round-end"]["is_left"] == 1 and by_name["max-at-round-start"]["is_left"] == 1
    assert by_name["limit-same-segment"]["is_candidate"] == 0 and by_name["limit-both-ends"]["is_candidate"] == 1
    for n in (63, 64, 65, 128, 129):
        assert by_name["segs-%d" % n]["is_left"] == 1 and by_name["segs-%d-right" % n]["is_right"] == 1, n


def test_host_restatement_alone_yields_candidates(driver):
    """the generator's parameters, checked without any device: at least 10 % of the randomly limited paths are candidates"""
    rand = [c for c in random_edge_cases() if not c["full"]]
    n_cand = sum(host_edge(driver, c["scores"], c["cigar"], c["cons"])["is_candidate"] for c in rand)
    assert 10 * n_cand >= len(rand), n_cand


# ---------------------------------------------------------------------------------------------------------------------
# 2. pairing, fake contig, completion alignment and finish on constructed loci
# ---------------------------------------------------------------------------------------------------------------------
def left_contig(rng, ref, begin, k, tail, mism=0, seq=None):
    """a left candidate: k reference bases from `begin` (path k=, or with `mism` leading mismatches), then `tail` novel bases"""
    s = seq
    while s is None or (tail and s[k] == ref[begin + k]):  # (the novel part does not go on matching: the alignment's shape is known)
        s = ref[begin:begin + k] + rand_seq(rng, tail)
    cigar = ("%dX%d=" % (mism, k - mism) if mism else "%d=" % k) + "%dI" % (len(s) - k)
    return dict(seq=s, begin=begin, cigar=cigar, cons=(0, len(s)))


def right_contig(rng, ref, begin, k, head, mism=0, seq=None):
    s = seq
    while s is None or (head and s[head - 1] == ref[begin - 1]):
        s = rand_seq(rng, head) + ref[begin:begin + k]
    cigar = "%dI" % (len(s) - k) + ("%d=%dX" % (k - mism, mism) if mism else "%d=" % k)
    return dict(seq=s, begin=begin, cigar=cigar, cons=(0, len(s)))


def plain_contig(rng, n):
    return dict(seq=rand_seq(rng, n), begin=10, cigar="%d=" % n, cons=(0, n))


def constructed_loci():
    """name -> (locus, complete scores); the paths steer the edge test and the pairing, the sequences the completion alignment"""
    rng = random.Random(41)
    ref = rand_seq(rng, 900)
    out = {}

    def add(name, contigs, lead=50, trail=60, complete=COMPLETE, window=ref):
        out[name] = ((window, lead, trail, contigs), complete)

    L = lambda b=200, k=80, tail=60, **kw: left_contig(rng, ref, b, k, tail, **kw)
    R = lambda b=280, k=80, head=60, **kw: right_contig(rng, ref, b, k, head, **kw)
    add("no-contigs", [])
    add("no-candidates", [plain_contig(rng, 120), plain_contig(rng, 90)])
    add("one-candidate", [L(), plain_contig(rng, 100)])
    add("two-lefts", [L(), L(b=210)])
    add("plain-pair", [L(), R()])
    add("swap", [R(), L()])                                     # the first of the pair is the right candidate
    add("dist-35", [L(), R(b=315)])                             # |200 + 80 - 315|
    add("dist-36", [L(), R(b=316)])
    add("dist-35-other-side", [L(), R(b=245)])
    add("closer-wins", [L(), R(b=300), R(b=285), R(b=290)])
    add("tie-dist-score", [L(), R(b=290, mism=2), R(b=290), R(b=270)])   # 10, 10 (better score), 10 (equal score: the earlier stays)
    add("tie-both", [L(), R(b=285), R(b=275), plain_contig(rng, 100)])
    add("not-unconditional", [L(b=170), R(b=280), L(), R(b=280, mism=3)])  # the first accepted pair (30) is replaced by 0
    add("candidates-32", [L(b=150 + 2 * i) if i % 2 == 0 else R(b=231 + 2 * i, mism=i % 3) for i in range(32)])
    add("candidates-33-plus-plain", [plain_contig(rng, 70)] + [R(b=300 - i) if i % 3 else L(b=180 + i) for i in range(33)])
    # fake contig lengths: one strip against two, and two E-bucket edges below
    for total in (1024, 1025, 1536, 1537, 2047, 2048, 2049):
        a = (total - 100) // 2
        add("fake-%d" % total, [L(k=80, tail=a - 80), R(k=80, head=total - 100 - a - 80)])
    # finish
    add("no-insertion-100", [L(), R()], complete=[2, 0, -100, 0, -1, 0])    # mismatches are free: the spacer aligns as mismatches
    # (the given paths need not be the sequences' own: 160=100I / 40I40= pair the two contigs at reference position 360)
    with_ins = lambda n: left_contig(rng, ref, 200, 160, 0, seq=ref[200:280] + rand_seq(rng, n) + ref[280:360])
    behind = right_contig(rng, ref, 360, 40, 0, seq=ref[360:440])
    add("two-equal-insertions", [dict(with_ins(100), cigar="160=100I"), behind])
    add("two-insertions-first-larger", [dict(with_ins(130), cigar="160=130I"), behind])
    add("run-with-deletion", [L(), right_contig(rng, ref, 310, 80, 60, seq=rand_seq(rng, 60) + ref[340:420])])  # 60 reference bases skipped
    add("run-at-first-segment", [dict(seq=rand_seq(rng, 80), begin=240, cigar="40=40I", cons=(0, 80)), R()], complete=[2, -8, -100, 0, -1, 1],
        lead=280)  # (the cut window begins where the right contig aligns: nothing for the left one to match)
    add("flank-left-39", [dict(L(tail=39), cigar="79=40I"), R(head=41)])  # (39 novel bases: the path says 40, or it were no candidate)
    add("flank-left-40", [L(tail=40), R(head=40)])
    add("flank-right-39", [L(tail=41), dict(R(head=39), cigar="40I79=")])
    add("too-short-to-finish", [dict(left_contig(rng, ref, 200, 80, 19), cigar="59=40I"), dict(right_contig(rng, ref, 280, 80, 20), cigar="40I60=")])
    add("no-cuts", [L(), R()], lead=0, trail=0)
    add("cut-into-the-flank", [L(), R()], lead=230, trail=60)
    return out


def run_constructed(dev, driver, names, loci):
    """-> name: (device text, host text, adapter text); one call per set of complete scores"""
    groups = {}
    for n in names:
        groups.setdefault(tuple(loci[n][1]), []).append(n)
    out = {}
    for complete, ns in groups.items():
        items = [loci[n][0] for n in ns]
        edges, recs = dev.smallsv_large_insertion_batch(EDGE, list(complete), items)
        host = loci_text(driver, EDGE, list(complete), items, 0)
        adapter = loci_text(driver, EDGE, list(complete), items, 1)
        for n, e, r, h, a in zip(ns, edges, recs, host, adapter):
            out[n] = (record_text(e, r), h, a, r)
    return out


def test_constructed_loci(dev, driver):
    loci = constructed_loci()
    got = run_constructed(dev, driver, list(loci), loci)
    for n, (text, host, adapter, _) in got.items():
        assert text == host, n
        assert adapter == host, n
    rec = {n: g[3] for n, g in got.items()}
    pair = lambda n: (rec[n]["has_pair"], rec[n]["left_contig"], rec[n]["right_contig"], rec[n]["break_dist"])
    for n in ("no-contigs", "no-candidates", "one-candidate", "two-lefts", "dist-36"):
        assert rec[n]["has_pair"] == 0 and rec[n]["cigar"] == "", n
    assert pair("plain-pair") == (1, 0, 1, 0) and pair("swap") == (1, 1, 0, 0)
    assert pair("dist-35") == (1, 0, 1, 35) and pair("dist-35-other-side") == (1, 0, 1, 35)
    assert pair("closer-wins") == (1, 0, 2, 5)
    assert pair("tie-dist-score") == (1, 0, 2, 10) and rec["tie-dist-score"]["break_score"] == 320
    assert pair("tie-both") == (1, 0, 1, 5)
    assert pair("not-unconditional") == (1, 2, 1, 0)
    assert rec["candidates-32"]["has_pair"] == 1 and rec["candidates-33-plus-plain"]["has_pair"] == 1
    for total in (1024, 1025, 1536, 1537, 2047, 2048, 2049):
        r = rec["fake-%d" % total]
        assert r["has_pair"] == 1 and path_lengths(r["cigar"])[0] == total, total
    assert rec["plain-pair"]["is_flank_ok"] == 1 and rec["plain-pair"]["n_insert_segments"] == 1
    assert rec["no-insertion-100"]["has_pair"] == 1 and rec["no-insertion-100"]["n_insert_segments"] == 0
    r = rec["two-equal-insertions"]
    assert r["cigar"].count("100I") == 2 and r["seg_first"] == r["seg_last"] == 3, r["cigar"]  # the later run
    r = rec["two-insertions-first-larger"]
    assert "130I" in r["cigar"] and r["seg_first"] == r["seg_last"] == 1, r["cigar"]
    r = rec["run-with-deletion"]
    assert "D" in r["cigar"] and r["seg_last"] == r["seg_first"] + 1, r["cigar"]
    r = rec["run-at-first-segment"]
    assert r["n_insert_segments"] == 1 and r["seg_first"] == 0, r["cigar"]
    flank = lambda n: (rec[n]["is_finished"], rec[n]["is_flank_ok"])
    assert flank("flank-left-39") == (1, 0) and flank("flank-left-40") == (1, 1) and flank("flank-right-39") == (1, 0)
    r = rec["too-short-to-finish"]  # 139 bases of insertion: isFinishedLargeInsertAlignment asks for 140
    assert r["has_pair"] == 1 and r["n_insert_segments"] == 1 and flank("too-short-to-finish") == (0, 0) and r["trim_end"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. per-item failures
# ---------------------------------------------------------------------------------------------------------------------
def test_per_item_failures(dev, driver):
    loci = constructed_loci()
    good = [loci[n][0] for n in ("plain-pair", "swap", "closer-wins", "flank-left-40")]
    failed = dict(good[0][3][0], status=E_DEVICE_FAULT)
    bad_align = (good[0][0], good[0][1], good[0][2], [failed, good[0][3][1]])
    window = good[0][0]
    empty = (window, 500, len(window) - 500, good[0][3])          # the cuts leave nothing of the window
    empty_no_pair = (window, 500, len(window) - 500, [good[0][3][0]])
    short = (window, 50, 60, [dict(good[0][3][0], seq=good[0][3][0]["seq"][:-1]), good[0][3][1]])
    items = [good[0], bad_align, good[1], empty, good[2], empty_no_pair, short, good[3]]
    edges, recs = dev.smallsv_large_insertion_batch(EDGE, COMPLETE, items)
    assert [r["status"] for r in recs] == [0, E_DEVICE_FAULT, 0, E_EMPTY_SEQ, 0, 0, E_INVALID_ARG, 0]
    assert [e["status"] for e in edges[1]] == [E_DEVICE_FAULT, 0] and edges[1][1]["is_right"] == 1
    assert [e["status"] for e in edges[6]] == [E_INVALID_ARG, 0]
    assert recs[1]["has_pair"] == 0 and recs[3]["has_pair"] == 1 and recs[3]["cigar"] == "" and recs[5]["has_pair"] == 0
    host = loci_text(driver, EDGE, COMPLETE, good, 0)
    for i, h in zip((0, 2, 4, 7), host):  # the neighbours are valid
        assert record_text(edges[i], recs[i]) == h, i
    # the adapter recomputes such a locus on the host and says so
    lines = loci_text(driver, EDGE, COMPLETE, [good[0], short, good[1]], 1)
    assert [int(l.split(" ")[0]) for l in lines] == [0, E_INVALID_ARG, 0]
    assert lines[0] == host[0] and lines[2] == host[1]


# ---------------------------------------------------------------------------------------------------------------------
# 3. staged opt-in
# ---------------------------------------------------------------------------------------------------------------------
def insertion_piles(driver, tmp_path, n):
    """the piles, windows and cuts the refiner hands to the device for n large-insertion / complex candidates (its own dump hook)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replay_piles
    from refiner_loci import complex_case, large_insertion_case
    rng = random.Random(PILE_SEED)
    cases = [large_insertion_case(rng) if i % 4 else complex_case(rng, "ins", two_haps=(i % 8 == 0), large=1) for i in range(n)]
    path = str(tmp_path / "dump.txt")
    driver.lib.mine_set_pile_dump.restype = ctypes.c_uint64
    driver.lib.mine_set_pile_dump(path.encode())
    for c in cases:
        assert not driver.run(c).startswith("EXCEPTION")
    assert driver.lib.mine_set_pile_dump(None) == n
    recs = replay_piles.parse_dump(path)
    assert [r["kind"] for r in recs] == ["S"] * n
    return recs


def test_staged_opt_in(dev, driver, tmp_path):
    import numpy as np
    from manta_amd._capi import SmallSvBatch
    piles = insertion_piles(driver, tmp_path, 24)
    opts, sc, extra = piles[0]["opt"], piles[0]["scores"], piles[0]["extra"]
    assert all(r["opt"] == opts and r["scores"] == sc and r["extra"] == extra for r in piles)
    reads = [[x.encode("latin-1") for x in r["reads"]] for r in piles]
    refs = [r["refs"][0] for r in piles]
    cuts = [r["cuts"] for r in piles]

    def staged(with_li, unset=False):
        pipe = SmallSvBatch(dev, opts, sc, extra)
        if with_li:
            pipe.set_large_insertion(EDGE, COMPLETE)
        if unset:
            pipe.set_large_insertion(None)
        pipe.upload(reads, refs, cuts)
        pipe.run()
        res = pipe.download()
        raw, keep = pipe.raw, pipe._keep
        li = pipe.download_large_insertion() if with_li and not unset else None
        if unset:
            with pytest.raises(Exception):
                pipe.download_large_insertion()
        pipe.close()
        return res, raw, keep, li

    res, raw, keep, (edges, recs) = staged(True)
    loci, contigs, aligns, seq, bits, cig = raw
    n_contigs = sum(len(r["contigs"]) for r in res)
    assert n_contigs >= 24 and len(recs) == 24
    # ... equal the stand-alone call on the downloaded output, handed back as it came
    alone_e, alone_r = dev.smallsv_large_insertion_raw(EDGE, COMPLETE, loci, contigs, aligns, seq, cig, keep[3], keep[4], keep[5])
    assert alone_e[:n_contigs] == edges[:n_contigs]
    assert alone_r == recs
    assert all(r["status"] == 0 for r in recs) and all(e["status"] == 0 for e in edges[:n_contigs])
    assert sum(r["is_flank_ok"] for r in recs) >= 8  # the piles do hold insertions too long to assemble through
    assert {r["has_pair"] for r in recs} == {0, 1}
    # ... and the host functions on the same contigs
    items, i = [], 0
    for l, r in enumerate(res):
        cs = []
        for c, a in zip(r["contigs"], r["aligns"]):
            cs.append(dict(seq=c["seq"], begin=a["begin1"], cigar=a["cigar1"], cons=(contigs[i].conservative_begin, contigs[i].conservative_end)))
            i += 1
        items.append((refs[l], cuts[l][0], cuts[l][1], cs))
    host = loci_text(driver, EDGE, COMPLETE, items, 0)
    i = 0
    for l, it in enumerate(items):
        assert record_text(edges[i:i + len(it[3])], recs[l]) == host[l], l
        i += len(it[3])
    # a second pipeline that never set the stage: the same downloads, byte for byte
    res2, raw2, _, _ = staged(False)
    assert res2 == res
    for a, b in zip(raw, raw2):
        assert bytes(a) == bytes(b)
    # switched off again, download_large_insertion refuses and the ordinary download is unchanged
    res3, raw3, _, _ = staged(True, unset=True)
    assert res3 == res
    for a, b in zip(raw, raw3):
        assert bytes(a) == bytes(b)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the refiner's switch
# ---------------------------------------------------------------------------------------------------------------------
def run_batched_li(driver, case, device_li):
    """one getCandidateAssemblyDataBatch call on a refiner with setDeviceLargeInsertion(device_li) -> (canonical text, work counters)"""
    from refiner_loci import RefineInput, fill
    keep, arr = [], (RefineInput * 1)()
    fill(arr[0], case, keep)
    buf = ctypes.create_string_buffer(1 << 24)
    counters = (ctypes.c_uint64 * 3)()
    driver.lib.mine_get_candidate_assembly_data_batch_li(arr, 1, int(device_li), counters, buf, len(buf))
    return buf.value.decode(), dict(zip(("aligned", "device", "fallback"), list(counters)))


@pytest.fixture(scope="module")
def ref_refiner():
    from refiner_loci import RefinerLib
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    return RefinerLib(REF_SO, "ref") if os.path.exists(REF_SO) else None


def test_refiner_switch(driver, ref_refiner):
    from refiner_loci import complex_case, large_insertion_case
    rng = random.Random(PILE_SEED)
    sample = [("large-insertion-%d" % i, large_insertion_case(rng)) for i in range(12)]
    for kind in ("del", "ins", "delins", "none"):
        sample.append(("complex-" + kind, complex_case(rng, kind, large=1)))
    sample.append(("complex-2hap", complex_case(rng, "del", two_haps=True, large=1)))
    sample.append(("complex-2hap-large", complex_case(rng, "ins", two_haps=True, large=1)))
    sample.append(("complex-edge", complex_case(rng, "del", near_edge=True, large=1)))
    sample.append(("complex-few-reads", complex_case(rng, "del", n_reads=2, large=1)))
    n_unknown = n_device = 0
    for name, c in sample:
        off, off_n = run_batched_li(driver, c, False)
        on, on_n = run_batched_li(driver, c, True)
        assert not off.startswith("EXCEPTION"), off[:200]
        assert on == off, name
        if ref_refiner is not None:
            assert on == (ref_refiner.run_multi([c], True) if ref_refiner.multi else ref_refiner.run(c)), name
        assert off_n["device"] == 0 and off_n["fallback"] == 0, name
        assert on_n["aligned"] == off_n["aligned"], name
        assert on_n["fallback"] == 0, name
        n_device += on_n["device"]
        if name.startswith("large-insertion"):
            n_unknown += "unknownSizeInsertion=1" in on
    assert n_unknown >= 8
    assert n_device > 0
