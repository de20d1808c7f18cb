"""Small-SV contig ranking and refined candidate ranges on the device (manta_amd/csrc/smallsv_select_kernels.hpp):
manta_small_cand_sv_batch, manta_smallsv_select_batch, the staged opt-in (manta_smallsv_set_select / manta_smallsv_download_select),
the host adapter selectSmallSVContigBatch and the refiner's setDeviceSmallSelect switch.

Pinned on the host restatement (selectSmallSVContig / smallCandSVRanges of manta_amd/host/refiner_util.hpp through
tests/cpp/host_refiner_sel_capi.cpp), on a plain-Python restatement written here and, through the refiner and wherever
oracle/_ref/libmanta_ref_refiner.so exists, live on the UNMODIFIED reference.  Every test runs on the wave emulator (CPU tier) and on
the device (gpu marker)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmanta_ref_refiner.so")
SEED = 20261021  # of the random sweep: the class counts of test_random_sweep's docstring
FILTER = [2, -8, -12, 0, -1, 0]  # SVRefinerOptions::contigFilterScores
E_INVALID_ARG, E_UNSUPPORTED, E_CAPACITY, E_DEVICE_FAULT = -1, -5, -6, -7
READ_OPS, REF_OPS = "MIS=X", "MDN=X"


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    return request.getfixturevalue(request.param)


def build_driver(lib, tag):
    lib_dir = os.path.dirname(lib.path)
    name = os.path.basename(lib.path)[3:-3]
    so = os.path.join(CPP, "libhost_refiner_sel_%s.so" % tag)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "manta_amd", "host"), os.path.join(CPP, "host_refiner_sel_capi.cpp"), "-o", so,
                           "-L" + lib_dir, "-l" + name, "-Wl,-rpath," + lib_dir])
    return so


@pytest.fixture(scope="module")
def driver(dev):
    from refiner_loci import RefinerLib
    return RefinerLib(build_driver(dev, "emu" if "emu" in os.path.basename(dev.path) else "gpu"), "mine")


# ---------------------------------------------------------------------------------------------------------------------
# the two rules in plain Python
# ---------------------------------------------------------------------------------------------------------------------
def cigar_text(segs):
    """[(length, op), ...] -> text; zero lengths dropped, equal neighbours merged (as the host's cigar_to_apath would: segment indices
    must mean the same on both sides)"""
    out = []
    for n, op in segs:
        if n == 0:
            continue
        if out and out[-1][1] == op:
            out[-1] = (out[-1][0] + n, op)
        else:
            out.append((n, op))
    return "".join("%d%s" % s for s in out), out


def segments(cigar):
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    return out


def py_ranges(ref, contig, begin, cigar, first, last):
    """setSmallCandSV's ranges (SVCandidateAssemblyRefiner.cpp:742-762) and getVariantRange (:677-717); the left walk ends with the
    value reached where the reference's index would become negative"""
    ref_pos, read_pos = begin, 0
    for i, (n, op) in enumerate(segments(cigar)):
        if i == first:
            ref_begin, read_begin = ref_pos, read_pos
        if op in REF_OPS:
            ref_pos += n
        if op in READ_OPS:
            read_pos += n
        if i == last:
            ref_end, read_end = ref_pos, read_pos
    right = 0
    while right < min(len(ref) - ref_end, len(contig) - read_end) and ref[ref_begin + right] == contig[read_begin + right]:
        right += 1
    left = 0
    while left >= max(-ref_begin, -read_begin):
        i, j = ref_end + left - 1, read_end + left - 1
        if i < 0 or j < 0 or ref[i] != contig[j]:
            break
        left -= 1
    return dict(ref_begin=ref_begin, ref_end=ref_end, read_begin=read_begin, read_end=read_end, cipos_begin=left, cipos_end=right)


def py_select(contigs):
    """the rank rule (:2119-2166) and the swap test (:2169-2219) over dicts of candidate, score, jumped, largest_indel, support ->
    dict(rank1, rank2, rank2_is_best, best, why).  The ratio tests in float32, as the reference's float expressions: 9 > 10 * 0.9f is
    false there and true in double (the float-10-9, float-20-18 and float-30-27 cases below)."""
    f = np.float32
    r1 = r2 = None
    for i, c in enumerate(contigs):
        if not c.get("candidate", 1):
            continue
        j, j1 = bool(c.get("jumped", 0)), bool(r1 is not None and contigs[r1].get("jumped", 0))
        if r1 is None or (j and not j1) or (j == j1 and c["score"] > contigs[r1]["score"]):
            if r1 is not None:
                r2 = r1
            r1 = i
        elif r2 is None or c["score"] > contigs[r2]["score"]:
            r2 = i
    out = dict(rank1=-1 if r1 is None else r1, rank2=-1 if r2 is None else r2, rank2_is_best=0, best=-1 if r1 is None else r1, why="none")
    if r1 is None:
        return out
    out["why"] = "single"
    if r2 is None:
        return out
    a, b = contigs[r1], contigs[r2]
    if a.get("jumped", 0) and not b.get("jumped", 0):
        out["why"] = "jumped"
        return out
    n1, n2 = len(a.get("support", [])), len(b.get("support", []))
    score_ok = f(b["score"]) > f(a["score"]) * f(0.9)
    by_support = f(n2) > f(n1) * f(1.2)
    by_size = f(b.get("largest_indel", 0)) > f(a.get("largest_indel", 0)) * f(1.1)
    out["why"] = "kept"
    if score_ok and (by_support or by_size):
        out.update(rank2_is_best=1, best=r2, why="support" if by_support else "size")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# host side through the driver
# ---------------------------------------------------------------------------------------------------------------------
RANGE_FIELDS = ("ref_begin", "ref_end", "read_begin", "read_end", "cipos_begin", "cipos_end")


def host_ranges(driver, ref, contig, begin, cigar, first, last):
    out = (ctypes.c_int * 6)()
    driver.lib.mine_small_cand_sv_ranges(ref.encode(), contig.encode(), int(begin), cigar.encode(), int(first), int(last), out)
    return dict(zip(RANGE_FIELDS, [int(v) for v in out]))


def loci_text(driver, loci_items, use_device):
    """mine_select_small_sv_loci on loci given as Lib.smallsv_select_batch takes them -> per locus (device status, rank1, rank2,
    rank2IsBest, best, [candidate dict, ...])"""
    flat = [(ref, c) for ref, items in loci_items for c in items]
    n, m = len(loci_items), max(1, len(flat))
    strs = lambda v: (ctypes.c_char_p * max(1, len(v)))(*([x.encode() for x in v] or [b""]))
    ints = lambda v: (ctypes.c_int * max(1, len(v)))(*(v or [0]))
    buf = ctypes.create_string_buffer(1 << 24)
    f = driver.lib.mine_select_small_sv_loci
    f.restype = ctypes.c_int
    f(n, ints([len(it) for _, it in loci_items]), strs([ref for ref, _ in loci_items]), strs([c["seq"] for _, c in flat]),
      ints([c["begin"] for _, c in flat]), strs([c["cigar"] for _, c in flat]), ints([c["score"] for _, c in flat]),
      ints([int(c.get("jumped", 0)) for _, c in flat]), ints([int(c.get("candidate", 1)) for _, c in flat]),
      strs([",".join("%d-%d" % p for p in c.get("segments", [])) for _, c in flat]),
      strs([",".join(str(r) for r in c.get("support", [])) for _, c in flat]), int(use_device), buf, len(buf))
    text = buf.value.decode()
    assert not text.startswith("EXCEPTION"), text[:300]
    out = []
    for line in text.splitlines():
        parts = line.split("|")
        head = [int(v) for v in parts[0].split(" ")]
        cands = []
        for p in parts[1:]:
            seg, *vals = p.split(" ")
            first, last = seg.split("-")
            cands.append(dict(zip(("seg_first", "seg_last") + RANGE_FIELDS, [int(first), int(last)] + [int(v) for v in vals])))
        out.append(tuple(head) + (cands,))
    return out


def strip(c):
    return {k: v for k, v in c.items() if k != "status"}


def check_loci(dev, driver, loci_items, name=""):
    """every record of a clean batch against the plain-Python restatement, the host restatement and the adapter -> the records"""
    recs = dev.smallsv_select_batch(loci_items)
    host = loci_text(driver, loci_items, 0)
    assert loci_text(driver, loci_items, 1) == host, name
    for l, ((ref, items), rec, h) in enumerate(zip(loci_items, recs, host)):
        where = "%s locus %d" % (name, l)
        want = py_select(items)
        assert rec["status"] == 0, where
        assert (rec["rank1_contig"], rec["rank2_contig"], rec["rank2_is_best"], rec["best_contig"], rec["selected"]) == (
            want["rank1"], want["rank2"], want["rank2_is_best"], want["best"], int(want["best"] >= 0)), (where, rec, want)
        cands = []
        if want["best"] >= 0:
            b = items[want["best"]]
            for first, last in b.get("segments", []):
                r = py_ranges(ref, b["seq"], b["begin"], b["cigar"], first, last)
                r.update(seg_first=first, seg_last=last)
                cands.append(r)
        assert [strip(c) for c in rec["candidates"]] == cands, where
        assert all(c["status"] == 0 for c in rec["candidates"]), where
        assert h == (0, want["rank1"], want["rank2"], want["rank2_is_best"], want["best"], cands), where
    return recs


# ---------------------------------------------------------------------------------------------------------------------
# 1. range and slide edges through manta_small_cand_sv_batch
# ---------------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n, avoid=""):
    out = []
    for _ in range(n):
        out.append(rng.choice([b for b in "ACGT" if b != (out[-1] if out else avoid)]))
    return "".join(out)


def other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def periodic_tail(ev, k):
    """k bases that continue ev's period: (ev + tail)[o] == tail[o] for o < k"""
    tail = []
    for o in range(k):
        tail.append((ev + "".join(tail))[o])
    return "".join(tail)


def slide_tasks(rng):
    """right slides of 0, 1, 63, 64, 65, 128 and 129 bases for a pure deletion and a pure insertion, each ended by a mismatch, by the
    end of the window and by the end of the contig -> [(name, task, expected cipos_end)]"""
    out = []
    for kind in ("del", "ins"):
        for k in (0, 1, 63, 64, 65, 128, 129):
            for stop in ("mismatch", "window", "contig"):
                prefix = rand_seq(rng, 20)
                ev = rand_seq(rng, 7, avoid=prefix[-1])
                while ev[-1] == prefix[-1]:  # no left slide
                    ev = rand_seq(rng, 7)
                tail = periodic_tail(ev, k)
                nxt = (ev + tail)[k]  # what the side holding the event reads at offset k
                short, long_ = prefix + tail, prefix + ev + tail  # the side without / with the event
                path = [(20, "="), (7, "D" if kind == "del" else "I"), (k, "=")]
                if stop == "mismatch":
                    brk = other(nxt) + rand_seq(rng, 5)
                    short, long_ = short + brk, long_ + brk
                    path.append((6, "="))
                ref, contig = (long_, short) if kind == "del" else (short, long_)
                if stop == "window":  # the window ends behind the k bases; the contig goes on in a soft clip that would still match
                    contig += (nxt + "ACG") if kind == "del" else "ACGT"
                    path.append((4, "S"))
                if stop == "contig":  # the contig ends; the window goes on with what would still match
                    ref += (nxt + "ACGTA") if kind == "ins" else "ACGTAC"
                text, _ = cigar_text(path)
                out.append(("%s-%d-%s" % (kind, k, stop), (ref, contig, 0, text, 1, 1), k))
    return out


def alternating(n_segs, events):
    """a path of exactly n_segs segments, 1=1X1=... with the given {index: (length, op)} in it (no equal neighbours), its window and
    contig -> (ref, contig, cigar text)"""
    rng = random.Random(n_segs)
    ref, contig, segs = [], [], []
    for i in range(n_segs):
        if i in events:
            n, op = events[i]
            s = rand_seq(rng, n)
            if op == "D":
                ref.append(s)
            else:
                contig.append(s)
            segs.append((n, op))
            continue
        # neighbours of an event are '=' and 'X' alternately; an event breaks the parity so that equal ops never touch
        op = "=" if (not segs or segs[-1][1] != "=") else "X"
        b = rng.choice("ACGT")
        ref.append(b)
        contig.append(b if op == "=" else other(b))
        segs.append((1, op))
    text, merged = cigar_text(segs)
    assert len(merged) == n_segs
    return "".join(ref), "".join(contig), text


def edge_tasks():
    """name -> task (reference window, contig, begin position, cigar text, seg_first, seg_last)"""
    rng = random.Random(SEED)
    out = {}
    for name, task, k in slide_tasks(rng):
        out["slide-" + name] = task
    # a mismatch at the first compared base is slide-*-0-mismatch; segment kinds
    p, s = rand_seq(rng, 15), rand_seq(rng, 15)
    d5, i4 = rand_seq(rng, 5), rand_seq(rng, 4)
    out["kind-del"] = (p + d5 + s, p + s, 0, "15=5D15=", 1, 1)
    out["kind-ins"] = (p + s, p + i4 + s, 0, "15=4I15=", 1, 1)
    out["kind-insdel"] = (p + d5 + s, p + i4 + s, 0, "15=4I5D15=", 1, 2)
    out["kind-insdel-ins-only"] = (p + d5 + s, p + i4 + s, 0, "15=4I5D15=", 1, 1)
    out["kind-insdel-del-only"] = (p + d5 + s, p + i4 + s, 0, "15=4I5D15=", 2, 2)
    out["kind-multi"] = (p + d5 + "AC" + s, p + i4 + "GT" + i4 + s, 0, "15=4I2X5D4I15=", 1, 4)
    out["kind-multi-with-match"] = (p + d5 + "AC" + s, p + i4 + "AC" + i4 + s, 0, "15=4I2=5D4I15=", 1, 4)
    out["begin-pos"] = ("GGGGGGG" + p + d5 + s + "CC", p + s, 7, "15=5D15=", 1, 1)
    # position in the path: the first, a middle and the last path index
    out["pos-first-del"] = (d5 + s, s, 0, "5D15=", 0, 0)
    out["pos-first-ins"] = (s, i4 + s, 0, "4I15=", 0, 0)
    out["pos-first-ins-begin"] = ("TT" + s, i4 + s, 2, "4I15=", 0, 0)
    out["pos-last-del"] = (p + d5, p, 0, "15=5D", 1, 1)
    out["pos-last-ins"] = (p, p + i4, 0, "15=4I", 1, 1)
    out["pos-whole-path"] = (p + d5 + s, p + i4 + s, 0, "15=4I5D15=", 0, 3)
    # paths of 1, 64, 65 and 130 segments: the carried prefix sums
    out["segs-1-ins"] = ("ACGTACGTAC", "TTGCA", 3, "5I", 0, 0)
    out["segs-1-del"] = ("ACGTACGTAC", "", 3, "5D", 0, 0)
    out["segs-1-match"] = ("ACGTACGTAC", "GTACG", 2, "5=", 0, 0)
    for n in (64, 65, 130):
        for at in sorted({0, 31, 62, 63, 64, n - 2, n - 1}):
            if at >= n:
                continue
            for op in ("D", "I"):
                ref, contig, text = alternating(n, {at: (3, op)})
                out["segs-%d-%s-at-%d" % (n, op, at)] = (ref, contig, 0, text, at, at)
        ref, contig, text = alternating(n, {5: (3, "D"), 6: (2, "I"), n - 3: (4, "I")})
        out["segs-%d-range" % n] = (ref, contig, 0, text, 5, n - 3)
        out["segs-%d-all" % n] = (ref, contig, 0, text, 0, n - 1)
    # left compares: cipos_begin of -1 and -k
    x = "CG"
    for k in (1, 2, 5, 63, 64, 65, 130):
        out["left-%d-del" % k] = (x + "A" * k + "AAA" + "CT" + s, x + "A" * k + "CT" + s, 0, "%d=3D%d=" % (2 + k, 2 + len(s)), 1, 1)
        out["left-%d-ins" % k] = (x + "A" * k + "CT" + s, x + "A" * k + "AAA" + "CT" + s, 0, "%d=3I%d=" % (2 + k, 2 + len(s)), 1, 1)
        # ... up to both bounds: nothing but the homopolymer before the event.  A pure event reaches index -1 on its empty side, where
        # the reference would read out of bounds: the value reached is reported.  An event with both sides ends one step further, at
        # max(-refBegin, -readBegin) - 1, without such a read
        out["left-%d-del-to-start" % k] = ("A" * k + "AAA" + "CT" + s, "A" * k + "CT" + s, 0, "%d=3D%d=" % (k, 2 + len(s)), 1, 1)
        out["left-%d-ins-to-start" % k] = ("A" * k + "CT" + s, "A" * k + "AAA" + "CT" + s, 0, "%d=3I%d=" % (k, 2 + len(s)), 1, 1)
        out["left-%d-insdel-to-start" % k] = ("A" * k + "AA" + "CT" + s, "A" * k + "AAA" + "CT" + s, 0, "%d=3I2D%d=" % (k, 2 + len(s)), 1, 2)
        out["left-%d-begin-pos" % k] = ("GGG" + "A" * k + "AAA" + "CT" + s, "A" * k + "CT" + s, 3, "%d=3D%d=" % (k, 2 + len(s)), 1, 1)
    out["left-first-index-del"] = ("AAA" + s, s, 0, "3D15=", 0, 0)   # read index -1 at the first compare
    out["left-first-index-ins"] = (s, "AAA" + s, 0, "3I15=", 0, 0)   # reference index -1 at the first compare
    # the shapes that give real CIPOS
    out["homopolymer-ins"] = (p + "C" + "T" * 9 + "G" + s, p + "C" + "T" * 12 + "G" + s, 0, "16=3I%d=" % (9 + 1 + 15), 1, 1)
    out["homopolymer-ins-right"] = (p + "C" + "T" * 9 + "G" + s, p + "C" + "T" * 12 + "G" + s, 0, "25=3I%d=" % 16, 1, 1)
    unit = "CAG"
    out["tandem-del"] = (p + "T" + unit * 8 + "A" + s, p + "T" + unit * 6 + "A" + s, 0, "16=6D%d=" % (18 + 1 + 15), 1, 1)
    out["tandem-del-mid"] = (p + "T" + unit * 8 + "A" + s, p + "T" + unit * 6 + "A" + s, 0, "22=6D%d=" % (12 + 1 + 15), 1, 1)
    return out


EXPECT = {  # what the names promise, by value: (cipos_begin, cipos_end)
    "kind-del": None, "left-1-del": (-1, None), "left-5-ins": (-5, None), "left-130-del": (-130, None),
    "left-5-del-to-start": (-5, None), "left-64-ins-to-start": (-64, None), "left-5-insdel-to-start": (-6, None),
    "left-5-begin-pos": (-5, None), "left-first-index-del": (0, None), "left-first-index-ins": (0, None),
    "homopolymer-ins": (0, 9), "homopolymer-ins-right": (-9, 0), "tandem-del": (0, 18), "tandem-del-mid": (-6, 12),
}


def test_range_and_slide_edges(dev, driver):
    rng = random.Random(SEED)
    tasks = edge_tasks()
    names = sorted(tasks)
    assert all(1 <= len(t[0]) <= 200 and len(t[1]) <= 200 for t in tasks.values())
    got = dev.small_cand_sv_batch([tasks[n] for n in names], strict=True)  # every task succeeds, the index -1 cases included
    for name, rec in zip(names, got):
        ref, contig, begin, cigar, first, last = tasks[name]
        want = py_ranges(ref, contig, begin, cigar, first, last)
        assert rec["status"] == 0 and (rec["seg_first"], rec["seg_last"]) == (first, last), name
        assert {k: rec[k] for k in RANGE_FIELDS} == want, (name, rec, want)
        assert host_ranges(driver, ref, contig, begin, cigar, first, last) == want, name
        assert rec["cipos_begin"] <= 0 <= rec["cipos_end"], name
        if EXPECT.get(name):
            lo, hi = EXPECT[name]
            assert rec["cipos_begin"] == lo and (hi is None or rec["cipos_end"] == hi), (name, rec)
    # the slides are what their names say, ended as they say
    by_name = dict(zip(names, got))
    for name, task, k in slide_tasks(rng):
        rec = by_name["slide-" + name]
        assert (rec["cipos_begin"], rec["cipos_end"]) == (0, k), (name, rec)
        ref, contig = task[0], task[1]
        room_ref, room_read = len(ref) - rec["ref_end"], len(contig) - rec["read_end"]
        if name.endswith("window"):
            assert room_ref == k < room_read, name
        elif name.endswith("contig"):
            assert room_read == k < room_ref, name
        else:
            assert k < min(room_ref, room_read), name
    # an empty refRange / readRange where the kind says so
    assert by_name["kind-del"]["read_begin"] == by_name["kind-del"]["read_end"] and by_name["kind-ins"]["ref_begin"] == by_name["kind-ins"]["ref_end"]
    assert by_name["pos-whole-path"]["ref_begin"] == 0 and by_name["pos-whole-path"]["read_end"] == len(tasks["pos-whole-path"][1])


def test_invalid_tasks(dev):
    from manta_amd._capi import small_cand_sv_arrays
    p, s, d5 = "ACGTTGCAAGGCTAT", "GATTACAGATTACAG", "CCCCC"
    good = (p + d5 + s, p + s, 0, "15=5D15=", 1, 1)
    tasks = [good,
             (p + d5 + s, p + s, 0, "15=5D15=", 1, 3),        # a segment index past the path
             good,
             (p + d5 + s, p + s, 0, "15=5D15=", 3, 3),
             (p + d5 + s, p + s, 0, "15=5D15=", 2, 1),        # first > last
             (p + d5 + s, p + s, 1, "15=5D15=", 1, 1),        # the reference span leaves the window by one base
             (p + d5 + s, p + s, -1, "15=5D15=", 1, 1),
             (p + d5 + s, p + s + "A", 0, "15=5D15=", 1, 1),  # the read length differs from the contig's
             (p + d5 + s, p + s[:-1], 0, "15=5D15=", 1, 1),
             good]
    bad = {1, 3, 4, 5, 6, 7, 8}
    with pytest.raises(Exception):
        dev.small_cand_sv_batch(tasks, strict=True)  # the call returns the code
    got = dev.small_cand_sv_batch(tasks)
    want = dev.small_cand_sv_batch([good])[0]
    assert want["status"] == 0 and want["cipos_end"] == 0
    for i, rec in enumerate(got):
        if i in bad:
            assert rec["status"] == E_INVALID_ARG and all(rec[k] == 0 for k in RANGE_FIELDS), i
        else:
            assert rec == want, i
    # an arena overrun: a text or path that ends one element behind its arena, a length that leaves it alone, an offset that wraps
    rec, n, arena, arena_bytes, cig, cig_words = small_cand_sv_arrays([good] * 6)
    rec[1].contig_off = arena_bytes - rec[1].contig_len + 1
    rec[2].cigar_len = cig_words + 1
    rec[3].ref_off = (1 << 64) - 1
    rec[4].cigar_off = (1 << 64) - 2
    got = dev.small_cand_sv_raw(rec, n, arena, arena_bytes, cig, cig_words)
    assert [r["status"] for r in got] == [0, E_INVALID_ARG, E_INVALID_ARG, E_INVALID_ARG, E_INVALID_ARG, 0]
    assert got[0] == want and got[5] == want
    # ... while one that ends exactly at its arena's end is inside (the last task's texts and path do)
    assert rec[5].contig_off + rec[5].contig_len == arena_bytes and rec[5].cigar_off + rec[5].cigar_len == cig_words


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rank rule through manta_smallsv_select_batch
# ---------------------------------------------------------------------------------------------------------------------
WINDOW = rand_seq(random.Random(7), 150)


def contig_of(score, d=30, **kw):
    """a contig of WINDOW with d bases deleted behind base 20: one candidate segment, variant size d"""
    c = dict(seq=WINDOW[:20] + WINDOW[20 + d:], begin=0, cigar="20=%dD%d=" % (d, len(WINDOW) - 20 - d), score=score, segments=[(1, 1)],
             largest_indel=d)
    c.update(kw)
    return c


def rank_cases():
    """name -> ([contig, ...], (rank1, rank2, rank2_is_best, best))"""
    c, sup = contig_of, lambda n: list(range(n))
    out = {}
    out["contigs-0"] = ([], (-1, -1, 0, -1))
    out["contigs-1"] = ([c(50)], (0, -1, 0, 0))
    out["contigs-2"] = ([c(50), c(60)], (1, 0, 0, 1))
    out["contigs-3"] = ([c(50), c(70), c(60)], (1, 2, 0, 1))
    out["contigs-64"] = ([c(100 + (i * 37) % 64) for i in range(64)], None)
    out["no-candidate"] = ([c(50, candidate=0), c(60, candidate=0, jumped=1)], (-1, -1, 0, -1))
    out["single-candidate"] = ([c(90, candidate=0), c(10), c(95, candidate=0)], (1, -1, 0, 1))
    out["equal-scores"] = ([c(50), c(50), c(50)], (0, 1, 0, 0))  # strict >: the first stays rank 1, the second rank 2
    out["jumped-displaces"] = ([c(100), c(40, jumped=1)], (1, 0, 0, 1))
    out["displaced-overwrites-better-rank2"] = ([c(40, jumped=1), c(100), c(50, jumped=1)], (2, 0, 0, 2))  # rank 2 held 100, holds 40 now
    out["late-lower-keeps-rank2"] = ([c(100), c(90), c(40, jumped=1), c(95)], (2, 0, 0, 2))
    out["displaced-overwrites-better-rank2-only"] = ([c(80), c(90), c(40, jumped=1)], (2, 1, 0, 2))  # (90 took rank 1 first: 80 is lost)
    out["displaced-overwrites"] = ([c(100), c(99), c(40, jumped=1)], (2, 0, 0, 2))  # rank 2 held 99 ... and holds 100 now
    out["not-jumped-after-jumped"] = ([c(40, jumped=1), c(100), c(90)], (0, 1, 0, 0))
    out["not-jumped-after-jumped-ratios-pass"] = ([c(40, jumped=1, support=sup(2)), c(100, d=60, support=sup(40))], (0, 1, 0, 0))
    out["both-jumped-higher-score"] = ([c(40, jumped=1), c(50, jumped=1)], (1, 0, 0, 1))
    out["both-jumped-swap"] = ([c(50, jumped=1, support=sup(5)), c(48, jumped=1, support=sup(7))], (0, 1, 1, 1))
    out["swap-by-support"] = ([c(100, support=sup(10)), c(95, support=sup(13))], (0, 1, 1, 1))
    out["no-swap-support-at-ratio"] = ([c(100, support=sup(10)), c(95, support=sup(12))], (0, 1, 0, 0))  # 12 > 10 * 1.2f is false
    out["swap-by-size"] = ([c(100, d=30, support=sup(10)), c(95, d=34, support=sup(10))], (0, 1, 1, 1))
    out["no-swap-size-at-ratio"] = ([c(100, d=30), c(95, d=33)], (0, 1, 0, 0))  # 33 > 30 * 1.1f is false
    out["score-gate-fails"] = ([c(100, d=30, support=sup(5)), c(90, d=60, support=sup(50))], (0, 1, 0, 0))  # 90 > 100 * 0.9f is false
    out["score-gate-passes"] = ([c(100, d=30, support=sup(5)), c(91, d=60, support=sup(50))], (0, 1, 1, 1))
    out["float-10-9"] = ([c(10, support=sup(1)), c(9, d=60, support=sup(50))], (0, 1, 0, 0))  # true in double
    out["float-20-18"] = ([c(20, support=sup(1)), c(18, d=60, support=sup(50))], (0, 1, 0, 0))
    out["float-30-27"] = ([c(30, support=sup(1)), c(27, d=60, support=sup(50))], (0, 1, 0, 0))
    out["negative-scores"] = ([c(-10, support=sup(1)), c(-12, support=sup(5))], (0, 1, 0, 0))  # -12 > -10 * 0.9f is false
    out["zero-support"] = ([c(100), c(95, support=[3])], (0, 1, 1, 1))  # 1 > 0 * 1.2f
    # support counts whose bits lie in the second qword and among the pseudo-read bits (the last bits of the last qword)
    out["support-second-qword"] = ([c(100, support=[1, 2, 3]), c(95, support=[64, 65, 100, 127])], (0, 1, 1, 1))
    out["support-pseudo-bits"] = ([c(100, support=[0, 63, 64, 120]), c(95, support=[5, 121, 122, 125, 126, 127])], (0, 1, 1, 1))
    out["support-pseudo-bits-short"] = ([c(100, support=[0, 63, 64, 120, 190]), c(95, support=[5, 121, 122, 125, 126, 191])], (0, 1, 0, 0))
    out["swap-takes-rank2-segments"] = ([c(100, support=sup(2)), c(95, d=40, support=sup(9), segments=[(1, 1), (0, 2)])], (0, 1, 1, 1))
    return out


def test_rank_rule_edges(dev, driver):
    cases = rank_cases()
    names = sorted(cases)
    loci = [(WINDOW, cases[n][0]) for n in names]
    recs = check_loci(dev, driver, loci, "rank")
    for name, rec in zip(names, recs):
        if cases[name][1] is not None:
            assert (rec["rank1_contig"], rec["rank2_contig"], rec["rank2_is_best"], rec["best_contig"]) == cases[name][1], name
    by_name = dict(zip(names, recs))
    assert len(by_name["swap-takes-rank2-segments"]["candidates"]) == 2
    assert by_name["contigs-64"]["selected"] == 1


def test_more_than_64_contigs(dev, driver):
    loci = [(WINDOW, [contig_of(50)]), (WINDOW, [contig_of(i) for i in range(65)]), (WINDOW, [contig_of(i) for i in range(64)])]
    with pytest.raises(Exception):
        dev.smallsv_select_batch(loci, strict=True)  # the call returns the code
    recs = dev.smallsv_select_batch(loci)
    assert [r["status"] for r in recs] == [0, E_UNSUPPORTED, 0]
    assert (recs[1]["selected"], recs[1]["best_contig"], recs[1]["candidates"]) == (0, -1, [])
    assert (recs[0]["best_contig"], recs[2]["best_contig"]) == (0, 63) and len(recs[2]["candidates"]) == 1
    # the adapter recomputes such a locus on the host and says so
    host, adapter = loci_text(driver, loci, 0), loci_text(driver, loci, 1)
    assert [a[0] for a in adapter] == [0, E_UNSUPPORTED, 0]
    assert [a[1:] for a in adapter] == [h[1:] for h in host] and adapter[1][4] == 64


def random_loci():
    rng = random.Random(SEED)
    loci = []
    for _ in range(3000):
        items = []
        for _ in range(rng.randint(1, 10)):
            n_sup = rng.choice([0, 1, 5, 10, 11, 12, 13, 20])
            items.append(contig_of(rng.randint(85, 100), d=rng.choice([30, 32, 33, 34, 40]), candidate=int(rng.random() < 0.45),
                                   jumped=int(rng.random() < 0.08), support=sorted(rng.sample(range(128), n_sup))))
        loci.append((WINDOW, items))
    return loci


def test_random_sweep(dev, driver):
    """With SEED the plain-Python restatement sorts the 3 000 loci into: none 382, single 682, kept 792, support 509, size 173,
    jumped 462 (printed below; each class must hold at least 50)."""
    loci = random_loci()
    classes = {}
    for _, items in loci:
        why = py_select(items)["why"]
        classes[why] = classes.get(why, 0) + 1
    print("classes:", sorted(classes.items()))
    assert set(classes) == {"none", "single", "kept", "support", "size", "jumped"}
    assert min(classes.values()) >= 50, classes
    check_loci(dev, driver, loci, "sweep")


# ---------------------------------------------------------------------------------------------------------------------
# 3. per-item failures and call failures
# ---------------------------------------------------------------------------------------------------------------------
def test_per_item_failures(dev, driver):
    c = contig_of
    clean = [(WINDOW, [c(50), c(60)]), (WINDOW, [c(40), c(90)]), (WINDOW, [c(10)]), (WINDOW, [c(70, support=[1, 2]), c(69, support=[1, 2, 3])]),
             (WINDOW, [c(20), c(20)])]
    want = dev.smallsv_select_batch(clean, strict=True)
    for key, code in (("status", E_DEVICE_FAULT), ("status", E_UNSUPPORTED), ("qc_status", E_UNSUPPORTED), ("qc_status", E_INVALID_ARG)):
        loci = [(w, list(items)) for w, items in clean]
        loci[1] = (WINDOW, [c(40), dict(c(90), **{key: code})])  # (the failed contig is the one that would have won)
        loci[3] = (WINDOW, [dict(c(70), **{key: code}), c(69)])
        with pytest.raises(Exception):
            dev.smallsv_select_batch(loci, strict=True)  # the call returns the code
        got = dev.smallsv_select_batch(loci)
        assert [r["status"] for r in got] == [0, code, 0, code, 0], key
        for l in (1, 3):  # left undecided
            assert (got[l]["selected"], got[l]["best_contig"], got[l]["rank1_contig"], got[l]["candidates"]) == (0, -1, -1, [])
        for l in (0, 2, 4):
            assert got[l] == want[l], (key, l)
    # a contig that is no candidate still fails its locus: the locus is not decided on part of its contigs
    got = dev.smallsv_select_batch([(WINDOW, [c(50), dict(c(60), candidate=0, status=E_DEVICE_FAULT)]), (WINDOW, [c(5)])])
    assert [r["status"] for r in got] == [E_DEVICE_FAULT, 0]


def test_invalid_loci(dev):
    """what the chosen contig's walk finds: a segment index outside the path, a reference span that leaves the window, a read length
    that differs from the contig's -- and what the call finds before it: a path, segment list, bitset or text outside its arena"""
    from manta_amd._capi import smallsv_select_arrays
    c = contig_of
    good = (WINDOW, [c(50), c(60)])
    want = dev.smallsv_select_batch([good], strict=True)[0]
    loci = [good,
            (WINDOW, [c(50), c(60, segments=[(1, 1), (2, 3)])]),            # a segment index past the path
            (WINDOW, [c(50, segments=[(5, 5)]), c(60)]),                    # ... of a contig that is not chosen: not walked
            (WINDOW, [c(50), c(60, begin=1)]),                              # the reference span leaves the window
            (WINDOW[:-1], [c(50), c(60)]),
            (WINDOW, [c(50), dict(c(60), seq=c(60)["seq"] + "A")]),         # the read length differs from the contig's
            good]
    got = dev.smallsv_select_batch(loci)
    assert [r["status"] for r in got] == [0, E_INVALID_ARG, 0, E_INVALID_ARG, E_INVALID_ARG, E_INVALID_ARG, 0]
    assert got[0] == want and got[6] == want and got[2] == want
    for l in (1, 3, 4, 5):
        assert (got[l]["selected"], got[l]["best_contig"], got[l]["candidates"]) == (0, -1, [])
    # arenas: every contig of the last locus is made to leave one arena in turn; its locus fails, the others do not
    base = [good, (WINDOW, [c(50), c(60)]), good]

    def attempt(change):
        a = smallsv_select_arrays(base)
        change(a)
        return [r["status"] for r in dev.smallsv_select_raw(**a)][:3]

    def put(obj, field, value):
        setattr(obj, field, value)

    assert attempt(lambda a: None) == [0, 0, 0]
    assert attempt(lambda a: put(a["aligns"][2].align, "cigar1_off", a["cig_used"] - 2)) == [0, E_INVALID_ARG, 0]
    assert attempt(lambda a: put(a["aligns"][3].align, "cigar1_len", 1 << 31)) == [0, E_INVALID_ARG, 0]
    assert attempt(lambda a: put(a["aligns"][2].align, "cigar1_off", (1 << 64) - 1)) == [0, E_INVALID_ARG, 0]
    assert attempt(lambda a: put(a["qc"][3], "seg_off", a["seg_pairs"])) == [0, E_INVALID_ARG, 0]
    assert attempt(lambda a: put(a["qc"][2], "n_segments", 33)) == [0, E_INVALID_ARG, 0]
    assert attempt(lambda a: put(a["contigs"][3], "support_off", a["bits_used"])) == [0, E_INVALID_ARG, 0]
    assert attempt(lambda a: put(a["contigs"][2], "seq_off", a["seq_used"] - 3)) == [0, E_INVALID_ARG, 0]
    # (the last contig's text, path and pair end exactly at their arenas' ends: inside)
    a = smallsv_select_arrays(base)
    assert a["contigs"][5].seq_off + a["contigs"][5].seq_len == a["seq_used"] and a["qc"][5].seg_off + a["qc"][5].n_segments == a["seg_pairs"]
    assert a["aligns"][5].align.cigar1_off + a["aligns"][5].align.cigar1_len == a["cig_used"]


def test_call_failures_write_nothing(dev):
    from manta_amd._capi import MantaError, SmallCandSv, SmallSvBatch, SmallSvSelect, smallsv_select_arrays
    from oracle_lib import asm_opts
    c = contig_of
    loci = [(WINDOW, [c(50), c(60, segments=[(1, 1), (1, 1)])]), (WINDOW, [c(5)])]  # three candidates
    a = smallsv_select_arrays(loci)

    def attempt(code, **kw):
        ls, cs = (SmallSvSelect * 2)(), (SmallCandSv * 64)()
        ctypes.memset(ls, 0xA5, ctypes.sizeof(ls))
        ctypes.memset(cs, 0xA5, ctypes.sizeof(cs))
        with pytest.raises(MantaError) as e:
            dev.smallsv_select_raw(locus_out=ls, cand_out=cs, **dict(a, **kw))
        assert e.value.code == code
        assert bytes(ls) == b"\xa5" * ctypes.sizeof(ls) and bytes(cs) == b"\xa5" * ctypes.sizeof(cs)

    attempt(E_CAPACITY, cand_cap=2)   # a too-small candidate arena
    attempt(E_CAPACITY, cand_cap=0)
    off = a["ref_off"].copy()
    off[1], off[2] = off[2], off[1]
    attempt(E_INVALID_ARG, ref_off=off)  # windows that are not in order
    got = dev.smallsv_select_raw(cand_cap=3, **a)  # ... and the same inputs are fine with room for exactly three
    assert [(r["status"], len(r["candidates"])) for r in got] == [(0, 2), (0, 1)]
    # the stage needs QC
    pipe = SmallSvBatch(dev, asm_opts(minWordLength=31), [2, -8, -24, -1, -1, 0], -100)
    with pytest.raises(MantaError) as e:
        pipe.set_select(True)
    assert e.value.code == E_INVALID_ARG
    pipe.set_select(False)  # switching it off is always fine
    pipe.set_qc(FILTER, 30)
    pipe.set_select(True)
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. staged opt-in
# ---------------------------------------------------------------------------------------------------------------------
def test_staged_opt_in(dev, driver):
    from manta_amd._capi import SmallSvBatch
    from oracle_lib import asm_opts
    from synth import config2_batch
    opts, sc, min_indel = asm_opts(minWordLength=31), [2, -8, -24, -1, -1, 0], 30
    batch = config2_batch(8, seed=4242)  # deletions / insertions of 10..60 bases: some reach the minimum, some do not
    refs, ref_off = batch[3], batch[4]

    def downloads(pipe, with_select):
        res = pipe.download()
        raw, used = pipe.raw, pipe.raw_used
        qc = pipe.download_qc()
        raw_qc = pipe.raw_qc
        sel = pipe.download_select() if with_select else None
        if not with_select:
            with pytest.raises(Exception):
                pipe.download_select()
        return res, raw, used, qc, raw_qc, sel

    pipe = SmallSvBatch(dev, opts, sc, -100)
    pipe.set_qc(FILTER, min_indel)
    pipe.set_select(True)
    pipe.upload_packed(*batch)
    pipe.run()
    res, raw, used, qc, raw_qc, sel = downloads(pipe, True)
    loci, contigs, aligns, seq, bits, cig = raw
    assert len(sel) == 8 and all(r["status"] == 0 for r in sel)
    # ... equal the stand-alone call on the downloaded output, handed back as it came
    alone = dev.smallsv_select_raw(loci, contigs, aligns, raw_qc[0], raw_qc[1], raw_qc[2], seq, used[0], cig, used[2], bits, used[1], refs, ref_off,
                                   strict=True)
    assert alone == sel
    # ... and the host restatement on the same alignments and QC results
    items, i = [], 0
    for l, r in enumerate(res):
        window = refs[int(ref_off[l]):int(ref_off[l + 1])].tobytes().decode()
        cs = []
        for c, a in zip(r["contigs"], r["aligns"]):
            assert a["status"] == 0 and qc[i]["status"] == 0
            cs.append(dict(seq=c["seq"], begin=a["begin1"], cigar=a["cigar1"], score=a["score"], jumped=a["is_jumped"], support=c["support"],
                           candidate=qc[i]["is_candidate"], segments=qc[i]["segments"], largest_indel=qc[i]["largest_indel"]))
            i += 1
        items.append((window, cs))
    host = loci_text(driver, items, 0)
    for l, (rec, h) in enumerate(zip(sel, host)):
        assert (0, rec["rank1_contig"], rec["rank2_contig"], rec["rank2_is_best"], rec["best_contig"], [strip(c) for c in rec["candidates"]]) == h, l
        want = py_select(items[l][1])
        assert (rec["rank1_contig"], rec["rank2_contig"], rec["best_contig"]) == (want["rank1"], want["rank2"], want["best"]), l
    n_sel = sum(r["selected"] for r in sel)
    assert n_sel >= 2 and len(sel) - n_sel >= 1, [r["selected"] for r in sel]  # (a condition on the sample: change the sample, not this line)
    assert sum(len(r["candidates"]) for r in sel) >= n_sel
    # a second run on the same object with the stage switched off, and a pipeline that never set it: the same downloads, byte for byte
    pipe.set_select(False)
    pipe.run()
    second = downloads(pipe, False)
    pipe.close()
    never = SmallSvBatch(dev, opts, sc, -100)
    never.set_qc(FILTER, min_indel)
    never.upload_packed(*batch)
    never.run()
    third = downloads(never, False)
    never.close()
    for other_run in (second, third):
        res2, raw2, used2, qc2, raw_qc2, _ = other_run
        assert res2 == res and qc2 == qc and used2 == used and raw_qc2[2] == raw_qc[2]
        for a, b in zip(raw, raw2):
            assert bytes(a) == bytes(b)
        assert bytes(raw_qc2[0]) == bytes(raw_qc[0]) and bytes(raw_qc2[1]) == bytes(raw_qc[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the refiner's switch
# ---------------------------------------------------------------------------------------------------------------------
def run_batched(driver, cases, device_qc, device_select):
    """one getCandidateAssemblyDataBatch call on a refiner with the two switches given -> (canonical text, counters)"""
    from refiner_loci import RefineInput, fill
    keep, arr = [], (RefineInput * len(cases))()
    for i, c in enumerate(cases):
        fill(arr[i], c, keep)
    buf = ctypes.create_string_buffer(1 << 24)
    counters = (ctypes.c_uint64 * 4)()
    driver.lib.mine_get_candidate_assembly_data_batch_small_select(arr, len(cases), int(device_qc), int(device_select), counters, buf, len(buf))
    return buf.value.decode(), dict(zip(("small", "device", "fallback", "qc_fallback"), list(counters)))


@pytest.fixture(scope="module")
def ref_refiner():
    from refiner_loci import RefinerLib
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"])
    return RefinerLib(REF_SO, "ref") if os.path.exists(REF_SO) else None


def test_refiner_switch(driver, ref_refiner):
    """The scenario calls cannot hold a locus that falls back: the assembler returns at most maxAssemblyCount (10) contigs per locus, far
    from 64, and no contig of these piles reaches the QC kernel's 32 indel runs.  The fallback counter is therefore asserted to be 0
    here; the fallback itself is pinned below the refiner: a locus of 65 contigs through the adapter that recomputes it on the host
    (test_more_than_64_contigs), a locus with a failed QC record through the records the refiner reads (test_per_item_failures)."""
    from refiner_loci import complex_case, large_insertion_case
    from test_refiner import scenario_cases
    sample = [(name, c) for name, c in scenario_cases(606) if name.startswith("complex") or name == "large-insertion"][::2]
    rng = random.Random(SEED)
    sample += [("del-two-haps", complex_case(rng, "del", two_haps=True)), ("delins", complex_case(rng, "delins")),
               ("ins", complex_case(rng, "ins")), ("li", large_insertion_case(rng))]
    n_sv = n_device = 0
    for name, c in sample:
        off, off_n = run_batched(driver, [c], False, False)
        on, on_n = run_batched(driver, [c], True, True)
        assert not off.startswith("EXCEPTION"), off[:200]
        assert on == off, name
        if ref_refiner is not None:
            assert on == (ref_refiner.run_multi([c], True) if ref_refiner.multi else ref_refiner.run(c)), name
        assert (off_n["device"], off_n["fallback"]) == (0, 0), name
        assert on_n["small"] == off_n["small"], name
        assert on_n["device"] == on_n["small"] and on_n["fallback"] == 0 and on_n["qc_fallback"] == 0, name
        n_sv += off.count("\nsv ")
        n_device += on_n["device"]
    print("refined candidates:", n_sv, "loci the device decided:", n_device, "of", len(sample), "calls")
    assert n_sv >= 5      # the sample does nominate candidates through the small-SV path
    assert n_device >= 5  # ... and with the switch on their ranking and ranges were the device's
    # the switch alone does nothing: it is effective only together with the QC switch
    alone, alone_n = run_batched(driver, [sample[0][1]], False, True)
    assert alone == run_batched(driver, [sample[0][1]], False, False)[0] and (alone_n["device"], alone_n["fallback"]) == (0, 0)
    # two small-SV loci of one chromosome and pile in one call
    first = complex_case(random.Random(SEED + 1), "del")
    second = dict(first, begin=[b + 2 for b in first["begin"]], end=[e - 2 for e in first["end"]])
    off, off_n = run_batched(driver, [first, second], True, False)
    on, on_n = run_batched(driver, [first, second], True, True)
    assert not off.startswith("EXCEPTION") and on == off
    assert (off_n["small"], off_n["device"], off_n["fallback"]) == (2, 0, 0)
    assert (on_n["small"], on_n["device"], on_n["fallback"]) == (2, 2, 0)


def set_small_cand_sv(driver, window, offset, contig, begin, cigar, first, last, use_device):
    buf = ctypes.create_string_buffer(1 << 16)
    driver.lib.mine_set_small_cand_sv(window.encode(), int(offset), contig.encode(), int(begin), cigar.encode(), int(first), int(last),
                                      int(use_device), buf, len(buf))
    return buf.value.decode()


def test_nonzero_cipos_begin_throws_the_same(driver):
    """The aligners place an indel at its leftmost position, so no scenario pile yields a candidate that slides to the left; the
    exception is pinned on setSmallCandSV as the refiner calls it with the switch off (the host's ranges) and on (the device record's)."""
    tasks = edge_tasks()
    n_throw = n_fine = 0
    for name in ("left-1-del", "left-5-ins", "left-64-del", "left-5-del-to-start", "left-5-insdel-to-start", "left-first-index-del",
                 "tandem-del-mid", "homopolymer-ins-right", "homopolymer-ins", "tandem-del", "kind-multi", "kind-del", "begin-pos"):
        ref, contig, begin, cigar, first, last = tasks[name]
        off = set_small_cand_sv(driver, ref, 1000, contig, begin, cigar, first, last, 0)
        on = set_small_cand_sv(driver, ref, 1000, contig, begin, cigar, first, last, 1)
        assert on == off, name
        want = py_ranges(ref, contig, begin, cigar, first, last)
        if want["cipos_begin"] != 0:
            assert off.startswith("EXCEPTION") and "Attempting to convert alignment to sv candidate. contigSize: %d segments: [%d,%d]" % (
                len(contig), first, last) in off, (name, off)
            n_throw += 1
        else:
            assert off.startswith("bp1 %d %d bp2 %d %d " % (1000 + want["ref_begin"] - 1, 1000 + want["ref_begin"] + want["cipos_end"],
                                                             1000 + want["ref_end"], 1000 + want["ref_end"] + want["cipos_end"] + 1)), (name, off)
            n_fine += 1
    assert n_throw >= 6 and n_fine >= 5
