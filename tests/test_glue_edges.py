"""The glue between the assembler and the aligners at its edges, on constructed loci (tests/glue_cases.py): the contig, the place of its
first and last 10-mer hit and the distance from a junction to a cut edge are the test's choice.

Small SV (smallsv_trim.hpp: scheduleContig and its callers): every family against oracle.small_sv_locus, on four routes -- the pool's
epilogue, contig_kernel's epilogue (MANTA_AMD_NO_CONTIG_POOL), smallsv_schedule_kernel alone (MANTA_AMD_NO_FUSED_SCHEDULE; _both_ways of
test_fused_schedule.py runs it beside every fused run and compares every returned field), and the general path.  The first assertion
per locus: the device's contigs are the constructed ones, in order.  The second: the oracle's own lead + trail < len(ref).

Spanning (pipeline_kernels.hpp: spanning_schedule_kernel / spanning_realign_kernel): against oracle_locus of test_spanning_pipeline.py,
contigs by equality.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import glue_cases as gc
from manta_amd._capi import MantaError, SpanningBatch
from oracle_lib import asm_opts
from test_fused_schedule import SC, _both_ways
from glue_cases import SPAN_SC
from test_spanning_pipeline import ALN, oracle_locus

ROUTES = ("pool", "contig_kernel", "general")


def _route(monkeypatch, route):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "general" if route == "general" else "fast")
    if route == "contig_kernel":
        monkeypatch.setenv("MANTA_AMD_NO_CONTIG_POOL", "1")
    else:
        monkeypatch.delenv("MANTA_AMD_NO_CONTIG_POOL", raising=False)


def run_family(lib, oracle, monkeypatch, capfd, loci, opts, routes=ROUTES, fused=None):
    """the family's loci in one call per route (each fused and unfused, against the oracle: _both_ways) -> {route: (results, routing)}.
    fused: how many loci the epilogue of contig_pool_kernel ("pool") and of contig_kernel must take (None: not this family's matter)"""
    out = {}
    for route in routes:
        _route(monkeypatch, route)
        res, routing = _both_ways(lib, oracle, monkeypatch, capfd, opts, [l.pair for l in loci], [l.cuts for l in loci])
        for l, r in zip(loci, res):
            assert [c["seq"].encode("latin-1") for c in r["contigs"]] == l.contigs[:opts[8]], (route, l.name)
            want = oracle.small_sv_locus(opts, SC, -100, l.reads, l.ref, l.cuts)
            trims = [(int(a), int(b)) for a, b in re.findall(r"^align \d+ lead=(-?\d+) trail=(-?\d+)", want, flags=re.M)]
            assert all(a + b < len(l.ref) for a, b in trims), (l.name, trims)
            # the hits lie where the case put them, and every slot is aligned
            assert [(a["lead"], a["trail"]) for a in r["aligns"]] == l.trims[:opts[8]], (route, l.name)
            assert all(a["status"] == 0 for a in r["aligns"]), (route, l.name)
        if route == "general":
            assert routing[0] == 0 and routing[1] == len(loci)
        elif fused is not None:
            assert routing == (fused, len(loci) - fused, 0), (route, routing)
        out[route] = (res, routing)
    first = out[routes[0]][0]
    assert all(out[r][0] == first for r in routes[1:])
    monkeypatch.delenv("MANTA_AMD_NO_CONTIG_POOL", raising=False)
    return out


# ---- the scans ----------------------------------------------------------------------------------------------------------------------
def check_scan_edges(lib, oracle, monkeypatch, capfd):
    for family in (gc.scan_edge_loci, gc.extreme_cut_loci, gc.n_window_loci):
        loci, opts = family()
        run_family(lib, oracle, monkeypatch, capfd, loci, opts, fused=len(loci))  # (both epilogues take every locus: glue_cases.add_ballast)


def test_emulated_trim_scan_edges(emu, oracle, monkeypatch, capfd):
    check_scan_edges(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_trim_scan_edges(gpu, oracle, monkeypatch, capfd):
    check_scan_edges(gpu, oracle, monkeypatch, capfd)


# ---- contig lengths -----------------------------------------------------------------------------------------------------------------
def check_contig_lengths(lib, oracle, monkeypatch, capfd):
    """table-size steps, E-bucket steps, the LDS / global table switch: both epilogues take every locus but the 513-base contig's, which
    they leave to smallsv_schedule_kernel.
      Reads of 1024 / 1025 bases (found: the LDS pipeline's envelope takes them -- contig_pool_kernel and contig_kernel assemble the
    whole read, hand nothing to the general kernel, and leave the locus to smallsv_schedule_kernel and its global table; every route equals
    the oracle)"""
    loci, opts = gc.contig_length_loci()
    run_family(lib, oracle, monkeypatch, capfd, loci, opts, fused=len(loci) - 1)
    alone = [l for l in loci if len(l.contigs[0]) == 513]
    run_family(lib, oracle, monkeypatch, capfd, alone, opts, fused=0)
    below = [l for l in loci if len(l.contigs[0]) == 512]
    run_family(lib, oracle, monkeypatch, capfd, below, opts, fused=1)
    loci, opts = gc.long_contig_loci()
    run_family(lib, oracle, monkeypatch, capfd, loci, opts, fused=0)


def test_emulated_trim_contig_lengths(emu, oracle, monkeypatch, capfd):
    check_contig_lengths(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_trim_contig_lengths(gpu, oracle, monkeypatch, capfd):
    check_contig_lengths(gpu, oracle, monkeypatch, capfd)


# ---- staging ------------------------------------------------------------------------------------------------------------------------
def check_staging(lib, oracle, monkeypatch, capfd):
    loci, opts = gc.staging_alignment_loci()
    fwd = run_family(lib, oracle, monkeypatch, capfd, loci, opts, fused=len(loci))
    rev = run_family(lib, oracle, monkeypatch, capfd, loci[::-1], opts, fused=len(loci))
    assert rev["pool"][0][::-1] == fwd["pool"][0]
    # smallsv_schedule_kernel's own LDS: either side of SCHED_SEQ_BYTES (the piles are small: the pool leaves them all)
    loci, opts = gc.staging_capacity_loci()
    out = run_family(lib, oracle, monkeypatch, capfd, loci, opts)
    assert out["pool"][1][0] == 0
    # the pool's share: its size follows the graph, so the windows sweep across it -- the epilogue takes the short windows and leaves
    # the long ones; contig_kernel's share is the launch's whole LDS class and holds every window of the sweep
    loci, opts = gc.pool_share_loci()
    out = run_family(lib, oracle, monkeypatch, capfd, loci, opts)
    taken = out["pool"][1][0]
    assert 0 < taken < len(loci) and out["pool"][1][2] == 0, out["pool"][1]
    assert out["contig_kernel"][1] == (len(loci), 0, 0), out["contig_kernel"][1]
    # ... and the bracket the coarse sweep found, in 16-base steps (and one base either side of each 16): the step lies inside it
    lo, hi = gc.POOL_SWEEP[taken - 1], gc.POOL_SWEEP[taken]
    fine = sorted(set(list(range(lo, hi + 1, 16)) + [w + d for w in range(lo + 16, hi, 64) for d in (-1, 1)]))
    loci, opts = gc.pool_share_loci(fine, seed0=7000)
    out = run_family(lib, oracle, monkeypatch, capfd, loci, opts)
    assert 0 < out["pool"][1][0] < len(loci) and out["pool"][1][2] == 0, (lo, hi, out["pool"][1])


def test_emulated_trim_staging(emu, oracle, monkeypatch, capfd):
    check_staging(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_trim_staging(gpu, oracle, monkeypatch, capfd):
    check_staging(gpu, oracle, monkeypatch, capfd)


# ---- several contigs per locus, the pending lists -----------------------------------------------------------------------------------
def check_multi_contig(lib, oracle, monkeypatch, capfd):
    loci, opts = gc.multi_contig_loci()
    run_family(lib, oracle, monkeypatch, capfd, loci, opts, fused=len(loci))
    for count in (1, 2):
        o = list(opts)
        o[8] = count
        out = run_family(lib, oracle, monkeypatch, capfd, loci[1:2], o, fused=1)
        assert len(out["pool"][0][0]["contigs"]) == count


def test_emulated_trim_multi_contig(emu, oracle, monkeypatch, capfd):
    check_multi_contig(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_trim_multi_contig(gpu, oracle, monkeypatch, capfd):
    check_multi_contig(gpu, oracle, monkeypatch, capfd)


def check_pending_flush(lib, oracle, monkeypatch, capfd):
    """one wave of smallsv_schedule_kernel files every contig of the run (a pop of 64 loci): its pending lists fill to SCHED_PEND.  The
    runs of short contigs check the counts schedFlush adds up (their buckets pair: bucket_sort_kernel rebuilds the lists); the runs of
    400-base contigs check the lists themselves (glue_cases.pending_loci)"""
    from manta_amd._capi import SmallSvBatch
    sets, opts = gc.pending_loci()
    monkeypatch.setenv("MANTA_AMD_SCHED_CHUNK", "64")
    for loci in sets:
        run_family(lib, oracle, monkeypatch, capfd, loci, opts, routes=("pool",))
        monkeypatch.setenv("MANTA_AMD_NO_FUSED_SCHEDULE", "1")
        b = SmallSvBatch(lib, opts, SC, -100)
        b.upload([l.reads for l in loci], [l.ref for l in loci], [l.cuts for l in loci])
        b.run()
        res = b.download()
        assert b.stats()["n_alignments"] == sum(len(l.contigs) for l in loci)
        assert all(a["status"] == 0 for r in res for a in r["aligns"])
        b.close()
        monkeypatch.delenv("MANTA_AMD_NO_FUSED_SCHEDULE")


def test_emulated_schedule_pending_flush(emu, oracle, monkeypatch, capfd):
    check_pending_flush(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_schedule_pending_flush(gpu, oracle, monkeypatch, capfd):
    check_pending_flush(gpu, oracle, monkeypatch, capfd)


def check_bucket_sort(lib, oracle, monkeypatch, capfd, n):
    from manta_amd._capi import SmallSvBatch
    loci, opts = gc.bucket_sort_loci(n)
    out = run_family(lib, oracle, monkeypatch, capfd, loci, opts, routes=("pool",))
    res = out["pool"][0]
    assert sum(len(r["aligns"]) for r in res) == n
    # aligned exactly once.  n_alignments is the sum of the bucket counts the schedule stage added up: it pins that n tasks were filed.
    # What guards the sorted lists: a slot bucket_sort_kernel dropped keeps its zeroed result record and fails the oracle comparison
    # above, and a list of n entries can hold a slot twice only in place of one it dropped.
    _route(monkeypatch, "pool")
    b = SmallSvBatch(lib, opts, SC, -100)
    b.upload([l.reads for l in loci], [l.ref for l in loci], [l.cuts for l in loci])
    b.run()
    assert b.stats()["n_alignments"] == n
    b.close()


def test_emulated_bucket_sort_130_loci(emu, oracle, monkeypatch, capfd):
    """(the CPU tier's size: 130 loci take 35 s on the emulator, 1100 would take about five minutes; the full 1100 loci, beyond
    bucket_sort_kernel's 16 x 64 shares, run on the device)"""
    check_bucket_sort(emu, oracle, monkeypatch, capfd, 130)


@pytest.mark.gpu
def test_gpu_bucket_sort_1100_loci(gpu, oracle, monkeypatch, capfd):
    check_bucket_sort(gpu, oracle, monkeypatch, capfd, 1100)


# ---- bytes outside ACGTN ------------------------------------------------------------------------------------------------------------
def check_junk(lib, oracle, monkeypatch, capfd, reflib=None):
    """the trim is byte-exact (the reference looks up substrings in a std::set<std::string>).  A pile with such bytes is the general
    path's on every route, and its contigs smallsv_schedule_kernel's: the routing line shows the loci as left."""
    loci, opts, want = gc.issue_reproducer()
    out = run_family(lib, oracle, monkeypatch, capfd, loci, opts)
    for route in ROUTES:
        res, routing = out[route]
        assert [(r["aligns"][0]["lead"], r["aligns"][0]["trail"], r["aligns"][0]["cigar1"]) for r in res] == want, route
        assert routing[0] == 0 and routing[1] == len(loci), route
    loci, opts = gc.junk_loci()
    out = run_family(lib, oracle, monkeypatch, capfd, loci, opts)
    n_junk = sum(1 for l in loci if not l.name.startswith("plain"))
    for route in ROUTES:
        assert out[route][1][1] >= n_junk, route
    if reflib is not None:
        for l in loci:
            assert reflib.small_sv_locus(opts, SC, -100, l.reads, l.ref, l.cuts) == oracle.small_sv_locus(opts, SC, -100, l.reads, l.ref, l.cuts), l.name


def test_emulated_trim_non_acgtn_bytes(emu, oracle, reflib, monkeypatch, capfd):
    check_junk(emu, oracle, monkeypatch, capfd, reflib)


@pytest.mark.gpu
def test_gpu_trim_non_acgtn_bytes(gpu, oracle, monkeypatch, capfd):
    check_junk(gpu, oracle, monkeypatch, capfd)


# ---- spanning -----------------------------------------------------------------------------------------------------------------------
def span_run(lib, loci, opts, strict=True, call_code=None):
    """call_code: the code the download call itself must report (download(strict=True) raises it)"""
    b = SpanningBatch(lib, opts, SPAN_SC, -100)
    b.upload([l.reads for l in loci], [l.ref1 for l in loci], [l.ref2 for l in loci], [l.cuts for l in loci])
    b.run()
    if call_code is not None:
        with pytest.raises(MantaError) as e:
            b.download(strict=True)
        assert e.value.code == call_code
    res = b.download(strict=strict)
    b.close()
    return res


def span_check(oracle, loci, opts, res):
    """every locus against the composed oracle; -> per locus the oracle's records"""
    wants = []
    for l, r in zip(loci, res):
        assert [c["seq"].encode("latin-1") for c in r["contigs"]] == l.contigs, l.name
        text, want = oracle_locus(oracle, opts, l.reads, l.ref1, l.ref2, l.cuts)
        assert [c["seq"] for c in r["contigs"]] == re.findall(r"^contig \d+ seq=(\S+)", text, flags=re.M), l.name
        got = [(a["score"], a["jump_insert_size"], a["jump_range"], a["begin1"], a["cigar1"], a["begin2"], a["cigar2"], a["is_uncut"])
               for a in r["aligns"]]
        assert got == want, l.name
        wants.append(want)
    return wants


def cut_distances(oracle, l, contig):
    """(jumpInsertSize, ref1EndPos - align1EndPos, begin2) of the contig's alignment to the CUT references, from the oracle"""
    a1l, a1t, a2l, a2t = l.cuts
    r1, r2 = l.ref1[a1l:len(l.ref1) - a1t], l.ref2[a2l:len(l.ref2) - a2t]
    m = ALN.match(oracle.align(2, SPAN_SC, -100, contig, r1, r2))
    ref_len = sum(int(n) for n, op in re.findall(r"(\d+)([=XDN])", m.group(5)))
    return int(m.group(2)), (len(r1) - 1) - (int(m.group(4)) + ref_len), int(m.group(6))


SPAN_OPTS = asm_opts(minWordLength=15, maxWordLength=15, minContigLength=15)


def check_realign_thresholds(lib, oracle):
    loci, fired = [], {}
    for ins in (0, 5):
        for e in (3, 4, 5, 6):
            for which, dist in (("end1", (e, 30)), ("begin2", (30, e)), ("both", (e, e))):
                loci.append(gc.span_locus(5000 + len(loci), [dist], [ins], name="%s %d insert %d" % (which, e, ins)))
                loci[-1].key = (which, e, ins)
    res = span_run(lib, loci, SPAN_OPTS)
    wants = span_check(oracle, loci, SPAN_OPTS, res)
    for l, want, r in zip(loci, wants, res):
        which, e, ins = l.key
        size, d1, d2 = cut_distances(oracle, l, l.contigs[0])
        # the construction holds: the oracle's own cut alignment has the junction where the case wants it
        assert size == ins and (d1, d2) == {"end1": (e, 30), "begin2": (30, e), "both": (e, e)}[which], (l.name, size, d1, d2)
        fired[l.key] = want[0][7]
        assert r["aligns"][0]["is_uncut"] == want[0][7]
    for which in ("end1", "begin2", "both"):
        assert [fired[(which, e, 5)] for e in (3, 4, 5, 6)] == [1, 1, 0, 0], which  # fires at 4, not at 5
        assert [fired[(which, e, 0)] for e in (3, 4, 5, 6)] == [0, 0, 0, 0], which  # never without an insertion


def test_emulated_spanning_realign_thresholds(emu, oracle):
    check_realign_thresholds(emu, oracle)


@pytest.mark.gpu
def test_gpu_spanning_realign_thresholds(gpu, oracle):
    check_realign_thresholds(gpu, oracle)


def check_shared_decision(lib, oracle):
    """the first contig that meets the rule zeroes the cuts for itself and for every later contig of the locus"""
    far = ((70, 90), (140, 160))  # (flanks of 40 bases: shorter ones do not pay the jump score; every contig has its own stretch of both windows)
    second = gc.span_locus(5500, [far[0], (4, 40), far[1]], [5, 5, 5], w=300, name="only the second contig fires")
    first = gc.span_locus(5501, [(4, 40), far[0], far[1]], [5, 5, 5], w=300, name="the first contig fires")
    none = gc.span_locus(5502, [far[0], (5, 40), far[1]], [5, 5, 5], w=300, name="no contig fires")
    loci = [second, first, none]
    res = span_run(lib, loci, SPAN_OPTS)
    span_check(oracle, loci, SPAN_OPTS, res)
    for l in loci:
        alone = [cut_distances(oracle, l, c) for c in l.contigs]
        assert [s > 0 and (d1 < 5 or d2 < 5) for s, d1, d2 in alone] == [l is first, l is second, False], l.name  # who fires on its own
    assert [[a["is_uncut"] for a in r["aligns"]] for r in res] == [[0, 1, 1], [1, 1, 1], [0, 0, 0]]
    # contig 0 of `second` keeps its cut alignment and the cuts' offsets
    m = ALN.match(oracle.align(2, SPAN_SC, -100, second.contigs[0], second.ref1[10:300 - 60], second.ref2[60:300 - 10]))
    assert (res[0]["aligns"][0]["begin1"], res[0]["aligns"][0]["begin2"]) == (int(m.group(4)) + 10, int(m.group(6)) + 60)


def test_emulated_spanning_shared_realign_decision(emu, oracle):
    check_shared_decision(emu, oracle)


@pytest.mark.gpu
def test_gpu_spanning_shared_realign_decision(gpu, oracle):
    check_shared_decision(gpu, oracle)


def check_span_buckets(lib, oracle):
    """jump contigs of 64 .. 257 bases in one call; every other one has its junction 4 bases from reference 1's cut edge.  (Flanks of
    about 30 bases -- the contigs of 64 and 65 -- do not pay the jump score of -100: those two are aligned without a jump and cannot
    fire.)  The others are re-aligned: both rounds launch several E buckets"""
    loci = []
    for n, total in enumerate((64, 65, 128, 129, 192, 193, 256, 257)):
        left = total // 2
        right = total - left - 5
        loci.append(gc.span_locus(5600 + n, [(4 if n % 2 else 30, 30)], [5], left=left, right=right, w=400, cuts=(10, 100, 100, 10),
                                  name="jump contig of %d" % total))
        assert len(loci[-1].contigs[0]) == total
    res = span_run(lib, loci, SPAN_OPTS)
    wants = span_check(oracle, loci, SPAN_OPTS, res)
    assert [w[0][7] for w in wants][2:] == [0, 1] * 3


def test_emulated_spanning_e_bucket_steps(emu, oracle):
    check_span_buckets(emu, oracle)


@pytest.mark.gpu
def test_gpu_spanning_e_bucket_steps(gpu, oracle):
    check_span_buckets(gpu, oracle)


def check_empty_windows(lib, oracle):
    """lead + trail equal to and beyond a window's length, for either reference, next to ordinary loci: the slot reports the empty
    sequence (SpanTaskInfo status 6 -> MANTA_E_EMPTY_SEQ, -4), every other locus equals the oracle; a window of one base is aligned"""
    w = 200
    cases = [((100, 100, 60, 10), -4), ((150, 100, 60, 10), -4), ((10, 60, 100, 100), -4), ((10, 60, 120, 130), -4),
             ((100, 99, 60, 10), 0), ((10, 60, 100, 99), 0)]
    loci, status = [], []
    for n, (cuts, st) in enumerate(cases):
        loci.append(gc.span_locus(5700 + n, [(30, 30)], [5], name="ordinary %d" % n))
        status.append(0)
        l = gc.span_locus(5750 + n, [(30, 30)], [5], name="cuts %r" % (cuts,))
        l.cuts = cuts
        loci.append(l)
        status.append(st)
    loci.append(gc.span_locus(5799, [(4, 30)], [5], name="ordinary, re-aligned"))
    status.append(0)
    res = span_run(lib, loci, SPAN_OPTS, strict=False, call_code=-4)
    assert [r["aligns"][0]["status"] for r in res] == status
    ok = [i for i, s in enumerate(status) if s == 0]
    span_check(oracle, [loci[i] for i in ok], SPAN_OPTS, [res[i] for i in ok])
    for i, s in enumerate(status):
        if s != 0:
            assert [c["seq"].encode("latin-1") for c in res[i]["contigs"]] == loci[i].contigs


def test_emulated_spanning_empty_cut_windows(emu, oracle):
    check_empty_windows(emu, oracle)


@pytest.mark.gpu
def test_gpu_spanning_empty_cut_windows(gpu, oracle):
    check_empty_windows(gpu, oracle)


# ---- the early alignment pass (api.cpp: spanningRunImpl) ------------------------------------------------------------------------------
def early_pass_loci():
    """one block: a big-class tandem pile that takes several word lengths (config5_locus(64): test_digests.py pins its n_iterations to 4)
    next to a dozen constructed loci that are final after their one word length, every third of them with its junction 4 bases from a
    cut edge -> (loci as (reads, ref1, ref2, cuts, minWordLength, maxWordLength), the constructed SpanLoci)"""
    from synth import config5_locus
    reads, ref1, ref2, k, kmax = config5_locus(64)
    made = [gc.span_locus(5800 + n, [((4, 30), (30, 4), (30, 30))[n % 3]], [5], name="early %d" % n) for n in range(12)]
    return [(reads, ref1, ref2, (100, 100, 100, 100), k, kmax)] + [(l.reads, l.ref1, l.ref2, l.cuts, 15, 15) for l in made], made


EARLY_OPTS = asm_opts(minWordLength=41, minContigLength=75)  # (test_digests.py; the constructed contigs are 85 bases long)


def early_pass_run(lib):
    """-> per locus (contigs, alignment records), JSON-able"""
    from manta_amd._capi import BatchOutput, pack_spanning
    loci, _ = early_pass_loci()
    batch = pack_spanning([l[0] for l in loci], [l[1] for l in loci], [l[2] for l in loci], [l[3] for l in loci])
    out = BatchOutput(lib, "spanning", len(loci), 10, 8 << 20, 1 << 20, 2 << 20)
    lib.spanning_batch(EARLY_OPTS, SPAN_SC, -100, batch, out, min_wl=np.array([l[4] for l in loci], dtype=np.uint32),
                       max_wl=np.array([l[5] for l in loci], dtype=np.uint32), block_loci=len(loci), n_workers=1)
    res = out.decode(np.diff(batch[2]))
    return [[r["n_iterations"], [c["seq"] for c in r["contigs"]],
             [[a["score"], a["jump_insert_size"], a["jump_range"], a["begin1"], a["cigar1"], a["begin2"], a["cigar2"], a["is_uncut"]] for a in r["aligns"]]]
            for r in res]


def check_early_pass(lib, kind, oracle, monkeypatch, capfd, expect_pass):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    monkeypatch.delenv("MANTA_AMD_EARLY_ALIGN", raising=False)
    capfd.readouterr()
    got = early_pass_run(lib)
    err = capfd.readouterr().err
    loci, made = early_pass_loci()
    assert got[0][0] == 4  # the tandem pile takes several word lengths
    fired = 0
    for (reads, ref1, ref2, cuts, k, kmax), g in zip(loci, got):
        o = list(EARLY_OPTS)
        o[0], o[1] = k, kmax
        text, want = oracle_locus(oracle, o, reads, ref1, ref2, cuts)
        assert g[1] == re.findall(r"^contig \d+ seq=(\S+)", text, flags=re.M)
        assert [tuple(a) for a in g[2]] == want
        fired += sum(a[7] for a in g[2][:1])
    assert [g[1] for g in got[1:]] == [[c.decode() for c in l.contigs] for l in made]
    assert fired >= 8  # two of every three constructed loci are re-aligned
    if expect_pass:
        assert "(early pass)" in err, err[-1500:]
    # the same call without the pass, in a fresh process (the knob is read once): identical results
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MANTA_AMD_EARLY_ALIGN="0", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    env.pop("MANTA_AMD_DEBUG", None)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--early-pass-child", kind], env=env, capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-1500:]
    assert json.loads(child.stdout.strip().splitlines()[-1]) == got
    print("early pass taken:", "(early pass)" in err)


def test_emulated_spanning_early_alignment_pass(emu, oracle, monkeypatch, capfd):
    """(the emulator takes the early pass too: the route is asserted in both tiers)"""
    check_early_pass(emu, "emu", oracle, monkeypatch, capfd, expect_pass=True)


@pytest.mark.gpu
def test_gpu_spanning_early_alignment_pass(gpu, oracle, monkeypatch, capfd):
    check_early_pass(gpu, "gpu", oracle, monkeypatch, capfd, expect_pass=True)


if __name__ == "__main__" and sys.argv[1:2] == ["--early-pass-child"]:
    from manta_amd._capi import Lib
    lib = Lib() if sys.argv[2] == "gpu" else Lib(path=os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libmanta_amd_emu.so"))
    print(json.dumps(early_pass_run(lib)))
