"""Small-SV scheduling in the epilogue of the LDS contig kernels (asm_contig.hpp: scheduleEpilogue; smallsv_trim.hpp holds the one copy
of the 10-mer trim): the wave that emitted a locus' contigs trims and files them at once, and smallsv_schedule_kernel takes only the
loci that are left.  Every result must equal the oracle and the run with MANTA_AMD_NO_FUSED_SCHEDULE (everything through
smallsv_schedule_kernel), record for record and in manta_smallsv_output_sizes; MANTA_AMD_DEBUG's routing line shows which way the
loci went."""
import ctypes
import re

import numpy as np
import pytest

from manta_amd._capi import BatchOutput, SmallSvBatch, pack_loci, small_sv_text
from oracle_lib import asm_opts
from synth import small_indel_locus

SC = [2, -8, -24, -1, -1, 0]
C2_CUTS = (100, 100, 800, 800)  # synth.config2_batch
O31 = dict(minWordLength=31)


def _routing(err):
    """(loci scheduled in the epilogue, loci left to smallsv_schedule_kernel, loci the LDS kernels handed to the general kernel), summed
    over the runs of the captured output"""
    m = re.findall(r"smallsv schedule: (\d+) loci in the contig kernels' epilogue, (\d+) left to smallsv_schedule_kernel", err)
    assert m, err[-2000:]
    h = re.findall(r"LDS assembler pipeline: .*?, (\d+) handed to the general kernel \(\+ (\d+) outside", err)
    return sum(int(a) for a, _ in m), sum(int(b) for _, b in m), sum(int(a) + int(b) for a, b in h)


def _sizes(b):
    sizes = [ctypes.c_uint64(0) for _ in range(4)]
    b.lib._check(b.lib.lib.manta_smallsv_output_sizes(b.h, *[ctypes.byref(x) for x in sizes]))
    return [int(x.value) for x in sizes]


def _staged(lib, capfd, opts, loci, cuts):
    """one staged run -> (decoded loci, output sizes, routing)"""
    b = SmallSvBatch(lib, opts, SC, -100)
    b.upload([l[0] for l in loci], [l[1] for l in loci], cuts)
    capfd.readouterr()
    b.run()
    sizes = _sizes(b)
    res = b.download(strict=False)  # (a contig the trim refuses carries its status; the call then reports -5)
    routing = _routing(capfd.readouterr().err)
    assert routing[0] + routing[1] == len(loci)
    b.close()
    return res, sizes, routing


def _pack(loci, cuts):
    bases, read_off, begin = pack_loci([l[0] for l in loci])
    refs = np.frombuffer(b"".join(l[1] for l in loci) + b"\0", dtype=np.uint8)
    ref_off = np.zeros(len(loci) + 1, dtype=np.uint64)
    np.cumsum([len(l[1]) for l in loci], out=ref_off[1:])
    return bases, read_off, begin, refs, ref_off, np.ascontiguousarray(np.array(cuts, dtype=np.int32).reshape(len(loci), 4))


def _batch(lib, capfd, opts, loci, cuts, block, refuse=None):
    """one whole-batch call; `refuse`: a locus whose word length lies outside the envelope (its block is refused, -5)"""
    batch = _pack(loci, cuts)
    out = BatchOutput(lib, "smallsv", len(loci), opts[8], 1 << 21, 1 << 17, 1 << 20)
    min_wl = max_wl = None
    if refuse is not None:
        min_wl, max_wl = np.full(len(loci), opts[0], dtype=np.uint32), np.full(len(loci), opts[1], dtype=np.uint32)
        max_wl[refuse] = 200
    capfd.readouterr()
    lib.smallsv_batch(opts, SC, -100, batch, out, min_wl=min_wl, max_wl=max_wl, block_loci=block, n_workers=2, strict=False)
    routing = _routing(capfd.readouterr().err)
    return out.decode(np.diff(batch[2])), [int(u.value) for u in out.used], routing


def _both_ways(lib, oracle, monkeypatch, capfd, opts, loci, cuts, staged=True, block=0, refuse=None):
    """fused and unfused runs of one batch; both equal the oracle and each other in every returned field.  -> the fused run's routing"""
    cuts = [cuts] * len(loci) if isinstance(cuts[0], int) else cuts
    run = (lambda: _staged(lib, capfd, opts, loci, cuts)) if staged else (lambda: _batch(lib, capfd, opts, loci, cuts, block, refuse))
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    monkeypatch.delenv("MANTA_AMD_NO_FUSED_SCHEDULE", raising=False)
    res, sizes, routing = run()
    monkeypatch.setenv("MANTA_AMD_NO_FUSED_SCHEDULE", "1")
    res0, sizes0, routing0 = run()
    monkeypatch.delenv("MANTA_AMD_NO_FUSED_SCHEDULE")
    assert routing0[0] == 0 and routing0[1] == routing[0] + routing[1]
    assert res == res0  # contigs, adjusted cuts, statuses, scores and CIGARs of every slot
    assert sizes == sizes0
    for (reads, ref), c, r in zip(loci, cuts, res):
        if refuse is not None and r["status"] != 0:
            assert r["status"] == -5
            continue
        if any(len(x["seq"]) < 10 for x in r["contigs"]):
            # (no oracle for a contig shorter than a 10-mer: the reference's own substr throws there.  The trim refuses the contig)
            assert all(a["status"] != 0 for a, x in zip(r["aligns"], r["contigs"]) if len(x["seq"]) < 10)
            continue
        assert small_sv_text(r) == oracle.small_sv_locus(opts, SC, -100, reads, ref, tuple(c))
    return res, routing


# ---- small batch: more config-2 loci than a pool holds at once (test_contig_pool.py), staged and whole-batch ----
def _config2_loci(n=28):
    return [small_indel_locus(900 + i, sub_rate=0.003 * (i % 4)) for i in range(n)]


def _plain_loci(n=8):
    """config-2 loci without substitutions: acyclic graphs, no repeat hit -- no kernel hands one of them on"""
    return [small_indel_locus(900 + 4 * i, sub_rate=0.0) for i in range(n)]


def check_small_batch(lib, oracle, monkeypatch, capfd):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    loci, opts = _config2_loci(), asm_opts(**O31)
    # (the loci with substitutions hold a few whose graph has a cycle or a repeat hit: the LDS kernels hand those to the general kernel)
    res, (fused, left, handed) = _both_ways(lib, oracle, monkeypatch, capfd, opts, loci, C2_CUTS)
    assert fused > 12 and left == handed  # every locus the contig kernels finished was scheduled there
    resB, (fusedB, leftB, handedB) = _both_ways(lib, oracle, monkeypatch, capfd, opts, loci, C2_CUTS, staged=False, block=12)
    assert (fusedB, leftB) == (fused, left)
    assert [small_sv_text(r) for r in resB] == [small_sv_text(r) for r in res]
    # plain config-2 loci that no kernel hands on: nothing for smallsv_schedule_kernel, on the pool and on the single-wave contig_kernel
    plain = _plain_loci()
    resP, routingP = _both_ways(lib, oracle, monkeypatch, capfd, opts, plain, C2_CUTS)
    assert routingP == (len(plain), 0, 0)
    monkeypatch.setenv("MANTA_AMD_NO_CONTIG_POOL", "1")
    res1, routing1 = _both_ways(lib, oracle, monkeypatch, capfd, opts, plain, C2_CUTS)
    assert routing1 == (len(plain), 0, 0) and res1 == resP


def test_emulated_fused_schedule_small_batch(emu, oracle, monkeypatch, capfd):
    check_small_batch(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_fused_schedule_small_batch(gpu, oracle, monkeypatch, capfd):
    check_small_batch(gpu, oracle, monkeypatch, capfd)


# ---- edges of the trim, each next to ordinary loci in the same call ----
def _edge_loci():
    """(loci, cuts per locus): config-2 loci whose windows and cuts drive the trim to its edges"""
    base = [small_indel_locus(700 + i) for i in range(6)]
    other = small_indel_locus(799)[1]
    loci = [base[0],
            (base[1][0], other),  # window in which no 10-mer of the contig hits: both scans run dry
            base[2], base[3], base[4], base[5],
            (base[0][0][:2], base[0][1]),  # two reads: no contig
            ([], base[1][1])]  # no reads
    cuts = [C2_CUTS,
            C2_CUTS,
            (100, 100, 50, 800),  # maxLeadingCut below leadingCut: empty forward range
            (100, 100, 800, 50),  # maxTrailingCut: empty backward range
            (100, 100, 50, 50),  # both ranges empty: the trim keeps the cuts
            (0, 0, 1800, 1800),  # the whole window searchable
            C2_CUTS, C2_CUTS]
    return loci, cuts


def check_edges(lib, oracle, monkeypatch, capfd):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    loci, cuts = _edge_loci()
    res, routing = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(**O31), loci, cuts)
    # (the graphs of piles of 0-2 reads take a pool share below the trim's 4 KB table: the epilogue leaves those two loci alone)
    assert routing == (6, 2, 0)
    # loci without a contig ON the fused route: minUnusedReads 60 ends selectContigs before its first contig on piles of 50 reads
    # (:750), whose graphs are as large as any -- the epilogue runs with no contig and writes the records of the empty slots
    few = [small_indel_locus(600 + i, n_reads=(80 if i % 2 == 0 else 50)) for i in range(5)]
    resZ, routingZ = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(minUnusedReads=60, **O31), few, C2_CUTS)
    assert routingZ == (5, 0, 0) and [len(r["contigs"]) for r in resZ] == [1, 0, 1, 0, 1]
    # every slot filled: maxAssemblyCount 1 and 2 on loci that yield two contigs and more
    for count in (1, 2):
        resN, (fusedN, _, _) = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(maxAssemblyCount=count, **O31), loci[:6], cuts[:6])
        assert fusedN == 6 and any(len(r["contigs"]) == count for r in resN)


def test_emulated_fused_schedule_edges(emu, oracle, monkeypatch, capfd):
    check_edges(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_fused_schedule_edges(gpu, oracle, monkeypatch, capfd):
    check_edges(gpu, oracle, monkeypatch, capfd)


def _short_contig_loci():
    """word length 6 over reads of 8 bases: contigs shorter than a 10-mer (status 2), next to contigs of 12 bases, in one locus too"""
    rng = np.random.default_rng(5)
    ref = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=200))
    a, b = ref[40:48], ref[120:132]
    return [([a] * 6, ref), ([b] * 6, ref), ([a] * 5 + [b] * 5, ref)]


def check_short_contigs(lib, oracle, monkeypatch, capfd):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    opts = asm_opts(minWordLength=6, maxWordLength=6, minContigLength=6)
    # On the pool a graph this small takes a share below the trim's 4 KB table, so its locus is smallsv_schedule_kernel's; the
    # single-wave contig_kernel owns its launch's whole LDS class, and there the epilogue itself meets the short contigs.
    res, routing = _both_ways(lib, oracle, monkeypatch, capfd, opts, _short_contig_loci(), (10, 10, 80, 80))
    assert routing == (0, 3, 0)
    monkeypatch.setenv("MANTA_AMD_NO_CONTIG_POOL", "1")
    res1, routing1 = _both_ways(lib, oracle, monkeypatch, capfd, opts, _short_contig_loci(), (10, 10, 80, 80))
    assert routing1 == (3, 0, 0) and res1 == res
    assert [[len(c["seq"]) for c in r["contigs"]] for r in res1] == [[8], [12], [12, 8]]
    assert [[a["status"] == 0 for a in r["aligns"]] for r in res1] == [[False], [True], [True, False]]


def test_emulated_fused_schedule_short_contigs(emu, oracle, monkeypatch, capfd):
    check_short_contigs(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_fused_schedule_short_contigs(gpu, oracle, monkeypatch, capfd):
    check_short_contigs(gpu, oracle, monkeypatch, capfd)


# ---- loci the epilogue must leave to smallsv_schedule_kernel, next to loci it takes ----
def _mixed_loci():
    good = [small_indel_locus(600 + i) for i in range(4)]
    long_contig = small_indel_locus(650, n_reads=40, read_len=300, ref_len=1800)  # contig beyond 512 bases: its table does not fit 4 KB
    wide_window = small_indel_locus(651, ref_len=24000)  # window of 24 KB: the texts do not fit the locus' LDS share
    return good[:2] + [long_contig] + good[2:] + [wide_window]


def check_mixed(lib, oracle, monkeypatch, capfd):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    loci  = _mixed_loci()
    cuts  = [C2_CUTS] * 5 + [(11000, 11000, 800, 800)]
    res, (fused, left, handed) = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(**O31), loci, cuts)
    assert any(len(c["seq"]) > 512 for c in res[2]["contigs"])
    assert fused == 4 and left == 2 and handed == 0  # (both were emitted by the contig kernels and left alone by their epilogue)
    # the whole-batch call, block by block; then with a failed locus among good ones (its block is refused, the other is served)
    _, (fusedB, leftB, _) = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(**O31), loci, cuts, staged=False, block=3)
    assert fusedB == 4 and leftB == 2
    resR, (fusedR, leftR, _) = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(**O31), loci, cuts, staged=False, block=3, refuse=4)
    assert [r["status"] for r in resR] == [0, 0, 0, -5, -5, -5] and (fusedR, leftR) == (2, 1)
    # the general path: everything through smallsv_schedule_kernel
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "general")
    resG, (fusedG, leftG, _) = _both_ways(lib, oracle, monkeypatch, capfd, asm_opts(**O31), loci[:3], cuts[:3])
    assert fusedG == 0 and leftG == 3 and resG == res[:3]


def test_emulated_fused_schedule_mixed_routes(emu, oracle, monkeypatch, capfd):
    check_mixed(emu, oracle, monkeypatch, capfd)


@pytest.mark.gpu
def test_gpu_fused_schedule_mixed_routes(gpu, oracle, monkeypatch, capfd):
    check_mixed(gpu, oracle, monkeypatch, capfd)
