"""The assembler's LDS pipeline at every capacity edge and tie (asm_edge_cases.py builds the piles and proves what they are).

For every bound that decides whether a locus stays on the pipeline (graph_kernel -> contig_kernel / contig_pool_kernel, and the big
class graph_big_kernel -> contig_big_kernel) or goes to assemble_kernel through the device-side punt list: the tightest pile that
still stays and its neighbour one over.  Both must equal the oracle (which equals the unmodified reference on the same piles: CPU
tier), and the ROUTE must be the expected one -- read from MANTA_AMD_DEBUG's pipeline line on both tiers, from manta_emu_fast_stats
and MANTA_EMU_PUNT_TRACE on the emulator as well.  A case whose route differs is a failure, not an expectation to adapt.

    edge (constant)                          stays                                   one over
    words (LG_MAX_NODES)                     1843                                    1844 -> general kernel
    successor / predecessor overflow tables  32 words with 3 (or 4) links            33 -> general kernel
    sibling table (LG_SIB_CAP)               16 pairs of sibling start words         15 pairs + 1 triple -> general kernel
    walk length (CK_MAX_EXT)                 1020 extension steps                    1021 -> general kernel ("contig too long")
    pile bytes in LDS (LG_BUDGET)            3008 padded dwords                      3012 -> the BIG class (host and device share lgPileFits)
    reads + 2 x maxAssemblyCount             128                                     129 -> the big class
    contig LDS class 0 (20 480 bytes)        ckNeed 20 480: contig_pool_kernel       20 496: contig_kernel's second class
    big: words / tables / siblings           7168 / 128 / 32                         -> general kernel (words / side tables / class)
    big: read sets                           1280 | 1281 (device memory) .. 1984     1985 -> general kernel (table / set pool)
    big: walk, pile                          1020 steps; cw + 2 = 3600               1021 (by contig_big_kernel); 3601 outside the envelope
Bounds that cannot be reached because another binds first (LG_MAX_PILE, contig class 1 from above, LGL_DYN_DWORDS, LGL_STAGE_BYTES,
contig_big_kernel's classes) are listed with the reason next to their constants in asm_edge_cases.py.

Neither tier runs a pile twice: the oracle's text is computed once per pile and shared."""
import ctypes
import os
import re
import subprocess
import sys
from functools import lru_cache

import pytest

import asm_edge_cases as E
from manta_amd._capi import assembly_text

K_SWEEP = (21, 32, 33, 64, 65, 128)  # 32|33 and 64|65: the edges of the graph_kernel<2>, <4> and <8> instantiations


@pytest.fixture(autouse=True)
def _fast_path(monkeypatch):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    monkeypatch.setenv("MANTA_EMU_PUNT_TRACE", "1")


tables = lru_cache(None)(E.small_table_cases)
capacities = lru_cache(None)(E.small_capacity_cases)
bigs = lru_cache(None)(E.big_cases)
_WANT = {}


def want(oracle, case):
    if case.name not in _WANT:
        _WANT[case.name] = oracle.assemble(case.opts, case.reads)
    return _WANT[case.name]


def fast_stats(emu):
    st = (ctypes.c_ulonglong * 8)()
    emu.lib.manta_emu_fast_stats(st)
    return st[0]  # loci that finished on the pipeline since the last call


BIG_FIELDS = ("envelope", "table", "words", "slab", "repeat", "contig", "pseudo", "rounds")


def pipeline_line(err):
    m = re.search(r"LDS assembler pipeline: (\d+) \+ (\d+) \(big class\) loci, (\d+) handed to the general kernel \(\+ (\d+) outside its envelope\)", err)
    assert m, err[-2000:]
    return tuple(int(x) for x in m.groups())


def big_line(err):
    m = re.search(r"big class, \d+ word-length rounds; handed back: (\d+) envelope, (\d+) table / set pool, (\d+) words / side tables / class, (\d+) slab arena, "
                  r"(\d+) by repeat_big_kernel, (\d+) by contig_big_kernel, (\d+) pseudo arena, (\d+) out of rounds", err)
    assert m, err[-2000:]
    return dict(zip(BIG_FIELDS, (int(x) for x in m.groups())))


def pool_line(err):
    m = re.search(r"contig_pool_kernel: (\d+) shares taken.*largest first\):((?: \d+)+)", err)
    assert m, err[-2000:]
    return int(m.group(1)), sum(int(x) for x in m.group(2).split())


ROUTES = {"small": (1, 0, 0, 0), "small-punt": (1, 0, 1, 0), "big": (0, 1, 0, 0), "big-punt": (0, 1, 1, 0), "outside": (1, 0, 0, 1)}
COMPANION = ["ACGTTGCAAGGCTTACCGGATTACCATGAC"] * 4  # next to a pile the host keeps off the pipeline: without a locus on it there is no debug line


def check_case(lib, oracle, case, capfd, emu):
    loci = [case.reads] + ([COMPANION] if case.route == "outside" else [])
    capfd.readouterr()
    if emu:
        fast_stats(lib)
    res = lib.assemble_batch(case.opts, loci)
    err = capfd.readouterr().err
    assert res[0]["status"] == 0 and assembly_text(res[0]) == want(oracle, case), case
    assert pipeline_line(err) == ROUTES[case.route], (case, case.m, err[-1500:])
    punted = case.route.endswith("punt")
    if case.big and case.route != "outside":
        got = big_line(err)
        assert got == {f: int(punted and f == case.counter) for f in BIG_FIELDS}, (case, got)
    if hasattr(case, "pooled"):  # contig LDS class: contig_pool_kernel takes class 0 only
        assert pool_line(err) == ((1, 1) if case.pooled else (0, 0)), (case, case.need, err[-1500:])
    if emu:
        assert fast_stats(lib) == len(loci) - (1 if punted or case.route == "outside" else 0), case
        if punted and case.trace:
            assert case.trace in err, (case, err[-1500:])
        if not punted:
            assert "punts locus" not in err, (case, err[-1500:])


def check_cases(lib, oracle, cases, capfd, emu):
    for c in cases:
        check_case(lib, oracle, c, capfd, emu)


# ---- the orders (no capacity involved) ----
def order_cases():
    out = []
    reads, segs = E.saturated_count_pile(31, 21)
    out.append(E.Case("saturated_counts", 21, reads, "small", minContigLength=21, maxAssemblyCount=2))
    out[-1].segs = segs
    for k in (21, 31, 32, 33, 64, 65, 128):
        out.append(E.Case("ties_k%d" % k, k, E.tie_pile(32, k), "small", minContigLength=k, maxAssemblyCount=2))
    # the big class has its own sort (byte passes over the whole key) and its own 4-bit count field
    reads, segs = E.saturated_count_pile(31, 21, big=True)
    out.append(E.Case("saturated_counts_big", 21, reads, "big", big=True, minContigLength=21, maxAssemblyCount=2))
    out[-1].segs = segs
    for k in (21, 33):
        out.append(E.Case("ties_big_k%d" % k, k, E.tie_pile(32, k, pad_reads=60 if k == 21 else 90), "big", big=True, minContigLength=k, maxAssemblyCount=2))
    out.append(E.Case("tag_pressure", 21, E.tag_pressure_pile(33, 21), "small"))
    # a threshold equal to a count and one above it.  Isolated segments: a contig is its segment and its support is the segment's count.
    #   minCoverage t / minSupportReads t: the segments with counts t + 1 and t come out (by support), the one with t - 1 does not
    #   minUnusedReads t: counts t-1, t, t+1 -- after two contigs t - 1 reads are unused, one less than the threshold: two contigs;
    #                     counts t, t+1, t+2 -- after two contigs t reads are unused, EQUAL to the threshold: the third comes out as well
    # (maxAssemblyCount 4, not 2: a cut after two contigs would give these answers whatever the thresholds did)
    for t in (1, 2, 3):
        for field, shift in (("minCoverage", 0), ("minSupportReads", 0), ("minUnusedReads", 0), ("minUnusedReads", 1)):
            reads, segs = E.threshold_pile(34 + t + 10 * shift, 21, t, shift)
            out.append(E.Case("%s%d%s" % (field, t, "_equal" if shift else ""), 21, reads, "small", minContigLength=21, maxAssemblyCount=4,
                              **dict(dict(minSupportReads=1, minUnusedReads=1), **{field: t})))
            out[-1].expect = [segs[c] for c in ((t + 2, t + 1, t) if shift else (t + 1, t))]
    return out


orders = lru_cache(None)(order_cases)


def check_orders(lib, oracle, capfd, emu):
    check_cases(lib, oracle, orders(), capfd, emu)
    # the piles say what they were built to say: the two contigs of the saturated pile are the 40- and the 18-count segments, in that order
    for sat in [c for c in orders() if c.name.startswith("saturated")]:
        seqs = re.findall(r"seq=([ACGT]+)", want(oracle, sat))
        assert seqs == [sat.segs[40], sat.segs[18]], seqs
    # ... and each threshold separates the count it equals from the count one below it
    for c in orders():
        if hasattr(c, "expect"):
            assert re.findall(r"seq=([ACGT]+)", want(oracle, c)) == c.expect, c


# ---- the neighbour on the same persistent workgroup: what a punted locus leaves in LDS (side-table counters, a full table, the cycle
# flag) must not reach the next locus.  One call, over-cap and at-cap piles alternating, in three orders ----
def neighbour_piles(big):
    if big:
        by = {c.name: c for c in bigs()}
        over = [by[n] for n in ("big_words7169", "big_sovf129", "big_povf129", "big_sib33", "big_sets1985", "big_walk1021")]
        at = [by[n] for n in ("big_words7168", "big_sovf128", "big_povf128", "big_sib32", "big_sets1984", "big_walk1020")]
        return over, at
    by = {c.name: c for c in tables(21) + capacities()}
    over = [by[n] for n in ("sovf33_k21", "povf33_k21", "sib33_k21", "words1844", "walk1021", "walk1021_mid")]
    over += [E.Case("sovf33_b", 21, E.sovf_pile(41, 21, 33), "small-punt", over=["sovf"]), E.Case("povf33_b", 21, E.povf_pile(42, 21, 33), "small-punt", over=["povf"])]
    at = [by[n] for n in ("sovf32_k21", "povf32_k21", "sib32_k21", "words1843", "walk1020", "walk1020_mid", "sovf32_fourway_k21", "ckclass789")]
    return over, at


def check_neighbours(lib, oracle, capfd, big, n_loci, cross_pairs=False):
    """The host queues the loci of a call most expensive first (reads x bases, ties in locus order): the order of the call decides the
    locus numbers, the order on a workgroup follows the cost -- mostly an over-cap pile right before its own at-cap neighbour.
    cross_pairs (emulator, where one workgroup takes the whole queue in that order): further calls of two loci, every at-cap pile with
    the over-cap pile of the next family, so that it also runs behind (or, where it is the dearer one, ahead of) a different table's
    leftovers."""
    over, at = neighbour_piles(big)
    assert len({tuple(c.opts) for c in over + at}) == 1
    seqs = [[c for pair in zip(over, at) for c in pair],            # over, at, over, at ...
            [c for pair in zip(at, reversed(over)) for c in pair],  # at, over ... with the partners changed
            [c for i in range(0, len(over), 2) for c in over[i:i + 2] + at[i:i + 2]]]  # two over, two at
    assert n_loci >= len(seqs[0]) and all(sorted(q, key=id) == sorted(over + at, key=id) for q in seqs)  # every pile, in every order
    batches = [[cyc[i % len(cyc)] for i in range(n_loci)] for cyc in seqs]
    if cross_pairs:
        batches += [[over[(i + 1) % len(over)], a] for i, a in enumerate(at)]
    for o, loci in enumerate(batches):
        n_loci = len(loci)
        capfd.readouterr()
        res = lib.assemble_batch(over[0].opts, [c.reads for c in loci])
        err = capfd.readouterr().err
        n_over = sum(1 for c in loci if c.route.endswith("punt"))
        assert pipeline_line(err) == ((0, n_loci, n_over, 0) if big else (n_loci, 0, n_over, 0)), (o, err[-1500:])
        if big:
            got, exp = big_line(err), {f: 0 for f in BIG_FIELDS}
            for c in loci:
                if c.route.endswith("punt"):
                    exp[c.counter] += 1
            assert got == exp
        for i, (c, r) in enumerate(zip(loci, res)):
            assert r["status"] == 0 and assembly_text(r) == want(oracle, c), (o, i, c)


def device_cus(lib):
    return int(re.search(r"(\d+) CUs", lib.device_name()).group(1))


# =====================================================  CPU tier  =====================================================
def test_constants_match_the_sources():
    h = E.header_constants()
    for name in ("LG_MAX_NODES", "LG_MAX_READS", "LG_OVF_CAP", "LG_SIB_CAP", "LG_MAX_PILE", "LG_BUDGET", "CK_MAX_EXT", "LGL_MAX_NODES", "LGL_MAX_READS",
                 "LGL_OVF_CAP", "LGL_MAX_PILE", "LGL_POOL_CAP", "LGL_POOL_OVF"):
        assert h[name] == getattr(E, name), name
    # the derived ones, from the LDS maps: LG_OFF_DYN = 512 + 512 + 256 + 1024 + 1024 waves + (4 + 16 + 2 + 2 + 4 + 1) x slots
    assert E.LG_OFF_DYN == 2304 + 1024 * h["LG_WAVES"] + 29 * h["LG_SLOTS"]
    assert E.CK_OFF_RECS == 768 + 8 * h["LG_SIB_CAP"] + 16 * h["LG_OVF_CAP"]
    assert E.LGL_STAGE_BYTES == 32 * h["LGL_POOL_CAP"] + 4 * h["LGL_SLOTS"]
    lgl_off_dyn = ((5632 + 8 * h["LG_SIB_CAP"] + 16 * h["LGL_OVF_CAP"] + 528 + 255) & ~255) + 1024 * h["LGL_WAVES"] + 32 * h["LGL_POOL_CAP"] + 9 * h["LGL_SLOTS"]
    assert E.LGL_DYN_DWORDS == (h["LGL_BUDGET"] - lgl_off_dyn) // 4
    src = open(os.path.join(E.CSRC, "api_internal.hpp")).read()
    assert "kClassDefault[LG_CLASSES] = {20480, 54272, 0, 0}" in src and "kClassBig[LGL_CLASSES] = {81920, 163840}" in src


def test_unreachable_bounds_are_unreachable():
    """the reasons given next to the constants, as arithmetic"""
    # LG_MAX_PILE: the smallest padded sum of a pile with cw + 2 = LG_MAX_PILE + 1 (one read: mw is smallest) is already over the LDS line
    cw = E.LG_MAX_PILE - 1
    bases = 16 * (cw - 1)  # one read of cw - 1 code dwords
    mw = (bases + 31) // 32 + 1
    assert ((cw + 2 + 3) & ~3) + ((mw + 2 + 3) & ~3) > E.LG_PILE_DWORDS
    assert E.ck_need(E.LG_MAX_NODES, E.LG_MAX_NODES, True) == 45776 < E.CK_CLASS_BYTES[1]
    assert E.ck_need(E.LG_MAX_NODES, 0, False) < E.CK_CLASS_BYTES[1]
    assert E.ck_need(E.LGL_MAX_NODES, E.LGL_POOL_CAP + E.LGL_POOL_OVF, True, big=True) == 132096 < E.LGL_CLASS_BYTES[1]
    assert E.ck_need(E.LGL_MAX_NODES, 0, False, big=True) < E.LGL_CLASS_BYTES[1]
    assert 16 * E.LGL_MAX_PILE + 64 <= E.LGL_STAGE_BYTES
    assert (E.LGL_MAX_PILE + 2) + (E.LGL_MAX_PILE // 2 + 236 + 2) + 6 <= E.LGL_DYN_DWORDS


def test_restatement_matches_the_reference_on_edge_piles(oracle, reflib):
    """what makes the oracle a reference here: the unmodified sources give the same text on every pile of this module"""
    cases = capacities() + bigs() + orders() + neighbour_piles(False)[0][-2:]
    for k in K_SWEEP:
        cases = cases + tables(k)
    for c in cases:
        assert want(oracle, c) == reflib.assemble(c.opts, c.reads), c


@pytest.mark.parametrize("k", K_SWEEP)
def test_emulated_side_tables_at_and_over_their_caps(emu, oracle, capfd, k):
    check_cases(emu, oracle, tables(k), capfd, True)


def test_emulated_small_class_capacities(emu, oracle, capfd):
    check_cases(emu, oracle, capacities(), capfd, True)


def check_host_classification(lib, oracle, capfd, emu):
    """a pile the small class' pack() refuses for its size (3012 padded dwords; cw + 2 is inside LG_MAX_PILE) is not marked for the small
    class by the host either: the big class takes it, not assemble_kernel"""
    c = [x for x in capacities() if x.name == "pile3012"][0]
    assert c.m["cw"] + 2 <= E.LG_MAX_PILE and c.m["reads"] + 2 * c.mac <= E.LG_MAX_READS
    capfd.readouterr()
    res = lib.assemble_batch(c.opts, [c.reads])
    err = capfd.readouterr().err
    assert "0 + 1 (big class) loci, 0 handed to the general kernel" in err, err[-1500:]
    assert assembly_text(res[0]) == want(oracle, c)


def test_emulated_host_classification_is_the_device_envelope(emu, oracle, capfd):
    check_host_classification(emu, oracle, capfd, True)


def test_emulated_big_class_bounds(emu, oracle, capfd):
    check_cases(emu, oracle, bigs(), capfd, True)


def test_emulated_seed_orders_the_records_cannot_carry(emu, oracle, capfd):
    check_orders(emu, oracle, capfd, True)


def test_emulated_neighbours_on_one_workgroup(emu, oracle, capfd):
    """the emulator has 2 CUs: graph_kernel runs min(loci, 4) workgroups, graph_big_kernel min(loci, 2), one after the other -- the first
    takes every locus of the queue, so any batch larger than that puts every pile behind a neighbour on the same workgroup.  Every pile
    of both classes, in the three orders, then the cross-family pairs (check_neighbours)"""
    check_neighbours(emu, oracle, capfd, False, 16, cross_pairs=True)
    check_neighbours(emu, oracle, capfd, True, 12, cross_pairs=True)


def test_emulated_edges_do_not_depend_on_lane_order(emu, oracle):
    """the side tables are filled through atomic_add tickets by all lanes: their entry order changes with the lane order
    (MANTA_EMU_LANE_ORDER=reverse, read once per process: a fresh child), the result and the route must not"""
    code = ("import os, sys\n"
            "sys.path.insert(0, %r)\n"
            "import conftest, test_asm_edges as t\n"
            "from oracle_lib import OracleLib\n"
            "from manta_amd._capi import Lib\n"
            "os.environ['MANTA_AMD_ASM_PATH'] = 'fast'\n"
            "lib, oracle = Lib(path=%r), OracleLib()\n"
            "for c in t.tables(21) + t.tables(33) + t.capacities() + t.orders()[:5]:\n"
            "    t.fast_stats(lib)\n"
            "    r = lib.assemble_batch(c.opts, [c.reads])[0]\n"
            "    assert t.assembly_text(r) == t.want(oracle, c), c\n"
            "    assert t.fast_stats(lib) == (0 if c.route.endswith('punt') else 1), c\n"
            "print('lane-order-ok')\n") % (os.path.dirname(os.path.abspath(__file__)), emu.path)
    env = dict(os.environ, MANTA_EMU_LANE_ORDER="reverse")
    env.pop("MANTA_AMD_DEBUG", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert "lane-order-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# =====================================================  device tier  =====================================================
@pytest.mark.gpu
@pytest.mark.parametrize("k", K_SWEEP)
def test_gpu_side_tables_at_and_over_their_caps(gpu, oracle, capfd, k):
    check_cases(gpu, oracle, tables(k), capfd, False)


@pytest.mark.gpu
def test_gpu_small_class_capacities(gpu, oracle, capfd):
    check_cases(gpu, oracle, capacities(), capfd, False)


@pytest.mark.gpu
def test_gpu_host_classification_is_the_device_envelope(gpu, oracle, capfd):
    check_host_classification(gpu, oracle, capfd, False)


@pytest.mark.gpu
def test_gpu_big_class_bounds(gpu, oracle, capfd):
    check_cases(gpu, oracle, bigs(), capfd, False)


@pytest.mark.gpu
def test_gpu_seed_orders_the_records_cannot_carry(gpu, oracle, capfd):
    check_orders(gpu, oracle, capfd, False)


@pytest.mark.gpu
def test_gpu_neighbours_on_one_workgroup_small_class(gpu, oracle, capfd):
    """graph_kernel's grid is min(loci, 2 x CUs) persistent workgroups: four times as many loci, so every workgroup takes several"""
    check_neighbours(gpu, oracle, capfd, False, 4 * 2 * device_cus(gpu))


@pytest.mark.gpu
def test_gpu_neighbours_on_one_workgroup_big_class(gpu, oracle, capfd):
    """graph_big_kernel's grid is min(loci, CUs): four loci per CU"""
    check_neighbours(gpu, oracle, capfd, True, 4 * device_cus(gpu))
