"""align_pair_kernel<E> with tagged states and the start tracking off the per-step path: the shapes at which those two can go wrong.

The packed pair aligner keeps every state as value * 8 | (7 - state) and tracks the traceback start with wave-uniform conditions only
(csrc/align_pair.hpp).  What that leaves to get wrong, each checked here against the oracle through align_batch:

  * the column that owns q = Q: every column of a lane (eQ = 0 .. E - 1) on the first and on the last lane a bucket can put it (lQ);
  * which rows count: the two tasks of a wave differ by 1 and by 200 rows, a 1-row task sits beside a 300-row one (in either half),
    and row counts straddle the 64-step period of the reference reload (63, 64, 65, 127, 128, 129);
  * where the start comes from: q = Q in an early row with equal values in later rows (the earlier row wins), off the edge in the last row
    at q < Q, the q = 0 off-edge candidate, and two halves of one wave that take their starts from different kinds;
  * floor-adjacent cells: the all-mismatch diagonal of a full query under the tightest eligible `mismatch` score set, in either half;
  * buckets of 1 .. 5 tasks (the odd last task runs against itself);
  * align_pair_multi_kernel, which inlines all six widths and is built for three waves per SIMD: config-2 loci through smallsv_batch
    against the oracle's small_sv_locus, once with the default grid and once with MANTA_AMD_ALIGN_WAVES_PER_CU=1, where the few waves
    each take many pairs and cross from one bucket's slots into the next.

Back-to-back pairs of one wave in a single sweep (a chain) are not built; the cases that only a chain could break (a chain's length, its
end at a bucket boundary, a second run with the chain switched off) have nothing to run against and are not here.

Neighbours of a batch share a wave (task 2 i in the low halves, 2 i + 1 in the high ones); every batch also runs reversed, so each case
sits in both halves.  The emulator tier runs E in (1, 2, 6) and leaves out batches of more than EMU_CELLS DP cells
(tests/test_align_margin.py already takes it through the full-size diagonals); every test states which widths must have run there.  The
device tier runs every width and every batch; its small-SV loci have the full config-2 shape, the emulator's the same generator's
loci at a third of the size."""
import os
import re

import numpy as np
import pytest

import align_margin_cases as mc
from manta_amd._capi import SmallSvBatch, align_text, small_sv_text
from oracle_lib import asm_opts
from synth import config2_batch, small_indel_locus, unpack_locus

KIND = mc.LARGE_INDEL
EMU_CELLS = 45000
PRODUCTION = mc.PRODUCTION["small-sv"]


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def dev(request):
    return request.getfixturevalue(request.param)


def on_emulator(dev):
    return "emu" in os.path.basename(dev.path)


def widths(dev):
    return mc.CPU_E[KIND] if on_emulator(dev) else mc.PACKED_E[KIND]


def mismatch_set(E):
    s = next(s for s in mc.score_sets(KIND, E) if s["name"] == "mismatch")
    assert s["eligible"] and s["slack"] > 0
    return s["sc"], s["extra"]


def _rnd(rs, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rs.randint(0, len(a), size=n)].tobytes() if n else b""


def planted(rs, Q, G):
    """a random reference of G rows and a query of Q bases: a copy of a window where the reference can hold one, with one substitution"""
    ref = _rnd(rs, G)
    if G >= Q:
        at = int(rs.randint(0, G - Q + 1))
        q = bytearray(ref[at:at + Q])
        q[int(rs.randint(0, Q))] = b"ACGT"[int(rs.randint(0, 4))]
        return bytes(q), ref
    return _rnd(rs, Q), ref


def early_tie(Q, G):
    """A^Q against A^G, G > Q: rows Q .. G all hold the same best value at q = Q; the reference keeps the first"""
    return b"A" * Q, b"A" * G


def off_edge_last_row(rs, Q, G, hang):
    """the query's first Q - hang bases are the reference's last ones, the rest hangs off its end: the start lies in the last row at q < Q"""
    ref = _rnd(rs, G, b"ACG")
    w = min(Q - hang, G)
    return _rnd(rs, Q - hang - w, b"T") + ref[G - w:] + b"T" * hang, ref


def all_off_edge(Q, G):
    """nothing matches and a mismatch costs more than leaving the edge: the q = 0 candidate of the last row wins"""
    return b"T" * Q, b"C" * G


_orc = {}


def run(dev, oracle, capfd, E, sc, extra, probs):
    """one align_batch call in the given order and one reversed; -> False if the emulator's budget left it out"""
    assert all(mc.pick_e(len(q)) == E for q, _ in probs), [len(q) for q, _ in probs]
    if on_emulator(dev) and sum(len(q) * len(r) for q, r in probs) > EMU_CELLS:
        return False
    for order in (probs, probs[::-1]):
        capfd.readouterr()
        res = dev.align_batch(KIND, sc, extra, [(q, r, None) for q, r in order])
        err = capfd.readouterr().err
        assert re.findall(r"manta_amd: align_pair_kernel<(\d+)>", err) == [str(E)], err
        for (q, r), got in zip(order, res):
            key = (tuple(sc), extra, q, r)
            if key not in _orc:
                _orc[key] = oracle.align(KIND, sc, extra, q, r, None)
            assert got["status"] == 0
            assert align_text(KIND, got) == _orc[key], (E, sc, extra, len(q), len(r))
    return True


def check_ran(dev, got, full, emu):
    """got: {E: batches that ran}.  The device runs `full` batches at every width; the emulator what its budget admits: emu = {E: batches}"""
    want = emu if on_emulator(dev) else {E: full for E in widths(dev)}
    assert got == want, (got, want)


def q_last_lane(E):
    """Q = 64 E - k: column Q on the last lane, in each of its columns"""
    return [64 * E - k for k in range(E)]


def q_first_lane(E):
    """the shortest queries of the bucket: column Q on the first lane the bucket can put it, in each of its columns"""
    lo = 64 * mc.e_prev(E) + 1
    return [lo + k for k in range(E)]


@pytest.mark.parametrize("scores", ["production", "mismatch"])
def test_every_column_owns_q_on_the_first_and_last_lane(dev, oracle, capfd, monkeypatch, scores):
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    got = {}
    for E in widths(dev):
        sc, extra = PRODUCTION if scores == "production" else mismatch_set(E)
        rs = np.random.RandomState(4100 + E)
        qs = q_first_lane(E) + q_last_lane(E)
        if E == 1:
            qs = [1, 2, 63, 64]
        # short references (the sweep is mostly fill and drain), then the two longest queries against references that hold them
        probs = [planted(rs, Q, 5 + i) for i, Q in enumerate(qs)]
        got[E] = run(dev, oracle, capfd, E, sc, extra, probs) + run(dev, oracle, capfd, E, sc, extra, [planted(rs, 64 * E, 64 * E + 9), planted(rs, 64 * E - 1, 64 * E + 8)])
    check_ran(dev, got, 2, {1: 2, 2: 2, 6: 0})


ROWS = [(300, 1), (1, 300), (1, 1, 1, 1), (63, 64, 65), (127, 128, 129), (70, 71), (30, 230)]
EMU_ROWS_E6 = {(1, 1, 1, 1): 1}  # E = 6 on the emulator: 322 columns x the rows of every other tuple are over its budget


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: "-".join(map(str, r)))
def test_neighbours_with_unequal_row_counts(dev, oracle, capfd, monkeypatch, rows):
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    got = {}
    for E in widths(dev):
        rs = np.random.RandomState(4200 + E)
        Q = 64 * mc.e_prev(E) + 2
        probs = [planted(rs, Q + (i % 2), G) for i, G in enumerate(rows)]
        got[E] = int(run(dev, oracle, capfd, E, *PRODUCTION, probs))
    check_ran(dev, got, 1, {1: 1, 2: 1, 6: EMU_ROWS_E6.get(rows, 0)})


def test_traceback_start_kinds(dev, oracle, capfd, monkeypatch):
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    got = {}
    for E in widths(dev):
        rs = np.random.RandomState(4300 + E)
        lo = 64 * mc.e_prev(E) + 1
        tie = early_tie(lo, lo + 40)
        hang = off_edge_last_row(rs, lo + 3, 50, 7)
        q0 = all_off_edge(lo + 1, 3)
        mid = planted(rs, lo + 2, lo + 30)
        sc, extra = PRODUCTION
        for key, prob in (("tie", tie), ("hang", hang), ("q0", q0)):
            text = oracle.align(KIND, sc, extra, prob[0], prob[1], None)
            begin, cigar = int(re.search(r"begin\d?=(\d+)", text).group(1)), text.rstrip().rsplit("cigar=", 1)[1]
            if key == "tie":  # the first of the 41 equal placements
                assert begin == 0 and cigar == "%d=" % len(prob[0]), text
            elif key == "hang":  # the alignment ends on the reference's last base with the query's tail soft-clipped
                assert cigar.endswith("S"), text
            else:  # nothing aligned
                assert re.fullmatch(r"\d+S", cigar) or "=" not in cigar, text
        # each kind beside itself, and the halves of one wave taking their starts from different kinds
        got[E] = sum(run(dev, oracle, capfd, E, sc, extra, probs)
                     for probs in ([tie, tie], [hang, hang], [q0, q0], [tie, hang], [hang, q0], [q0, tie], [mid, tie, hang, q0, mid]))
    check_ran(dev, got, 7, {1: 7, 2: 7, 6: 3})


def test_floor_cells_in_either_half(dev, oracle, capfd, monkeypatch):
    """the all-mismatch diagonal of a full query at the tightest eligible `mismatch` set, beside a short task and beside itself"""
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    got = {}
    for E in widths(dev):
        sc, extra = mismatch_set(E)
        Q = 64 * E
        diag = (b"A" * Q, b"C" * Q)
        short = (b"A" * (64 * mc.e_prev(E) + 1), b"C")
        got[E] = run(dev, oracle, capfd, E, sc, extra, [diag, short]) + run(dev, oracle, capfd, E, sc, extra, [diag, diag])
    check_ran(dev, got, 2, {1: 2, 2: 2, 6: 0})  # (E = 6 on the emulator: test_align_margin.py's `mis` group runs that diagonal)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_bucket_sizes(dev, oracle, capfd, monkeypatch, n):
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    for E in widths(dev):
        rs = np.random.RandomState(4400 + 10 * E + n)
        lo = 64 * mc.e_prev(E) + 1
        probs = [planted(rs, lo + i, 9 + 3 * i) for i in range(n)]
        assert run(dev, oracle, capfd, E, *PRODUCTION, probs)


# ------------------------------------------------------------------------------------------------------ smallsv_batch: align_pair_multi_kernel

SMALLSV_SC = [2, -8, -24, -1, -1, 0]
_loci = {}


def smallsv_case(dev, oracle):
    """-> (upload arguments, packed ?, assembler options, the oracle's text per locus), computed once per tier.  Device: 32 config-2 loci.
    Emulator: 24 loci of the config-2 shape at a third of the size with three read lengths, so that their contigs (about 50, 95 and 175
    bases) fill three packed buckets -- a single bucket would run align_pair_kernel<E>, not the multi-width kernel"""
    emu_tier = on_emulator(dev)
    if emu_tier not in _loci:
        if emu_tier:
            opts, cuts = asm_opts(minWordLength=21, maxWordLength=31), (40, 40, 200, 200)
            loci = [small_indel_locus(4600 + i, n_reads=24, read_len=(36, 60, 100)[i % 3], ref_len=600) for i in range(24)]
            args = ([l[0] for l in loci], [l[1] for l in loci], [cuts] * len(loci))
            want = [oracle.small_sv_locus(opts, SMALLSV_SC, -100, reads, ref, cuts) for reads, ref in loci]
        else:
            opts, args = asm_opts(minWordLength=31), config2_batch(32, seed=4600)
            want = [oracle.small_sv_locus(opts, SMALLSV_SC, -100, *unpack_locus(args, l)) for l in range(32)]
        _loci[emu_tier] = (args, not emu_tier, opts, want)
    return _loci[emu_tier]


@pytest.mark.parametrize("waves_per_cu", [None, "1"], ids=["default-grid", "one-wave-per-cu"])
def test_smallsv_batch_runs_the_multi_width_kernel(dev, oracle, capfd, monkeypatch, waves_per_cu):
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    if waves_per_cu:
        monkeypatch.setenv("MANTA_AMD_ALIGN_WAVES_PER_CU", waves_per_cu)
    args, packed, opts, want = smallsv_case(dev, oracle)
    pipe = SmallSvBatch(dev, opts, SMALLSV_SC, -100)
    (pipe.upload_packed if packed else pipe.upload)(*args)
    capfd.readouterr()
    pipe.run()
    res = pipe.download()
    err = capfd.readouterr().err
    m = re.search(r"manta_amd: align_pair_multi_kernel: (\d+) waves over (\d+) packed buckets", err)
    assert m, err[-2000:]
    print(m.group(0), "-", sum(len(r["contigs"]) for r in res), "contigs")
    assert int(m.group(2)) >= (3 if on_emulator(dev) else 2)
    if waves_per_cu and on_emulator(dev):  # (the device has more CUs than this batch has pairs)
        assert int(m.group(1)) < int(m.group(2))  # fewer waves than buckets: a wave goes on from one bucket's pairs to the next's
    assert len(res) == len(want) and sum(len(r["contigs"]) for r in res) >= len(res)
    for l, r in enumerate(res):
        assert small_sv_text(r) == want[l], l
