"""Adversarial inputs for the packed 16-bit pair aligners (align_pair_kernel<E>, align_jump_pair_kernel<E>): generators only, no device code.

Three things live here, all plain Python and independent of the library:

  * a restatement of the kernels' eligibility rule (pairEligible / jumpPairEligible: "real" cells can never sink to where sentinel-derived
    cells can climb), with the slack each score set leaves;
  * score sets AT that rule's edge for every packed bucket width E: per shape the eligible set with the smallest positive slack and its
    ineligible neighbour one unit further, next to the unchanged production sets;
  * deterministic sequences that realise the rule's worst cases (all-mismatch diagonals of a full 64 E query, all-match runs, ties between
    an affine gap and the jump state, raw bytes, bucket edges), and the order in which a batch presents them, since neighbours of a bucket
    share a wave (task_ids[2 i] in the low int16 halves, task_ids[2 i + 1] in the high ones).

tests/golden/align_margin_cases.json.xz holds, per case, its spec, a digest of its sequences, the scores and the reference's output;
tests/golden/make_align_margin_golden.py writes it.  Sequences are regenerated here from the spec (numpy's legacy RandomState and Python's
random.Random, both frozen streams); changing anything in this file invalidates the golden file, and the digests say so.
"""
import hashlib
import random

import numpy as np

LARGE_INDEL, JUMP = 1, 2
KESET = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 24, 32)  # bucket widths: a query of Q bases runs with the first E >= ceil(Q / 64) columns per lane
PACKED_E = {LARGE_INDEL: (1, 2, 3, 4, 5, 6), JUMP: (1, 2, 3, 4, 5, 6, 8)}
CPU_E = {LARGE_INDEL: (1, 2, 6), JUMP: (1, 8)}  # what the emulator tier runs (the device tier: tests/test_align_margin.py DEVICE_E)
ROW_LIMIT = 0xfffe  # the longest total reference a packed bucket may hold (a traceback start's row is a 16-bit key)
GROUPS = ("mis", "tie", "mix")
PRODUCTION = {"small-sv": ([2, -8, -24, -1, -1, 0], -100), "spanning": ([2, -8, -12, -1, -1, 0], -100)}

# ---------------------------------------------------------------------------------------------------------------- eligibility, restated


def _neg(x):
    return min(x, 0)


def slack(E, sc, L):
    """large-indel: 4096 - (64 E perCol + gaps + 64 E match + liftJD + 64); the bucket is inside the margin iff this is > 0"""
    match, mismatch, open_, extend, off_edge = sc[:5]
    q = 64 * E
    per_col = -min(mismatch, off_edge, 0)
    gaps = -_neg(open_) - _neg(extend) - _neg(L)
    lift = max(L - open_, 0)  # a sentinel-derived insert cell rises by L - open through the jump-deletion candidate
    return 4096 - (q * per_col + gaps + q * max(match, 0) + lift + 64)


def jump_slack(E, sc, jump):
    """jump: 8192 - (64 E perCol + gaps + 64 E match + 64)"""
    match, mismatch, open_, extend, off_edge = sc[:5]
    q = 64 * E
    per_col = -min(mismatch, off_edge, 0)
    return 8192 - (q * per_col - open_ - extend - jump + q * match + 64)


def _caps(sc, extra, small, big):
    match, mismatch, open_, extend, off_edge = sc[:5]
    return (open_ <= 0 and extend <= 0 and extra <= 0 and 0 <= match <= 64 and mismatch >= small and off_edge >= small and extend >= small
            and open_ >= big and extra >= big)


def pair_eligible(E, sc, L, allow_edge_ins):
    return E <= 6 and not allow_edge_ins and _caps(sc, L, -512, -2048) and slack(E, sc, L) > 0


def jump_pair_eligible(E, sc, jump):
    return E <= 8 and _caps(sc, jump, -1024, -4096) and jump_slack(E, sc, jump) > 0


def eligible(kind, E, sc, extra):
    return pair_eligible(E, sc, extra, sc[5]) if kind == LARGE_INDEL else (not sc[5] and jump_pair_eligible(E, sc, extra))


def slack_of(kind, E, sc, extra):
    return slack(E, sc, extra) if kind == LARGE_INDEL else jump_slack(E, sc, extra)


def pick_e(qlen):
    need = (qlen + 63) // 64
    return next((e for e in KESET if e >= need), KESET[-1])


def e_prev(E):
    i = KESET.index(E)
    return KESET[i - 1] if i else 0


# ---------------------------------------------------------------------------------------------------------------------------- score sets

# shape -> (p, E) -> (scores, extra).  Every shape is eligible at p = 1 for every packed E and leaves the margin (or a cap) as p grows.
SHAPES = {
    # every way of consuming a query base costs about p.  Jump aligner: the optimal path itself lies in the deepest real cells.
    # Large-indel aligner: its jump-insertion state takes ANY number of query bases for L = -2 p, so no cell sinks below about -4 p here ...
    "mismatch": lambda p, E: ([1, -p, -p, -p, -p, 0], -2 * p),
    # ... and only a large-indel score as deep as the whole diagonal (L = -64 E p) keeps the optimal path of an all-mismatch query on it:
    # the diagonal's last cells and the gap states beside them (diagonal + L) are the deepest real cells the rule allows for
    "deep": lambda p, E: ([1, -p, -p, -p, -p, 0], -64 * E * p),
    # sentinel-derived cells climb fastest
    "match": lambda p, E: ([p, -1, -2, -1, -1, 0], -4),
    # gap-state candidates: first the open, then the large-indel / jump score
    "gap-open": lambda p, E: ([2, -8, -p, -1, -1, 0], -100),
    "gap-extra": lambda p, E: ([2, -8, -24, -1, -1, 0], -p),
    # large-indel only: L less negative than open, so that the liftJD term is live
    "lift": lambda p, E: ([1, -p, -100, -1, -1, 0], -20),
}
LARGE_INDEL_ONLY = ("deep", "lift")


def tight(kind, E, shape):
    """-> (p of the eligible set with the smallest positive slack, p of its ineligible neighbour)"""
    make = SHAPES[shape]
    p = 1
    assert eligible(kind, E, *make(p, E)), (kind, E, shape)
    while eligible(kind, E, *make(p + 1, E)):
        p += 1
    return p, p + 1


def score_sets(kind, E):
    """the score sets one bucket width runs: dicts of name, sc, extra, eligible, slack, full (a whole batch or the reduced one)"""
    out = []

    def add(name, sc, extra, full):
        out.append(dict(name=name, sc=list(sc), extra=extra, eligible=eligible(kind, E, sc, extra), slack=slack_of(kind, E, sc, extra), full=full))

    add("production", *PRODUCTION["small-sv" if kind == LARGE_INDEL else "spanning"], True)
    for shape in SHAPES:
        if shape in LARGE_INDEL_ONLY and kind != LARGE_INDEL:
            continue
        p, p1 = tight(kind, E, shape)
        add(shape, *SHAPES[shape](p, E), True)
        add(shape + "+1", *SHAPES[shape](p1, E), False)
    if kind == LARGE_INDEL:  # (the jump aligner refuses is_allow_edge_insertion)
        sc, extra = PRODUCTION["small-sv"]
        add("edge-ins", sc[:5] + [1], extra, False)
    return out


# ----------------------------------------------------------------------------------------------------------------------------- sequences


def _rnd(rs, alphabet, n):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rs.randint(0, len(a), size=n)].tobytes() if n else b""


def _subst(rs, s, n, alphabet):
    s = bytearray(s)
    for _ in range(n):
        s[rs.randint(0, len(s))] = alphabet[rs.randint(0, len(alphabet))]
    return bytes(s)


def _rand_align_case(rng, kind, maxlen):
    """the random background of tests/test_oracle_vs_ref.py, restated: the stored digests depend on every draw of it, so it is kept
    here, where an edit shows up as a digest mismatch"""
    def rs(n, al="ACGT"):
        return "".join(rng.choice(al) for _ in range(n))

    def mut(s, rate):
        out = []
        for c in s:
            x = rng.random()
            if x < rate / 3:
                continue
            if x < 2 * rate / 3:
                out.append(rng.choice("ACGTN"))
                out.append(c)
                continue
            if x < rate:
                out.append(rng.choice("ACGTN"))
                continue
            out.append(c)
        return "".join(out)

    ref1 = rs(rng.randint(1, maxlen), rng.choice(["ACGT", "AC", "ACGTN"]))
    if kind == JUMP:
        ref2 = rs(rng.randint(1, maxlen), rng.choice(["ACGT", "AC"]))
        a, b = rng.randint(0, len(ref1)), rng.randint(0, len(ref2))
        q = ref1[max(0, a - rng.randint(0, maxlen // 2)):a] + rs(rng.choice([0, 0, 0, 1, 3, 8])) + ref2[b:b + rng.randint(0, maxlen // 2)]
        return (mut(q, rng.choice([0, 0.05, 0.2])) or rs(rng.randint(1, 10)), ref1, ref2)
    if rng.random() < 0.3:
        return (rs(rng.randint(1, maxlen // 2 + 1)), ref1, None)
    a = rng.randint(0, len(ref1))
    b = rng.randint(a, len(ref1))
    c = rng.randint(b, len(ref1))
    d = rng.randint(c, len(ref1))
    q = ref1[a:b] + rs(rng.choice([0, 0, 2, 30])) + ref1[c:d]
    return (mut(q, rng.choice([0, 0.05, 0.2])) or rs(rng.randint(1, 10)), ref1, None)


def _rand_background(kind, spec):
    rng = random.Random(spec["seed"])
    lo, hi = 64 * e_prev(spec["e"]) + 1, 64 * spec["e"]
    for _ in range(1000):
        q, r1, r2 = _rand_align_case(rng, kind, hi + 30)
        if lo <= len(q) <= hi:
            return q.encode("latin-1"), r1.encode("latin-1"), (r2.encode("latin-1") if r2 is not None else None)
    raise AssertionError(spec)


def make_case(kind, spec):
    """-> (query, ref1, ref2 or None) as bytes"""
    f = spec["f"]
    if f == "rand":
        return _rand_background(kind, spec)
    rs = np.random.RandomState(spec["seed"])
    Q, G = spec["q"], spec.get("g", 0)
    ACGT = b"ACGT"
    ref2 = None
    if f == "allmis":
        q, ref = b"A" * Q, b"C" * G
    elif f == "nq":
        q, ref = b"N" * Q, _rnd(rs, ACGT, G)
    elif f == "nr":
        q, ref = _rnd(rs, ACGT, Q), b"N" * G
    elif f == "allmatch":
        q, ref = b"A" * Q, b"A" * G
    elif f == "period":  # a pure repeat against the same repeat with one unit of phase slip in the middle
        unit = b"ACG"[:spec["k"]]
        q = (unit * Q)[:Q]
        full = (unit * (G + 1))[:G + 1]
        ref = full[:G // 2] + full[G // 2 + 1:]
    elif f == "half":  # half the query matches nowhere (the reference has no T), the other half is an exact copy of a window
        ref = _rnd(rs, b"ACG", G)
        w = Q - Q // 2
        at = spec["at"]
        q = (ref[at:at + w] + b"T" * (Q // 2)) if spec.get("mirror") else (b"T" * (Q // 2) + ref[at:at + w])
    elif f == "raw":  # bytes are compared raw: lower case and bytes >= 0x80 are symbols of their own
        alphabet = b"ACGTacgt\x80\xc1\xff"
        ref = _rnd(rs, alphabet, G)
        q = _subst(rs, ref[spec["at"]:spec["at"] + Q], max(1, Q // 16), alphabet)
    elif f in ("tie-del", "tie-ins"):
        # two reference windows joined in the query: across a deletion of d reference bases, or around d inserted bases.  For the jump
        # aligner ref2 holds the second window again, so that the jump competes with the gap.
        d, lf, rf = spec["d"], spec["lf"], spec["rf"]
        body = Q if f == "tie-del" else Q - d
        w1 = body // 2
        W1, W2 = _rnd(rs, ACGT, w1), _rnd(rs, ACGT, body - w1)
        mid = _rnd(rs, ACGT, d)
        if f == "tie-del":
            q, ref = W1 + W2, _rnd(rs, ACGT, lf) + W1 + mid + W2 + _rnd(rs, ACGT, rf)
        else:
            q, ref = W1 + mid + W2, _rnd(rs, ACGT, lf) + W1 + W2 + _rnd(rs, ACGT, rf)
        if kind == JUMP:
            ref2 = _rnd(rs, ACGT, lf + 3) + W2 + _rnd(rs, ACGT, rf + 2)
    elif f in ("in1", "in2", "r1one", "r2one"):  # jump only: the query lies wholly in one reference; the other may be a single base
        n1 = 1 if f == "r1one" else G
        n2 = 1 if f == "r2one" else G
        ref, ref2 = _rnd(rs, ACGT, n1), _rnd(rs, ACGT, n2)
        src = ref if f in ("in1", "r2one") else ref2
        q = _subst(rs, src[spec["at"]:spec["at"] + Q], 2, ACGT)
    elif f == "jins":  # jump only: ref1's window, k inserted bases, ref2's window
        ref, ref2 = _rnd(rs, ACGT, G), _rnd(rs, ACGT, G)
        k = spec["k"]
        w1 = (Q - k) // 2
        a, b = spec["at"] + w1, spec["at"]
        q = ref[a - w1:a] + _rnd(rs, ACGT, k) + ref2[b:b + Q - k - w1]
    else:
        raise KeyError(f)
    assert len(q) == Q, spec
    if kind == JUMP and ref2 is None:
        ref, ref2 = ref[:spec["split"]], ref[spec["split"]:]
    return q, ref, ref2


def digest(q, r1, r2):
    return hashlib.sha1(b"|".join((q, r1, r2 or b""))).hexdigest()[:12]


def cells(lens):
    return lens[0] * (lens[1] + lens[2])


def q_set(E):
    return (64 * e_prev(E) + 1, 64 * E - 1, 64 * E)


def _seed(kind, E, n):
    return 1000000 * kind + 10000 * E + n


def shortest_case(kind, E):
    """the shortest query of the bucket against the shortest reference: the partner that leaves almost the whole sweep to the other half"""
    g = 1 if kind == LARGE_INDEL else 2
    return dict(f="allmis", group="mis", seed=_seed(kind, E, 0), q=64 * e_prev(E) + 1, g=g, **({"split": 1} if kind == JUMP else {}))


def sequence_cases(kind, E):
    """the cases of one bucket that do not depend on the scores, in batch order (neighbours share a wave)"""
    out = []
    gmin = 1 if kind == LARGE_INDEL else 2
    qlo, qm, qhi = q_set(E)

    def add(f, group, q, g=None, lite=False, **kw):
        spec = dict(f=f, group=group, seed=_seed(kind, E, len(out) + 1), q=q, **kw)
        if g is not None:
            spec["g"] = g
            if kind == JUMP and f in ("allmis", "nq", "nr", "allmatch", "period", "half", "raw"):
                spec["split"] = (1, g // 2, g - 1, (g + 1) // 3)[len(out) % 4] if g > 2 else 1
        if f == "rand":
            spec["e"] = E
        if lite:
            spec["lite"] = 1
        out.append(spec)

    # all-mismatch diagonals; G = 1 and G = 3 Q are neighbours (a very unequal pair)
    for Q in (qlo, qm, qhi):
        seen = set()
        for g in {qhi: (gmin, 3 * Q, Q - 1, Q, Q + 1), qm: (gmin, Q, Q - 1, Q + 1), qlo: (gmin, Q)}[Q]:  # (the long sweep once per bucket)
            g = max(g, gmin)
            if g not in seen:
                seen.add(g)
                add("allmis", "mis", Q, g, lite=(Q == qhi and g == Q))
    add("nq", "mis", qhi, qhi + 17)
    add("nr", "mis", qm, qm + 17, lite=True)
    # every placement ties
    for g in (qm, qm + 1, 2 * qm + 37):
        add("allmatch", "tie", qm, max(g, gmin), lite=(g == qm + 1))
    add("period", "tie", qhi, qhi + 11, k=2)
    add("period", "tie", qlo, qlo + 12, k=3, lite=True)
    # half junk, half exact; raw bytes; random background
    add("half", "mix", qhi, qhi + 50, at=23, lite=True)
    add("half", "mix", qhi, qhi + 50, at=31, mirror=1)
    add("raw", "mix", qm, qm + 20, at=9, lite=True)
    for i in range(2):
        add("rand", "mix", 0, lite=(i == 0))
    if kind == JUMP:
        add("r1one", "mix", qhi, qhi + 30, at=11, lite=True)
        add("r2one", "mix", qm, qm + 30, at=7)
        add("in1", "mix", qhi, qhi + 40, at=19)
        add("in2", "mix", qlo, qlo + 40, at=5)
        for k, Q in ((0, qhi), (1, qm), (8, max(qlo, 12))):
            add("jins", "mix", Q, Q + 40, at=3, k=k, lite=(k == 1))
    return out


def tie_cases(kind, E, sc, extra):
    """two windows across a deletion / around an insertion of d bases with open + d extend = extra - 1, extra, extra + 1: the affine gap and
    the jump state (large-indel: jump-deletion / jump-insertion; jump aligner: the jump to ref2) tie at the middle d and each wins on one
    side.  Left out where extend = 0, where d would pass 2000, and where an insertion leaves the query's windows under 8 bases each."""
    open_, extend = sc[2], sc[3]
    if extend == 0:
        return []
    d0 = int(round((extra - open_) / float(extend)))
    out = []
    qlo, qm, qhi = q_set(E)
    for f, Q in (("tie-del", qm), ("tie-ins", qhi)):
        for d in (d0 - 1, d0, d0 + 1):
            if d < 1 or d > 2000 or Q < 16 or (f == "tie-ins" and Q - d < 16):
                continue
            n = 100 + len(out) + (50 if f == "tie-ins" else 0)
            out.append(dict(f=f, group="tie", seed=_seed(kind, E, n) + 7 * d, q=Q, d=d, lf=9 + d % 5, rf=12, lite=1))
    return out


def set_cases(kind, E, s):
    """every case of (kind, E, score set) in batch order; the reduced sets keep the cases marked lite"""
    cs = sequence_cases(kind, E) + tie_cases(kind, E, s["sc"], s["extra"])
    return cs if s["full"] else [c for c in cs if c.get("lite")]


def batch_order(kind, E, s, group, cases):
    """-> indices into cases + [shortest] (index len(cases)) for one device batch of a family group.

    A full batch presents the group's cases as neighbours (a copy of the same family shares the wave), pads to an even count with the
    shortest task, and then presents them again shifted by one behind the shortest task: whoever sat in the low halves now sits in the high
    ones, the first case shares its wave with the shortest task, and the odd last task runs against itself."""
    idx = [i for i, c in enumerate(cases) if c["group"] == group]
    if not s["full"] or not idx:
        return idx
    S = len(cases)
    first = idx + ([S] if len(idx) % 2 else [])
    return first + [S] + idx


def small_buckets(kind, E, cases):
    """buckets holding exactly 1, 2 and 3 tasks: a diagonal that leaves the table one row early, the shortest task, the full diagonal"""
    pick = [next(i for i, c in enumerate(cases) if c["f"] == "allmis" and c["q"] == 64 * E and c["g"] == 64 * E + 1), len(cases),
            next(i for i, c in enumerate(cases) if c["f"] == "allmis" and c["q"] == 64 * E and c["g"] == 64 * E)]
    return [pick[:1], pick[:2], pick]


# ----------------------------------------------------------------------------------------------------------------------------- row limit


def _row_case(kind, spec):
    """a short query (two windows, or one) planted at `at` in a random reference of spec["g"] rows; jump: the reference splits at `split`"""
    rs = np.random.RandomState(spec["seed"])
    G, at = spec["g"], spec["at"]
    ref = _rnd(rs, b"ACGT", G)
    if spec.get("two"):
        q = ref[at:at + 25] + ref[at + 45:at + 70] if kind == LARGE_INDEL else ref[at:at + 32] + ref[spec["at2"]:spec["at2"] + 32]
    else:
        q = ref[at:at + 48]
    q = _subst(rs, q, 1, b"ACGT")
    if kind == JUMP:
        return q, ref[:spec["split"]], ref[spec["split"]:]
    return q, ref, None


def row_limit_batches(kind):
    """-> list of (name, packed, scores, extra, [spec, ...]): total references of 65 534 rows stay packed, 65 535 moves the whole bucket to the
    unpacked kernel.  Queries of at most 64 bases (E = 1) so that the emulator can afford the sweeps; a query that short cannot pay for the
    spanning path's jump score of -100, so the jump aligner's batches run with -20."""
    G = ROW_LIMIT
    s = lambda n, **kw: dict(f="rows", seed=_seed(kind, 99, n), **kw)
    short = s(1, g=100, at=20, split=40)
    if kind == LARGE_INDEL:
        end, start = s(2, g=G, at=G - 49, two=0), s(3, g=G, at=0, two=1)
        over = s(4, g=G + 1, at=G - 48, two=0)
        sc, extra = PRODUCTION["small-sv"]
        return [("alone", True, sc, extra, [end]), ("short+start", True, sc, extra, [short, start]), ("over", False, sc, extra, [over, short])]
    seam1 = s(2, g=G, at=G - 60, two=0, split=1)
    seam_last = s(3, g=G, at=G - 49, two=0, split=G - 1)
    seam_mid = s(4, g=G, at=G // 2 - 32, two=1, at2=G // 2 + 7, split=G // 2)
    over = s(5, g=G + 1, at=G // 2 - 32, two=1, at2=G // 2 + 7, split=G // 2)
    sc, extra = PRODUCTION["spanning"][0], -20
    return [("alone", True, sc, extra, [seam1]), ("last+short", True, sc, extra, [seam_last, short]), ("short+mid", True, sc, extra, [short, seam_mid]),
            ("over", False, sc, extra, [over, short])]


def make_any(kind, spec):
    return _row_case(kind, spec) if spec["f"] == "rows" else make_case(kind, spec)
