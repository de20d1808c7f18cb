"""Piles that sit exactly ON a capacity bound of the assembler's LDS pipeline and their neighbours one over it (test_asm_edges.py).

The pipeline (asm_lds.hpp graph_kernel -> asm_contig.hpp contig_kernel / contig_pool_kernel; big class: asm_lds_big.hpp) keeps a
locus only while every one of its fixed-size structures holds; anything else goes to assemble_kernel through the punt list.  Random
piles sit far from every such bound, so each generator here BUILDS a pile for one bound and proves, through `measure` -- a plain
restatement of the quantities the kernels count, from the reads' text alone -- that the pile has exactly the value it was asked for
and crosses no OTHER bound by accident (`crossed`).  Edges are implicit by overlap as in the reference: a successor of w is any
word of the pile equal to w[1:] + c.

Every read is drawn from its own seeded random text, so the graphs are acyclic (`measure` checks: `chain` is None for a cycle)."""
import random
import re
import os

from oracle_lib import asm_opts

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "manta_amd", "csrc")

# ---- the bounds (tests/test_asm_edges.py::test_constants_match_the_sources reads them back from the headers) ----
LG_MAX_NODES = 1843    # words of a small-class graph
LG_MAX_READS = 128     # reads + 2 x maxAssemblyCount
LG_OVF_CAP = 32        # words with > 2 successors; the same for predecessors (a fourth link shares the third's entry)
LG_SIB_CAP = 32        # predecessor-less words that have a sibling
LG_MAX_PILE = 2046     # code dwords + 2.  UNREACHABLE: a read costs ceil(L/16)+1 code and ceil(L/32)+1 N-bitmap dwords, so mw >= cw/2 and
#                        the LDS line below refuses every pile from cw ~ 2000 on.  LG_PILE_DWORDS is the bound that binds and is tested.
LG_BUDGET = 81920
LG_OFF_DYN = 69888
LG_PILE_DWORDS = (LG_BUDGET - LG_OFF_DYN) // 4   # 3008: padded code + N-bitmap dwords of a pile in graph_kernel's LDS
CK_MAX_EXT = 1020      # extension steps of one walk, both directions together
CK_OFF_RECS = 1536
CK_CLASS_BYTES = (20480, 54272)   # contig_kernel's default LDS classes.  The second is UNREACHABLE from above: ckNeed of the largest
#                                   small-class graph (LG_MAX_NODES words, a read set each) is 45 776 bytes; LG_MAX_NODES binds first.
LGL_MAX_NODES = 7168
LGL_MAX_READS = 256
LGL_OVF_CAP = 128
LGL_MAX_PILE = 3598    # code dwords; the envelope is cw + 2 <= LGL_MAX_PILE + 2
LGL_POOL_CAP = 1280    # read sets (words with more than one read) in LDS ...
LGL_POOL_OVF = 704     # ... and further ones in the workgroup's device-memory workspace
LGL_DYN_DWORDS = 6016  # UNREACHABLE before LGL_MAX_PILE: 236 reads at most (maxAssemblyCount 10), so mw <= cw/2 + 236 and
#                        cwPad + mwPad <= 3600 + 2040 + 4; its second line (4 cwPad + LGL_MAX_NODES + 16 <= 4 LGL_DYN_DWORDS) allows cwPad 4220.
LGL_STAGE_BYTES = 73728  # host-only test for unpacked input, bases + 64 <= this.  UNREACHABLE: cw >= bases/16 + reads, so a pile inside
#                          LGL_MAX_PILE has at most 16 x 3598 = 57 568 bases.
LGL_CK_RECS = 4096
LGL_CLASS_BYTES = (81920, 163840)  # contig_big_kernel's classes.  The second is UNREACHABLE: 7168 words need 68 608 bytes + 32 per read
#                                    set, and the set pool ends at 1984 sets (132 096 bytes in all).


def header_constants():
    """the same names read from the sources (simple `static const unsigned NAME = <integer>;` lines, plus the two derived offsets)"""
    out = {}
    for f in ("asm_lds.hpp", "asm_lds_base.hpp", "asm_lds_big.hpp", "asm_contig.hpp"):
        for m in re.finditer(r"static const unsigned (\w+)\s*=\s*(\d+);", open(os.path.join(CSRC, f)).read()):
            out[m.group(1)] = int(m.group(2))
    return out


def rs(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def others(rng, c, n=1):
    return rng.sample([x for x in "ACGT" if x != c], n)


def measure(reads, k):
    """What the kernels count for this pile at word length k, from the text alone."""
    count = {}
    for r in reads:
        seen = set()
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if "N" in w or w in seen:
                continue
            seen.add(w)
            count[w] = count.get(w, 0) + 1
    succ = {w: [w[1:] + c for c in "ACGT" if w[1:] + c in count] for w in count}
    npred = {w: sum(1 for c in "ACGT" if c + w[:-1] in count) for w in count}
    sib = sum(1 for w in count if npred[w] == 0 and any(w[:-1] + c in count for c in "ACGT" if c != w[-1]))
    # longest path, in words (Kahn): the most words any walk can string together; None if the graph has a cycle
    indeg = dict(npred)
    depth = {w: 1 for w in count}
    todo = [w for w in count if indeg[w] == 0]
    done = 0
    while todo:
        w = todo.pop()
        done += 1
        for s in succ[w]:
            depth[s] = max(depth[s], depth[w] + 1)
            indeg[s] -= 1
            if indeg[s] == 0:
                todo.append(s)
    cw = sum((len(r) + 15) // 16 + 1 for r in reads)
    mw = sum((len(r) + 31) // 32 + 1 for r in reads)
    return dict(reads=len(reads), words=len(count), fat=sum(1 for c in count.values() if c > 1),
                sovf=sum(1 for w in count if len(succ[w]) > 2), povf=sum(1 for w in count if npred[w] > 2), sib=sib,
                four_way=sum(1 for w in count if len(succ[w]) > 3 or npred[w] > 3),
                cw=cw, mw=mw, padded=((cw + 2 + 3) & ~3) + ((mw + 2 + 3) & ~3), bases=sum(len(r) for r in reads),
                longest=max([len(r) for r in reads] or [0]), chain=(max(depth.values() or [0]) if done == len(count) else None),
                max_count=max(count.values() or [0]))


def ck_need(n_nodes, n_fat, acyclic, big=False):
    """ckNeed / ckNeedOf<LgL> (asm_lds.hpp): LDS the contig kernel needs for a graph"""
    kahn = 0 if acyclic else (4 * ((n_nodes + 3) // 4) + 2 * n_nodes + 32 + 15) & ~15
    pool = (32 if big else 16) * max(n_fat, 1)
    return (LGL_CK_RECS if big else CK_OFF_RECS) + ((8 * n_nodes + 15) & ~15) + (((n_nodes + 15) & ~15) if big else 0) + max(pool, kahn)


def crossed(m, mac, big=False):
    """names of the class' bounds this pile is over (the generators assert: exactly the one asked for, or none)"""
    assert m["chain"] is not None, "cyclic graph"
    need = max(ck_need(m["words"], m["fat"], a, big) for a in (True, False))
    if big:
        cw_pad, mw_pad = (m["cw"] + 2 + 3) & ~3, (m["mw"] + 2 + 3) & ~3
        b = dict(reads=m["reads"] + 2 * mac > LGL_MAX_READS or m["reads"] > 255, words=m["words"] > LGL_MAX_NODES, sovf=m["sovf"] > LGL_OVF_CAP,
                 povf=m["povf"] > LGL_OVF_CAP, sib=m["sib"] > LG_SIB_CAP, pool=m["fat"] > LGL_POOL_CAP + LGL_POOL_OVF, walk=m["chain"] - 1 > CK_MAX_EXT,
                 pile=m["cw"] + 2 > LGL_MAX_PILE + 2 or m["longest"] > 0xffff,
                 dyn=cw_pad + mw_pad > LGL_DYN_DWORDS or 4 * cw_pad + LGL_MAX_NODES + 16 > 4 * LGL_DYN_DWORDS, stage=m["bases"] + 64 > LGL_STAGE_BYTES,
                 ck=need > LGL_CLASS_BYTES[-1])
    else:
        b = dict(reads=m["reads"] + 2 * mac > LG_MAX_READS, words=m["words"] > LG_MAX_NODES, sovf=m["sovf"] > LG_OVF_CAP, povf=m["povf"] > LG_OVF_CAP,
                 sib=m["sib"] > LG_SIB_CAP, walk=m["chain"] - 1 > CK_MAX_EXT, pile=m["padded"] > LG_PILE_DWORDS or m["longest"] > 0xffff,
                 max_pile=m["cw"] + 2 > LG_MAX_PILE, ck=need > CK_CLASS_BYTES[-1])
    return sorted(n for n, over in b.items() if over)


class Case:
    """route: 'small' / 'big' = finishes on that class of the pipeline; 'small-punt' / 'big-punt' = taken by the class, handed to the
    general kernel by the device; 'outside' = the host gives it to the general kernel.  trace: what MANTA_EMU_PUNT_TRACE prints for it
    (None: that path prints nothing).  counter: the field of the big class' debug line a big-punt raises."""

    def __init__(self, name, k, reads, route, over=(), trace=None, counter=None, big=False, **opts):
        o = dict(minWordLength=k, maxWordLength=k, minCoverage=1, maxAssemblyCount=10)
        o.update(opts)
        self.name, self.k, self.reads, self.route, self.trace, self.counter, self.big = name, k, reads, route, trace, counter, big
        self.mac = o["maxAssemblyCount"]
        self.opts = asm_opts(**o)
        self.m = measure(reads, k)
        got = crossed(self.m, self.mac, big)
        assert got == sorted(over), (name, got, over, self.m)
        if not big and "reads" not in over and "pile" not in over:
            assert self.m["reads"] + 2 * self.mac <= LG_MAX_READS
        if big:  # the host must not give it to the small class
            assert self.m["reads"] + 2 * self.mac > LG_MAX_READS or self.m["padded"] > LG_PILE_DWORDS

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------------------
# the constructions.  `pad_to`: big class -- duplicates of a short read that is a substring of the pile's first read (no new word, no new
# read set beyond the four words it covers) bring the read count into the big class' range
# ---------------------------------------------------------------------------------------------------------------------------------
def _pad(reads, k, pad_to):
    if pad_to:
        assert len(reads) <= pad_to
        reads = reads + [reads[0][:k + 3]] * (pad_to - len(reads))
    return reads


def words_pile(seed, k, n, copies=3, seg=400, pad_to=0):
    """n distinct words in segments of at most `seg` words (a single segment would cross the walk bound first)"""
    rng = random.Random(seed)
    reads = []
    while n > 0:
        m = min(seg, n)
        n -= m
        reads += [rs(rng, m + k - 1)] * copies
    return _pad(reads, k, pad_to)


def _backbones(rng, k, n_branch, per_backbone, copies):
    """backbones with branch points 24 apart; (backbone, branch position) pairs"""
    reads, points = [], []
    while n_branch > 0:
        nb = min(per_backbone, n_branch)
        n_branch -= nb
        B = rs(rng, 24 * nb + 2 * k + 50)
        reads += [B] * copies
        points += [(B, k + 20 + 24 * i) for i in range(nb)]
    return reads, points


def _branch_reads(rng, points, four_way, snippet, join):
    """per alternative base one list of snippets; join > 1: that many snippets per read, an N between them (no word spans it)"""
    alts = [[], [], []]
    for i, (B, p) in enumerate(points):
        for j, a in enumerate(others(rng, B[p], 3 if i < four_way else 2)):
            alts[j].append(snippet(B, p, a))
    return ["N".join(sn[i:i + join]) for sn in alts for i in range(0, len(sn), join)]


def sovf_pile(seed, k, n_branch, four_way=0, per_backbone=40, copies=2, join=1, pad_to=0):
    """n_branch words with three successors (the first `four_way` of them with four): two (three) snippets B[p-k:p] + a, a != B[p]"""
    rng = random.Random(seed)
    reads, points = _backbones(rng, k, n_branch, per_backbone, copies)
    return _pad(reads + _branch_reads(rng, points, four_way, lambda B, p, a: B[p - k:p] + a, join), k, pad_to)


def povf_pile(seed, k, n_branch, four_way=0, per_backbone=40, copies=2, join=1, pad_to=0):
    """the mirror image: snippets a + B[p+1:p+1+k]"""
    rng = random.Random(seed)
    reads, points = _backbones(rng, k, n_branch, per_backbone, copies)
    return _pad(reads + _branch_reads(rng, points, four_way, lambda B, p, a: a + B[p + 1:p + 1 + k], join), k, pad_to)


def sib_pile(seed, k, n_pairs, n_triples=0, pad_to=0):
    """groups of sibling start words: S (k + 6 bases) twice and S with base k-1 replaced (once: a pair, two table entries; twice: a triple)"""
    rng = random.Random(seed)
    reads = []
    for i in range(n_pairs + n_triples):
        S = rs(rng, k + 6)
        reads += [S, S] + [S[:k - 1] + a + S[k:] for a in others(rng, S[k - 1], 2 if i >= n_pairs else 1)]
    return _pad(reads, k, pad_to)


def walk_pile(seed, k, ext, middle_seed=False, copies=3, pad_to=0):
    """one chain of ext + 1 words; middle_seed: a further copy of a central window makes its words the first seed, so that the walk reaches
    the bound from two directions"""
    rng = random.Random(seed)
    S = rs(rng, ext + k)
    reads = [S] * copies
    if middle_seed:
        c = len(S) // 2
        reads.append(S[c - (k + 10) // 2:c - (k + 10) // 2 + k + 10])
    if pad_to:  # (big class: the padding reads are a central window too)
        c = len(S) // 2
        reads += [S[c:c + k + 3]] * (pad_to - len(reads))
    return reads


def _dwords(reads):
    cw = sum((len(r) + 15) // 16 + 1 for r in reads)
    mw = sum((len(r) + 31) // 32 + 1 for r in reads)
    return cw, ((cw + 2 + 3) & ~3) + ((mw + 2 + 3) & ~3)


def budget_pile(seed, k, target, by_code_dwords=False):
    """five random 320-base segments in rotation until the measure would pass `target`, then one shortened read to land on it: the padded
    dword sum of the small class (steps of 4), or -- by_code_dwords -- cw + 2 of the big class"""
    rng = random.Random(seed)
    segs = [rs(rng, 320) for _ in range(5)]
    val = (lambda rd: _dwords(rd)[0] + 2) if by_code_dwords else (lambda rd: _dwords(rd)[1])
    reads, i = [], 0
    while val(reads + [segs[i % 5]]) <= target:
        reads.append(segs[i % 5])
        i += 1
    L = 320
    while L >= k and val(reads + [segs[i % 5][:L]]) > target:
        L -= 1
    if L >= k:
        reads.append(segs[i % 5][:L])
    assert val(reads) == target, (val(reads), target)
    return reads


def reads_pile(seed, k, n_reads):
    """n_reads overlapping windows of one random text"""
    rng = random.Random(seed)
    T = rs(rng, 60 + k + 30)
    return [T[i % 60:i % 60 + k + 30] for i in range(n_reads)]


def fat_pile(seed, k, n_fat, n_pairs=65):
    """n_fat words with more than one read, each in EXACTLY two reads: n_pairs short segments in two copies (130 reads: the big class'
    range without padding), and 2000 words with one read.  graph_big_kernel's table pass hands a set to a word at its second sighting
    and, when two waves sight it at once, one entry more that stays empty -- with exactly one second sighting per word the number of
    entries handed out is n_fat whatever the waves' timing, which the at-cap pile needs (identical padding reads would not give that)"""
    rng = random.Random(seed)
    reads = []
    for i in range(n_pairs):
        m = n_fat // n_pairs + (1 if i < n_fat % n_pairs else 0)
        reads += [rs(rng, m + k - 1)] * 2
    return reads + words_pile(seed + 1, k, 2000, copies=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------------
def small_table_cases(k):
    """the three side tables at cap - 1, cap, cap + 1 and with four-way words (their fourth link shares the entry)"""
    c = []
    for n in (31, 32, 33):
        over = n > LG_OVF_CAP
        c.append(Case("sovf%d_k%d" % (n, k), k, sovf_pile(1, k, n), "small-punt" if over else "small", over=["sovf"] if over else []))
        c.append(Case("povf%d_k%d" % (n, k), k, povf_pile(2, k, n), "small-punt" if over else "small", over=["povf"] if over else []))
    c.append(Case("sovf32_fourway_k%d" % k, k, sovf_pile(3, k, 32, four_way=32), "small"))
    c.append(Case("povf32_fourway_k%d" % k, k, povf_pile(4, k, 32, four_way=32), "small"))
    c.append(Case("sib32_k%d" % k, k, sib_pile(5, k, 16), "small"))
    c.append(Case("sib33_k%d" % k, k, sib_pile(5, k, 15, 1), "small-punt", over=["sib"]))
    for x, (field, n) in zip(c, [("sovf", 31), ("povf", 31), ("sovf", 32), ("povf", 32), ("sovf", 33), ("povf", 33), ("sovf", 32), ("povf", 32), ("sib", 32), ("sib", 33)]):
        assert x.m[field] == n, (x.name, x.m)
    assert c[6].m["four_way"] == 32 and c[7].m["four_way"] == 32
    return c


def small_capacity_cases(k=21):
    c = []
    for n in (LG_MAX_NODES, LG_MAX_NODES + 1):
        over = n > LG_MAX_NODES
        c.append(Case("words%d" % n, k, words_pile(6, k, n), "small-punt" if over else "small", over=["words"] if over else []))
        assert c[-1].m["words"] == n and c[-1].m["fat"] == n
    # (words1843 is also the closest a small-class graph comes to contig_kernel's 54 272-byte class from below: 45 776 bytes)
    assert ck_need(c[0].m["words"], c[0].m["fat"], True) == 45776
    for e in (CK_MAX_EXT - 1, CK_MAX_EXT, CK_MAX_EXT + 1):
        for mid in (False, True):
            over = e > CK_MAX_EXT
            c.append(Case("walk%d%s" % (e, "_mid" if mid else ""), k, walk_pile(7, k, e, middle_seed=mid), "small-punt" if over else "small",
                          over=["walk"] if over else [], trace="contig too long" if over else None))
            assert c[-1].m["chain"] == e + 1 and c[-1].m["words"] == e + 1 and c[-1].m["max_count"] == (4 if mid else 3)
    # pile bytes: 3008 padded dwords fit graph_kernel's LDS; 3012 do not, and the HOST knows (lgPileFits): the big class takes the pile
    c.append(Case("pile%d" % LG_PILE_DWORDS, k, budget_pile(8, k, LG_PILE_DWORDS), "small"))
    c.append(Case("pile%d" % (LG_PILE_DWORDS + 4), k, budget_pile(8, k, LG_PILE_DWORDS + 4), "big", over=[], big=True))
    assert c[-2].m["padded"] == LG_PILE_DWORDS and c[-1].m["padded"] == LG_PILE_DWORDS + 4 and c[-1].m["cw"] + 2 <= LG_MAX_PILE
    assert c[-1].m["reads"] <= 108
    # read count: reads + 2 x maxAssemblyCount = 128, then 129 (the host gives that one to the big class)
    for mac, n in ((10, 108), (10, 109), (2, 124), (2, 125)):
        over = n + 2 * mac > LG_MAX_READS
        c.append(Case("reads%d_mac%d" % (n, mac), k, reads_pile(9, k, n), "big" if over else "small", big=over, maxAssemblyCount=mac))
        assert c[-1].m["reads"] + 2 * mac == (129 if over else 128)
    # contig LDS classes: 789 words with a read set each need exactly 20 480 bytes (the pool class), 790 need 20 496 (contig_kernel's
    # 54 272-byte class); every word has a set, so ckNeed does not depend on the proof of acyclicity (16 x sets > the cycle test's state)
    for n in (789, 790):
        c.append(Case("ckclass%d" % n, k, walk_pile(10, k, n - 1), "small"))
        x = c[-1]
        x.need = ck_need(x.m["words"], x.m["fat"], True)
        assert x.need == ck_need(x.m["words"], x.m["fat"], False) == (20480 if n == 789 else 20496), x.need
        x.pooled = x.need <= CK_CLASS_BYTES[0]
    return c


BIG_PAD = 130  # reads of a padded big-class pile (+ 20 for maxAssemblyCount 10: between the small class' 128 and the big class' 256)


def big_cases(k=21):
    """the big class' own bounds; single-copy backbones keep the read-set count low while the side tables fill"""
    c = []

    def add(name, reads, over=None, counter=None, trace=None, route=None):
        c.append(Case(name, k, reads, route or ("big-punt" if over else "big"), over=[over] if over else [], counter=counter, trace=trace, big=True))
        return c[-1]

    for n in (LGL_MAX_NODES, LGL_MAX_NODES + 1):
        x = add("big_words%d" % n, words_pile(11, k, n, copies=1, pad_to=BIG_PAD), "words" if n > LGL_MAX_NODES else None, "words", "too many words")
        assert x.m["words"] == n
    for n in (LGL_OVF_CAP, LGL_OVF_CAP + 1):
        over = n > LGL_OVF_CAP
        x = add("big_sovf%d" % n, sovf_pile(12, k, n, four_way=5, per_backbone=36, copies=1, join=8, pad_to=BIG_PAD), "sovf" if over else None, "words", "side tables full")
        assert x.m["sovf"] == n
        x = add("big_povf%d" % n, povf_pile(13, k, n, four_way=5, per_backbone=36, copies=1, join=8, pad_to=BIG_PAD), "povf" if over else None, "words", "side tables full")
        assert x.m["povf"] == n
    add("big_sib32", sib_pile(14, k, 16, pad_to=BIG_PAD))
    add("big_sib33", sib_pile(14, k, 15, 1, pad_to=BIG_PAD), "sib", "words", "side tables full")
    assert c[-2].m["sib"] == 32 and c[-1].m["sib"] == 33
    # the set pool: the 1281st set lives in the workgroup's device-memory workspace (no route change); the 1985th does not exist
    for n in (LGL_POOL_CAP, LGL_POOL_CAP + 1, LGL_POOL_CAP + LGL_POOL_OVF, LGL_POOL_CAP + LGL_POOL_OVF + 1):
        over = n > LGL_POOL_CAP + LGL_POOL_OVF
        x = add("big_sets%d" % n, fat_pile(15, k, n), "pool" if over else None, "table", "table pass (table or set pool full)")
        assert x.m["fat"] == n and x.m["max_count"] == 2
    for e in (CK_MAX_EXT, CK_MAX_EXT + 1):
        over = e > CK_MAX_EXT
        x = add("big_walk%d" % e, walk_pile(16, k, e, copies=2, pad_to=BIG_PAD), "walk" if over else None, "contig", "contig too long")
        assert x.m["chain"] == e + 1
    # pile: cw + 2 = LGL_MAX_PILE + 2 stays; one dword more and the host keeps it off the pipeline
    add("big_pile%d" % (LGL_MAX_PILE + 2), budget_pile(17, k, LGL_MAX_PILE + 2, by_code_dwords=True))
    add("big_pile%d" % (LGL_MAX_PILE + 3), budget_pile(17, k, LGL_MAX_PILE + 3, by_code_dwords=True), "pile", route="outside")
    assert c[-2].m["cw"] == LGL_MAX_PILE and c[-1].m["cw"] == LGL_MAX_PILE + 1
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# orders the compact records cannot carry (no capacity involved): which contigs come out, and in which order, IS the seed order
# ---------------------------------------------------------------------------------------------------------------------------------
def saturated_count_pile(seed, k, big=False):
    """isolated segments whose words have counts 14, 15, 16, 17, 18 and 40; every word of a segment starts with the segment's own base and
    the bases run AGAINST the counts.  With maxAssemblyCount 2 the contig loop builds four candidates: by true count from the 40-, 18-,
    17- and 16-count segments; a sort on counts saturated at 15 (the record's field) ties five segments, orders them by k-mer and builds
    from the 15-, 16-, 17- and 18-count ones -- the 40-count segment, the first contig of the assembly, is never walked"""
    rng = random.Random(seed)
    reads, segs = [], {}
    # (big: a further segment of count 13 brings the pile to 133 reads, the big class' range, and is never a candidate)
    for cnt, base in ((15, "A"), (16, "A"), (17, "C"), (18, "G"), (40, "T"), (14, "T")) + (((13, "T"),) if big else ()):
        segs[cnt] = base * 4 + rs(rng, k - 1)  # four words, each starting with `base`
        reads += [segs[cnt]] * cnt
    rng.shuffle(reads)
    return reads, segs


def tie_pile(seed, k, pad_reads=0):
    """words of equal count that share everything but their last one or two bases (so: their first 16, or 32, bases), more than twenty of
    them, each its own read in two copies, in shuffled order; plus, for the first group, the words that hold the group's prefix shifted
    by one (they precede the group's words: four-way branches)"""
    rng = random.Random(seed)
    t = 1 if k - 2 < (32 if k > 32 else 16) else 2
    groups = 2 if t == 2 else 6
    reads = []
    for g in range(groups):
        P = rs(rng, k - t)
        tails = ["".join((a, b)) for a in "ACGT" for b in "ACGT"] if t == 2 else list("ACGT")
        reads += [P + x for x in tails] * 2
        if g == 0:
            reads += [z + P + x for z in "AC" for x in (list("ACGT") if t == 2 else [""])] * 2
    assert all(len(r) == k for r in reads)
    if pad_reads:  # big class: an isolated segment in that many copies (it is the first seed; the tie decides the other candidates)
        reads += [rs(rng, k + 3)] * pad_reads
    rng.shuffle(reads)
    return reads


def threshold_pile(seed, k, t, shift=0):
    """isolated segments whose words have counts t - 1, t and t + 1 (+ shift); returns the reads and the segments by count"""
    rng = random.Random(seed)
    reads, segs = [], {}
    for cnt in (t - 1 + shift, t + shift, t + 1 + shift):
        segs[cnt] = rs(rng, k + 8)
        reads += [segs[cnt]] * cnt
    rng.shuffle(reads)
    return reads, segs


def key_words(word):
    """a word as the kernels' key: 2-bit codes, A C G T = 0..3, sixteen bases per dword from the top, zero padded"""
    out = []
    for i in range(0, len(word), 16):
        v = 0
        for j, ch in enumerate(word[i:i + 16]):
            v |= "ACGT".index(ch) << (30 - 2 * j)
        out.append(v)
    return out


def key_hash(word):
    """LdsGraph::keyHash (asm_lds.hpp): bucket = h & 511, tag = h >> 15"""
    h = 0x811C9DC5
    for v in key_words(word):
        h ^= v
        h = (h * 0x9E3779B1) & 0xffffffff
        h ^= h >> 15
    h ^= h >> 13
    h = (h * 0x85EBCA6B) & 0xffffffff
    h ^= h >> 16
    return h


def tag_pressure_pile(seed, k, n_words=1700, want_pairs=3):
    """~n_words distinct words among which `want_pairs` pairs share hash bucket AND 17-bit tag (a slot cannot tell them apart without the
    key compare).  Random piles of this size have such a pair once in forty: the pairs are searched among the words of many random
    segments and the pile is built around the segments that hold them."""
    rng = random.Random(seed)
    seg_words = 20
    segs, by_sig, pairs = [], {}, []
    while len(pairs) < want_pairs:
        S = rs(rng, seg_words + k - 1)
        si = len(segs)
        segs.append(S)
        for i in range(seg_words):
            h = key_hash(S[i:i + k])
            sig = (h & 511, h >> 15)
            if sig in by_sig and by_sig[sig] != si and all(si not in p and by_sig[sig] not in p for p in pairs):
                pairs.append((by_sig[sig], si))
            by_sig.setdefault(sig, si)
    keep = [s for p in pairs for s in p]
    keep += [i for i in range(len(segs)) if i not in keep][:n_words // seg_words - len(keep)]
    reads = [segs[i] for i in keep]
    rng.shuffle(reads)
    words = [r[i:i + k] for r in reads for i in range(seg_words)]
    sigs = {}
    for w in set(words):
        h = key_hash(w)
        sigs.setdefault((h & 511, h >> 15), []).append(w)
    assert sum(1 for v in sigs.values() if len(v) > 1) >= want_pairs
    return reads
