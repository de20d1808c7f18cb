"""Constructed loci for the pipeline glue (tests/test_glue_edges.py): the contig, the place of every 10-mer hit and the distance
from a junction to a cut edge are chosen here, not left to a generator.  No device code.

The technique: a pile of five to seven copies of ONE read, assembled at a single word length k with minContigLength at most the read's
length, yields exactly that read as its one contig -- provided no k-mer of the read repeats and it holds no 'N' (the seed is the whole
read's path, every copy supports it, and nothing is left for a second contig).  Several groups of copies with DIFFERENT copy counts
(7, 6, 5) yield their reads in that order: the seed is the most frequent unused word.  Every helper returns the contigs it intends, and
the tests' first assertion per locus is that the device's contigs equal them, in order.

Small-SV helpers also restate the reference's 10-mer trim on strings (SVCandidateAssemblyRefiner.cpp:1984-2011) and assert, here, that
the hits lie where the case wants them (a chance hit of a random window would move them) and that lead + trail < len(ref): where the
reference's own range goes negative (:2032-2037) there is nothing to compare, and such a locus is a generator bug."""
import random
import zlib

from oracle_lib import asm_opts
from test_fused_schedule import SC  # small-SV scores, large-indel score -100
from test_spanning_pipeline import SC as SPAN_SC  # spanning scores, jump score -100

MER = 10
MER_BATCH = 55  # smallsv_trim.hpp: start positions per scan window
SCHED_SEQ_BYTES = 6144  # smallsv_trim.hpp (device constants have no other home on the Python side)
SCHED_PEND = 8  # pipeline_kernels.hpp
EDGE_D = (0, 1, 53, 54, 55, 56, 109, 110, 111)
CONTIG_LENGTHS = (10, 11, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 384, 385, 511, 512, 513)


def opts_for(k, min_len, **kw):
    """one word length k; minContigLength is the shortest contig of the family, 15 (Manta's default) at the most"""
    kw.setdefault("minCoverage", BALLAST_COVERAGE)
    return asm_opts(minWordLength=k, maxWordLength=k, minContigLength=min(min_len, 15), **kw)


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def kmers_unique(seq, k):
    return len({seq[i:i + k] for i in range(len(seq) - k + 1)}) == len(seq) - k + 1


def rand_contig(rng, n, k, avoid=()):
    """n random bases without a repeated (k-1)-mer (no branch in the graph: the pile's precondition), sharing no 10-mer with the texts in `avoid`"""
    assert n >= k
    taken = {t[i:i + MER] for t in avoid for i in range(len(t) - MER + 1)}
    while True:
        s = rand_seq(rng, n)
        if kmers_unique(s, min(k - 1, MER)) and not any(s[i:i + MER] in taken for i in range(n - MER + 1)):
            return s


def rand_flank(rng, n, contigs):
    """n random bases that hold no 10-mer of the contigs, even across their own ends' neighbours (checked again by trim())"""
    mers = {c[i:i + MER] for c in contigs for i in range(len(c) - MER + 1)}
    while True:
        s = rand_seq(rng, n)
        if not any(s[i:i + MER] in mers for i in range(n - MER + 1)):
            return s


def trim(contig, ref, cuts):
    """the reference's trim on strings -> (lead, trail)"""
    lead_cut, trail_cut, max_lead, max_trail = cuts
    mers = {contig[i:i + MER] for i in range(len(contig) - MER + 1)}
    n = len(ref)
    max_ref = n - (trail_cut + MER)
    max_fwd = min(max_lead, max_ref)
    i = lead_cut
    while i <= max_fwd and not (len(ref[i:i + MER]) == MER and ref[i:i + MER] in mers):
        i += 1
    lead = i
    min_rev = max(lead_cut, n - max_trail)
    i = max_ref
    while i >= min_rev and not (i >= 0 and len(ref[i:i + MER]) == MER and ref[i:i + MER] in mers):
        i -= 1
    return lead, n - (i + MER)


class Locus:
    """one small-SV locus: reads, window, cuts, the contigs it must yield, and per contig the (lead, trail) the trim must find"""

    def __init__(self, reads, ref, cuts, contigs, want=None, name=""):
        self.reads, self.ref, self.cuts, self.contigs, self.name = reads, ref, tuple(cuts), list(contigs), name
        self.trims = [trim(c, ref, self.cuts) for c in self.contigs]
        for (lead, trail) in self.trims:
            assert 0 <= lead and 0 <= trail and lead + trail < len(ref), (name, lead, trail, len(ref))
        if want is not None:
            assert self.trims == list(want), (name, self.trims, want)

    @property
    def pair(self):
        return (self.reads, self.ref)


BALLAST_COVERAGE = 3  # minCoverage of a pile with ballast: the ballast's words, two reads each, seed nothing


def add_ballast(loci, k, n=4, length=80):
    """On contig_pool_kernel a locus' LDS share is its graph's own size, and the epilogue takes the locus only when the share holds the
    trim's 4 KB table and the texts (asm_contig.hpp: scheduleEpilogue) -- a pile of five short reads is smallsv_schedule_kernel's there.
    `n` more reads, two copies each, enlarge the graph without a contig of their own: with minCoverage 3 none of their words is a seed,
    they share no (k-1)-mer with the contigs or each other, so no walk reaches them.  The contigs stay what they were (asserted by the
    tests on every route)."""
    for l in loci:
        rng = random.Random(zlib.crc32(l.contigs[0]))
        texts = list(l.contigs)
        for _ in range(n):
            while True:
                s = rand_seq(rng, length)
                seen = {t[i:i + k - 1] for t in texts for i in range(len(t) - k + 2)}
                if kmers_unique(s, k - 1) and not any(s[i:i + k - 1] in seen for i in range(length - k + 2)):
                    break
            texts.append(s)
            l.reads = l.reads + [s, s]
    return loci


def pile(contigs, counts=(7, 6, 5)):
    """groups of copies, the most copies first (a single contig: five copies)"""
    if len(contigs) == 1:
        return [contigs[0]] * 5
    assert len(contigs) <= len(counts)
    return [c for c, n in zip(contigs, counts) for _ in range(n)]


def placed(seed, clen, k, lead_cut, d_fwd, d_bwd, trail_cut, max_lead=None, max_trail=None, edit=None, decoy=False, name="", want="auto"):
    """A window that holds the contig once: its first 10-mer `d_fwd` positions behind leadingCut, its last one `d_bwd` positions below
    refSize - trailingCut - 10.  `edit(window copy of the contig) -> bytes` alters the window's copy (an 'N', another byte);
    `decoy`: the contig's last 10-mer one position before leadingCut and its first one position behind the last start the backward scan
    may take -- both must be ignored."""
    rng = random.Random(seed)
    contig = rand_contig(rng, clen, k)
    pre = rand_flank(rng, lead_cut + d_fwd, [contig])
    post = rand_flank(rng, trail_cut + d_bwd, [contig])
    if decoy:
        assert lead_cut >= 1 and trail_cut >= 1 and d_fwd >= 9 and d_bwd >= 9
        pre = pre[:lead_cut - 1] + contig[-MER:] + pre[lead_cut + 9:]
        at = len(post) - trail_cut - 9  # in `post`: start of the 10-mer one position behind refSize - trailingCut - 10
        post = post[:at] + contig[:MER] + post[at + MER:]
    body = contig if edit is None else edit(contig)
    assert len(body) == clen
    ref = pre + body + post
    p = lead_cut + d_fwd
    cuts = (lead_cut, trail_cut, len(ref) if max_lead is None else max_lead, len(ref) if max_trail is None else max_trail)
    if want == "auto":
        want = [(p, trail_cut + d_bwd)] if edit is None else None
    return Locus(pile([contig]), ref, cuts, [contig], want, name or "placed(%d,%d,%d,%d)" % (seed, clen, d_fwd, d_bwd))


# ---- the scans' window edges --------------------------------------------------------------------------------------------------------
def scan_edge_loci(k=15, clen=40):
    """forward and backward scan: first / last hit d positions into the scan for every d of EDGE_D (both scans step 55 positions), with
    and without decoys outside the scan range, and the hit at / behind maxLeadingCut and at / below minRevRefIndex"""
    loci = []
    for n, d in enumerate(EDGE_D):
        loci.append(placed(1000 + n, clen, k, 20, d, 30, 20, name="fwd d=%d" % d))
        loci.append(placed(1100 + n, clen, k, 20, 30, d, 20, name="bwd d=%d" % d))
        loci.append(placed(1200 + n, clen, k, 20, d, d, 20, name="both d=%d" % d))
        if d >= 9:
            loci.append(placed(1300 + n, clen, k, 20, d, d, 20, decoy=True, name="decoys d=%d" % d))
    # maxLeadingCut: the hit exactly there counts; one and two behind it do not, lead is maxFwd + 1 (the backward hit keeps the window)
    for n, past in enumerate((0, 1, 2)):
        p = 20 + 70
        loci.append(placed(1500 + n, clen, k, 20, 70, 30, 20, max_lead=p - past, want=[(p if past == 0 else p - past + 1, 50)],
                           name="maxLeadingCut %d before the hit" % past))
    # minRevRefIndex = refSize - maxTrailingCut: the last hit exactly there counts, one and two below it do not
    for n, below in enumerate((0, 1, 2)):
        # last 10-mer at q = refSize - 20 - 10 - 70; minRev = q + below  <=>  maxTrailingCut = refSize - q - below = 100 - below
        loci.append(placed(1600 + n, clen, k, 20, 30, 70, 20, max_trail=100 - below,
                           want=[(50, 90 if below == 0 else 100 - below + 1 - MER)], name="minRevRefIndex %d above the hit" % below))
    return add_ballast(loci, k), opts_for(k, clen)


def extreme_cut_loci(k=15, clen=40):
    loci = [placed(1700, clen, k, 0, 0, 30, 20, name="leadingCut 0, hit at 0"),
            placed(1701, clen, k, 20, 30, 0, 0, name="trailingCut 0, hit ends the window"),
            placed(1702, clen, k, 0, 0, 0, 0, name="window == contig"),
            placed(1703, clen, k, 20, 30, 30, 20, max_lead=1 << 20, max_trail=1 << 20, name="max cuts beyond the window"),
            placed(1704, clen, k, 0, 60, 60, 0, max_lead=1 << 30, max_trail=1 << 30, name="max cuts far beyond, cuts 0")]
    return add_ballast(loci, k), opts_for(k, clen)


def n_window_loci(k=15, clen=40):
    """an 'N' in the window inside the 10-mer that would be the first / the last hit: the scans take the next one"""
    def put(pos, byte=b"N"):
        return lambda c: c[:pos] + byte + c[pos + 1:]
    loci = []
    for n, d in enumerate((0, 52, 54, 55)):
        # first hit moves from p to p + 4 (the first 10-mer clear of window position p + 3)
        l = placed(1800 + n, clen, k, 20, d, 30, 20, edit=put(3), name="N in the first hit, d=%d" % d)
        assert l.trims == [(20 + d + 4, 50)], l.trims
        loci.append(l)
        l = placed(1850 + n, clen, k, 20, 30, d, 20, edit=put(clen - 4), name="N in the last hit, d=%d" % d)
        assert l.trims == [(50, 20 + d + 4)], l.trims
        loci.append(l)
    l = placed(1890, clen, k, 20, 30, 30, 20, edit=lambda c: c[:3] + b"N" + c[4:clen - 4] + b"N" + c[clen - 3:], name="N in both")
    assert l.trims == [(54, 54)]
    loci.append(l)
    return add_ballast(loci, k), opts_for(k, clen)


def contig_length_loci(lengths=CONTIG_LENGTHS, k=10):
    """one locus per contig length (table-size steps, ceil(len / 64) E-bucket steps, the LDS / global table switch at 512 / 513); word
    length 10 so that the 10- and 11-base contigs assemble"""
    loci = [placed(2000 + n, clen, k, 20, 7 + n % 5, 3 + n % 7, 20, name="contig of %d" % clen) for n, clen in enumerate(lengths)]
    return add_ballast(loci, k), asm_opts(minWordLength=k, maxWordLength=k, minContigLength=10, minCoverage=BALLAST_COVERAGE)


def long_contig_loci(k=15):
    """reads of 1024 and 1025 bases"""
    loci = [placed(2050 + n, clen, k, 20, 7, 5, 20, name="contig of %d" % clen) for n, clen in enumerate((1024, 1025))]
    return loci, opts_for(k, 1024)


POOL_SWEEP = [512 + 400 * n for n in range(17)]


def pool_share_loci(windows=POOL_SWEEP, seed0=2250, k=15, clen=40):
    """Equal piles (equal graphs, so equal shares of the pool's LDS), one per window length.  The pool's epilogue takes a locus while
    schedStagedBytes(contig, window) fits the share behind the 4 KB table and leaves it beyond (asm_contig.hpp: scheduleEpilogue).  The
    share's size follows the graph kernel's node and set counts and is not restated here: a coarse sweep (POOL_SWEEP, 400-base steps)
    brackets the step from the routing counts, and the test then runs the bracket again in 16-base steps, so that windows on both sides
    of the real step, and at it, are run.  The step itself is benign by construction -- scheduleContig checks bytesC + bytesR <=
    lseqBytes again with the texts' real alignment and reads them from global memory otherwise, so an off-by-16 in the epilogue's bound
    moves the routing, not a result; what the sweep pins is that results on both sides equal the oracle."""
    loci = [placed(seed0 + n, clen, k, 100, 120, w - 100 - 120 - clen - 100, 100, name="pool share, window of %d" % w)
            for n, w in enumerate(windows)]
    assert [len(l.ref) for l in loci] == list(windows)
    return add_ballast(loci, k), opts_for(k, clen)


def staged_bytes(clen, ref_size):
    """smallsv_trim.hpp: schedStagedBytes"""
    return ((clen + 30) & ~15) + ((ref_size + 30) & ~15)


def staging_alignment_loci(k=15, L=300, c0=40):
    """sixteen loci whose window lengths are L .. L+15 and whose contig lengths step by one too: in one batch the texts' offsets in the
    window arena and in the text arena take every residue mod 16"""
    loci = []
    for j in range(16):
        clen = c0 + j
        pre = 60
        loci.append(placed(2100 + j, clen, k, 20, pre - 20, L + j - pre - clen - 20, 20, name="window of %d, contig of %d" % (L + j, clen)))
        assert len(loci[-1].ref) == L + j
    return add_ballast(loci, k), opts_for(k, c0)


def staging_capacity_loci(k=15, clen=100):
    """contig + window either side of SCHED_SEQ_BYTES from schedStagedBytes' formula: the largest window that is staged whatever the
    texts' addresses, the windows around the step, and windows that are read from global memory whatever the addresses"""
    units = SCHED_SEQ_BYTES - ((clen + 30) & ~15)  # bytes left for the window's units
    top = units - 30 + 15  # largest refSize with ((refSize + 30) & ~15) <= units
    assert staged_bytes(clen, top) == SCHED_SEQ_BYTES and staged_bytes(clen, top + 1) == SCHED_SEQ_BYTES + 16
    loci = []
    for n, ref_size in enumerate((top - 16, top - 1, top, top + 1, top + 15, top + 16, top + 17, top + 40)):
        loci.append(placed(2200 + n, clen, k, 100, 120, ref_size - 100 - 120 - clen - 100, 100, name="window of %d (step at %d)" % (ref_size, top)))
        assert len(loci[-1].ref) == ref_size
    return loci, opts_for(k, clen)


# ---- several contigs per locus ------------------------------------------------------------------------------------------------------
def multi_locus(seed, lens, k, gaps, lead_cut=20, trail_cut=20, counts=(7, 6, 5), name=""):
    """window = flank, contig 0, flank, contig 1, ...: each contig has its own first and last hit.  gaps: len(lens) + 1 flank lengths
    (behind leadingCut / in front of the trailing cut for the outer ones)"""
    rng = random.Random(seed)
    contigs = []
    for n in lens:
        contigs.append(rand_contig(rng, n, k, avoid=contigs))
    # (no word of one group may continue into another: the first k-1 and last k-1 bases of different contigs share no k-1-mer)
    km = [set(c[i:i + k - 1] for i in range(len(c) - k + 2)) for c in contigs]
    assert all(not (km[a] & km[b]) for a in range(len(km)) for b in range(a)), name
    ref, want_at = rand_flank(rng, lead_cut + gaps[0], contigs), []
    for c, g in zip(contigs, gaps[1:]):
        want_at.append(len(ref))
        ref += c + rand_flank(rng, g, contigs)
    ref += rand_flank(rng, trail_cut, contigs)
    want = [(at, len(ref) - at - len(c)) for at, c in zip(want_at, contigs)]
    return Locus(pile(contigs, counts), ref, (lead_cut, trail_cut, len(ref), len(ref)), contigs, want, name or "multi %d" % seed)


def multi_contig_loci(k=15):
    loci = [multi_locus(2300, (40, 45), k, (5, 60, 9), name="two contigs"),
            multi_locus(2301, (40, 70, 130), k, (55, 3, 56, 110), name="three contigs, three buckets"),
            multi_locus(2302, (64, 65, 33), k, (0, 0, 0, 0), name="three contigs back to back")]
    return add_ballast(loci, k), opts_for(k, 33)


def pending_loci(k=15):
    """contigs per bucket around SCHED_PEND (8): 8, 9, 16 and 17 contigs of one bucket, then a mix over three buckets -- each set a run of
    its own, three contigs per locus at most.  Contigs of 40 to 130 bases land in E buckets that run on align_pair_kernel with these
    scores: bucket_sort_kernel rebuilds their lists from the per-slot records, and only the COUNTS schedFlush adds up are read.  The
    runs of 400-base contigs land in the E = 8 bucket, which does not pair (align_pair.hpp: E <= 6): its aligner reads the lists
    schedFlush wrote -- the full flush of eight, the second one behind it at pos 8, the partial one at the end."""
    def run(seed, lens):
        out = []
        for j in range(0, len(lens), 3):
            out.append(multi_locus(seed + j, lens[j:j + 3], k, (3, 4, 5, 6)[:len(lens[j:j + 3]) + 1], name="pending %d+%d" % (seed, j)))
        return out
    sets = [run(2400, [40] * 8), run(2500, [41] * 9), run(2600, [42] * 16), run(2700, [43] * 17),
            run(2800, [40, 70, 130] * 6 + [40, 40, 40]),
            run(6000, [400] * 8), run(6100, [401] * 9), run(6200, [402] * 16), run(6300, [403] * 17)]
    return sets, opts_for(k, 40)


def bucket_sort_loci(n, k=15, n_long=12):
    """n one-contig loci of 5 x 40-base reads.  The window holds the contig's halves `g` bases apart (the trim keeps 40 + g bases: the
    sort's classes are window lengths / 8; g repeats, so several windows are equally long); about a dozen windows stay longer than 4088
    bases (the class saturates at 511 x 8)"""
    loci = []
    for j in range(n):
        rng = random.Random(3000 + j)
        contig = rand_contig(rng, 40, k)
        if j % max(1, n // n_long) == 7:
            # (the trim is given no room: maxLeadingCut / maxTrailingCut at the cuts, so the aligned window stays above 4088 bases)
            ref = rand_flank(rng, 30, [contig]) + contig + rand_flank(rng, 4100 + 8 * (j % 5), [contig])
            loci.append(Locus(pile([contig]), ref, (20, 20, 20, 20), [contig], [(21, 20)], "long window %d" % j))
            assert len(ref) - 41 > 4088
        else:
            g, pre, post = (j * 13) % 97, 20 + rng.choice((0, 3, 11)), 20 + (j * 7) % 24
            ref = rand_flank(rng, pre, [contig]) + contig[:20] + rand_flank(rng, g, [contig]) + contig[20:] + rand_flank(rng, post, [contig])
            loci.append(Locus(pile([contig]), ref, (20, 20, len(ref), len(ref)), [contig], [(pre, post)], "sorted %d" % j))
    return loci, opts_for(k, 40)


# ---- bytes outside ACGTN in the trim ------------------------------------------------------------------------------------------------
JUNK = (b"R", b"a", b"=", b"\xe9")


def junk_locus(seed, clen, k, at, window_bytes=None, lower=False, name="", cuts=(20, 20, 300, 300), post_len=190):
    """contig with the bytes `at` = {position: byte}; the window's copy carries `window_bytes` = {position: byte} there instead (default:
    the same bytes).  lower: the whole pile in lower case.
      A word with such a byte is no successor or predecessor candidate of a pure word (only A, C, G, T extend a contig), so the pile
    yields the whole read only when the SEED holds every such byte: the seed is the lexicographically smallest of the equally frequent
    words (IterativeAssembler.cpp:689-696).  The contig is drawn again until that is so."""
    rng = random.Random(seed)
    first = max(0, min(min(at, default=0) - 3, clen - k))  # the word meant as the seed: it starts with "AAA" (or with the byte itself)
    for _ in range(2000):
        contig = bytearray(rand_seq(rng, clen))
        contig[first:first + 3] = b"AAA"
        if first:
            contig[first - 1:first] = b"C"
        if lower:
            contig = bytearray(bytes(contig).lower())
        for p, b in at.items():
            contig[p] = b[0]
        contig = bytes(contig)
        words = [contig[i:i + k] for i in range(clen - k + 1)]
        i = words.index(min(words))
        if kmers_unique(contig, MER) and all(i <= p < i + k for p in (range(clen) if lower else at)):
            break
    else:
        raise AssertionError("no contig whose seed holds the bytes: " + name)
    body = bytearray(contig)
    for p, b in (window_bytes or {}).items():
        body[p] = b[0]
    pre, post = rand_flank(rng, 150, [contig]), rand_flank(rng, post_len, [contig])
    ref = pre + bytes(body) + post
    return Locus(pile([contig]), ref, cuts, [contig], None, name or "junk %d" % seed)


def junk_loci(k=15):
    """-> (loci, opts): every junk byte at every position class, against windows that carry the same byte, another junk byte, 'N' and
    the plain base there; plain loci in between (a batch that mixes both forms of the table)"""
    loci, seed = [], 4000
    for b in JUNK:
        for clen, pos in ((60, 3), (60, 56), (60, 30), (19, 9)):
            other = JUNK[(JUNK.index(b) + 1) % len(JUNK)]
            for wname, wb in (("same", None), ("other junk", {pos: other}), ("N", {pos: b"N"}), ("plain", {pos: b"ACGT"[seed % 4:seed % 4 + 1]})):
                seed += 1
                # (19 bases: every 10-mer spans the byte, and a window with another byte there has no hit at all.  Scans that end 5
                # bases into the copy from either side keep the reference's own range positive)
                cuts = (20, 20, 300, 300) if clen > 19 else (20, 20, 155, 205)
                loci.append(junk_locus(seed, clen, k, {pos: b}, wb, name="%r at %d of %d, window %s" % (b, pos, clen, wname), cuts=cuts))
        loci.append(placed(seed + 500, 60, k, 20, 130, 170, 20, name="plain between junk"))
    loci.append(junk_locus(4900, 60, k, {3: b"R", 10: b"a"}, None, name="two junk bytes"))
    loci.append(junk_locus(4901, 60, k, {3: b"R", 10: b"a"}, {3: b"a", 10: b"R"}, name="two junk bytes, swapped in the window"))
    # (a lower-case pile extends nothing: its contigs are single words.  One word per read keeps the contig under the test's control)
    loci.append(junk_locus(4902, k, k, {}, None, lower=True, name="all lower case"))
    loci.append(junk_locus(4903, k, k, {}, {0: b"A"}, lower=True, name="all lower case, one upper-case base in the window"))
    loci.append(junk_locus(4904, 600, k, {300: b"R"}, None, name="junk in a contig beyond 512 bases (global table)"))
    # (contig + window beyond SCHED_SEQ_BYTES: table build and lookups read the texts from global memory)
    loci.append(junk_locus(4905, 60, k, {30: b"R"}, None, name="junk next to a window that is not staged", post_len=6200))
    assert staged_bytes(60, len(loci[-1].ref)) - 32 > SCHED_SEQ_BYTES
    loci.append(junk_collision_locus(k))
    return loci, asm_opts(minWordLength=k, maxWordLength=k, minContigLength=15)


def mer_slot(mer, clen):
    """smallsv_trim.hpp: merHashBytes and the table size of a contig of `clen` bases -> the 10-mer's home slot"""
    h = 2166136261
    for b in mer:
        h = ((h ^ b) * 16777619) & 0xffffffff
    h ^= h >> 15
    cap = 64
    while cap < 2 * clen:
        cap <<= 1
    return h & (cap - 1)


def junk_collision_locus(k=15, clen=60):
    """The byte compare behind the hash.  The contig's first 10-mer ends on an 'R'; the window carries an 'a' there.  That window
    10-mer, equal in its first nine bytes, probes from a home slot from which every slot up to the contig 10-mer's own home is taken:
    linear probing then leads its lookup to the contig's entry whatever the order the table was filled in (the set of taken slots does
    not depend on it), and only the comparison of all ten bytes tells them apart.  The true first hit is ten positions later.  (The
    seed is searched; the hash is restated above.)"""
    for seed in range(4950, 4950 + 5000):
        l = junk_locus(seed, clen, k, {9: b"R"}, {9: b"a"}, name="probe chain to a 10-mer that differs in its last byte (seed %d)" % seed)
        c = l.contigs[0]
        cap, taken = 64, set()
        while cap < 2 * clen:
            cap <<= 1
        for m in sorted({c[i:i + MER] for i in range(clen - MER + 1)}):
            at = mer_slot(m, clen)
            while at in taken:
                at = (at + 1) % cap
            taken.add(at)
        home, probe = mer_slot(c[:MER], clen), mer_slot(c[:9] + b"a", clen)
        dist = (home - probe) % cap
        if 0 < dist <= 8 and all((probe + j) % cap in taken for j in range(dist)):
            assert l.trims == [(160, 190)]
            return l
    raise AssertionError("no seed with such a probe chain")


def issue_reproducer(k=15):
    """the three cases of the issue: an 'R' at byte 3 and at byte 56 of a 60-base contig cut out of the window, and at byte 9 of a
    19-base one -> (loci, opts, (lead, trail, cigar) per locus)"""
    out = []
    for pos, clen in ((3, 60), (56, 60), (9, 19)):
        l = junk_locus(77, clen, k, {pos: b"R"}, None, name="issue: R at %d of %d" % (pos, clen))
        assert l.trims == [(150, 190)]
        out.append(l)
    return out, asm_opts(minWordLength=k, maxWordLength=k, minContigLength=15), [(150, 190, "60="), (150, 190, "60="), (150, 190, "19=")]


# ---- spanning ----------------------------------------------------------------------------------------------------------------------
class SpanLocus:
    def __init__(self, reads, ref1, ref2, cuts, contigs, name=""):
        self.reads, self.ref1, self.ref2, self.cuts, self.contigs, self.name = reads, ref1, ref2, tuple(cuts), list(contigs), name

    @property
    def triple(self):
        return (self.reads, self.ref1, self.ref2)


def jump_contig(ref1, ref2, j1, j2, insert, left=40, right=40):
    """ref1[j1-left:j1] + insert + ref2[j2:j2+right]"""
    assert j1 - left >= 0 and j2 + right <= len(ref2)
    return ref1[j1 - left:j1] + insert + ref2[j2:j2 + right]


def span_locus(seed, dists, inserts, k=15, left=40, right=40, w=200, name="", cuts=None):
    """One locus, one contig per entry of `dists` = (e1, e2) / `inserts`: contig c joins reference 1 at j1 and reference 2 at j2 so that
    ref1EndPos - align1EndPos = e1 and begin2 = e2 on the CUT references, i.e. the junction lies e1 + 1 bases before the trailing cut
    of reference 1 and e2 bases behind the leading cut of reference 2.  All contigs share the cuts, so they take different junctions:
    `dists` are given relative to ONE pair of cuts and the windows are long enough for every contig's flanks."""
    rng = random.Random(seed)
    while True:
        ref1, ref2 = rand_seq(rng, w), rand_seq(rng, w)
        if kmers_unique(ref1 + b"N" + ref2, 12):
            break
    if cuts is None:
        cuts = (10, 60, 60, 10)
    a1l, a1t, a2l, a2t = cuts
    contigs = []
    ref1, ref2 = bytearray(ref1), bytearray(ref2)
    for (e1, e2), ins_len in zip(dists, inserts):
        j1 = (w - a1l - a1t - 1) - e1 + a1l  # align1EndPos = j1 - a1l
        j2 = a2l + e2
        if ins_len == 0:
            # (a junction without insert is placed uniquely: the bases next to it, outside the contig, continue neither flank)
            ref1[j1] = b"ACGT"[(b"ACGT".index(ref2[j2]) + 1) % 4]
            ref2[j2 - 1] = b"ACGT"[(b"ACGT".index(ref1[j1 - 1]) + 1) % 4]
        # (no base of the insert continues either flank: it differs from the base of reference 1 and of reference 2 it would lie on)
        ins = bytes(rng.choice([x for x in b"ACGT" if x != ref1[j1 + i] and x != ref2[j2 - ins_len + i]]) for i in range(ins_len))
        c = jump_contig(bytes(ref1), bytes(ref2), j1, j2, ins, left, right)
        assert kmers_unique(c, k), name
        contigs.append(c)
    km = [set(c[i:i + k - 1] for i in range(len(c) - k + 2)) for c in contigs]
    assert all(not (km[a] & km[b]) for a in range(len(km)) for b in range(a)), (name, "the contigs' flanks overlap")
    ref1, ref2 = bytes(ref1), bytes(ref2)
    assert all(inserts) or len(contigs) == 1  # (the bases changed above may lie in another contig's flank)
    return SpanLocus(pile(contigs), ref1, ref2, cuts, contigs, name or "span %d" % seed)
