#!/usr/bin/env python3
"""Records the reference's GlobalJumpIntronAligner<int> outputs (run on the authoring machine only; needs the reference tree).

Writes
  tests/golden/intron_aligner_reference_tests.json   the 16 cases of alignment/test/GlobalJumpIntronAlignerTest.cpp: inputs, the scores of
                                                     the test file's three helper functions, every BOOST_REQUIRE* expectation parsed from the
                                                     source, and the reference's full output text for ScoreType int (what Manta instantiates;
                                                     the test file itself uses short -- `ref_text_short` is stored where the two differ)
  tests/golden/intron_aligner_cases.json.xz          generated cases (tests/intron_cases.py): spec + scores + output text, no sequences

The reference is run through a small driver of this project's own (DRIVER below), compiled against the reference's headers into a
temporary directory outside the repository; neither reference text nor the binary is kept.  Nothing but this script ever does that:
build(), the tests, smoke() and bench.py only read the two files.
"""
import json
import lzma
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import intron_cases  # noqa: E402

REF = os.environ.get("MANTA_REFERENCE", "/root/reference")
LIB = os.path.join(REF, "src/c++/lib")
TEST_SRC = os.path.join(LIB, "alignment/test/GlobalJumpIntronAlignerTest.cpp")

# input: u32 n, then per case 8 x i32 (match mismatch open extend offEdge jump intronOpen intronOffEdge), u32 flags (1 ref1Fw, 2 ref2Fw,
# 4 stranded), 3 x u32 lengths, the three sequences.  output: one line per case; per-case seconds on stderr.
DRIVER = r"""
#include "alignment/GlobalJumpIntronAligner.hpp"
#include "blt_util/align_path.hpp"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
template <typename T> static void run(FILE* f, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    int32_t s[8]; uint32_t h[4];
    if (fread(s, 4, 8, f) != 8 || fread(h, 4, 4, f) != 4) { fprintf(stderr, "short input\n"); exit(2); }
    std::string q(h[1], 0), r1(h[2], 0), r2(h[3], 0);
    if ((h[1] && fread(&q[0], 1, h[1], f) != h[1]) || (h[2] && fread(&r1[0], 1, h[2], f) != h[2]) || (h[3] && fread(&r2[0], 1, h[3], f) != h[3])) exit(2);
    AlignmentScores<T> scores(s[0], s[1], s[2], s[3], s[4]);
    GlobalJumpIntronAligner<T> aligner(scores, T(s[5]), T(s[6]), T(s[7]));
    JumpAlignmentResult<T> res;
    const auto t0 = std::chrono::steady_clock::now();
    aligner.align(q.begin(), q.end(), r1.begin(), r1.end(), r2.begin(), r2.end(), (h[0] & 1) != 0, (h[0] & 2) != 0, (h[0] & 4) != 0, res);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("score %d align1 %d:%s align2 %d:%s jumpInsertSize %u jumpRange %u\n", int(res.score), int(res.align1.beginPos),
           ALIGNPATH::apath_to_cigar(res.align1.apath).c_str(), int(res.align2.beginPos), ALIGNPATH::apath_to_cigar(res.align2.apath).c_str(),
           unsigned(res.jumpInsertSize), unsigned(res.jumpRange));
    fprintf(stderr, "%.6f\n", sec);
  }
}
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  uint32_t n = 0;
  if (!f || fread(&n, 4, 1, f) != 1) return 2;
  if (argc > 2 && !strcmp(argv[2], "short")) run<short>(f, n); else run<int>(f, n);
  return 0;
}
"""


class Reference:
    def __init__(self):
        self.tmp = tempfile.TemporaryDirectory(prefix="intron_ref_")
        src = os.path.join(self.tmp.name, "driver.cpp")
        open(src, "w").write(DRIVER)
        self.exe = os.path.join(self.tmp.name, "driver")
        shim = os.path.join(ROOT, "oracle", "ref_shim")
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-DNDEBUG", "-I", shim, "-I", LIB, src, os.path.join(LIB, "blt_util/align_path.cpp"),
                               os.path.join(LIB, "blt_util/blt_exception.cpp"), os.path.join(LIB, "alignment/Alignment.cpp"),
                               os.path.join(shim, "parse_util_shim.cpp"), "-o", self.exe])

    def run(self, cases, short=False):
        """cases: (scores8, flags, q, r1, r2) -> (list of output lines, list of seconds)"""
        path = os.path.join(self.tmp.name, "in.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for sc, flags, q, r1, r2 in cases:
                f.write(struct.pack("<8iIIII", *sc, flags, len(q), len(r1), len(r2)))
                f.write(q + r1 + r2)
        p = subprocess.run([self.exe, path] + (["short"] if short else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        return p.stdout.decode().splitlines(), [float(x) for x in p.stderr.decode().split()]


def strip_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def bodies(src, pattern):
    for m in re.finditer(pattern, src):
        depth, i = 1, m.end()
        while depth:
            depth += (src[i] == "{") - (src[i] == "}")
            i += 1
        yield m, src[m.end():i - 1], src[:m.start()].count("\n") + 1


def parse_reference_tests():
    src = strip_comments(open(TEST_SRC).read())
    # the helpers: each forwards to testAlignScores(seq, ref1, ref2, match, mismatch, open, extend, spliceOpen, offEdge, spliceOffEdge, jump,
    # stranded, bp1Fw, bp2Fw) with literals or its own `stranded` / `fw` parameters (defaults true)
    helpers = {}
    for m, body, _ in bodies(src, r"static\s+JumpAlignmentResult<score_t>\s+(\w+)\s*\(([^)]*)\)\s*\{"):
        call = re.search(r"return\s+testAlignScores\(([^;]*)\);", body)
        if call:
            helpers[m.group(1)] = [a.strip() for a in call.group(1).split(",")][3:]
    assert sorted(helpers) == ["testAlign", "testAlignSplice", "testAlignSpliceNoJump"], helpers
    cases = []
    for m, body, line in bodies(src, r"BOOST_AUTO_TEST_CASE\((\w+)\)\s*\{"):
        seqs = dict(re.findall(r"static const std::string (\w+)\(\"([^\"]*)\"\);", body))
        call = re.search(r"result\s*=\s*(\w+)\(([^;]*)\);", body)
        args = [a.strip() for a in call.group(2).split(",")]
        env = {"stranded": "true", "fw": "true"}
        for k, v in zip(("stranded", "fw"), args[3:]):
            env[k] = v
        vals = [env.get(a, a) for a in helpers[call.group(1)]]
        match, mismatch, open_, extend, splice_open, off_edge, splice_off_edge, jump = (int(v) for v in vals[:8])
        stranded, fw1, fw2 = (v == "true" for v in vals[8:])
        expect = {}
        for em in re.finditer(r"BOOST_REQUIRE_EQUAL\(\s*(.+?),\s*([^;]+?)\s*\);", body):
            lhs, rhs = em.group(1).strip(), em.group(2).strip()
            m2 = re.match(r"apath_to_cigar\(result\.align(\d)\.apath\)", lhs)
            key = ("cigar" + m2.group(1)) if m2 else None
            m2 = re.match(r"result\.align(\d)\.beginPos", lhs)
            key = key or (("begin" + m2.group(1)) if m2 else None)
            if key is None and lhs in ("result.score", "result.jumpInsertSize", "result.jumpRange"):
                key = lhs.split(".")[1]
            if key is None:
                raise SystemExit("unparsed expectation in %s: %s" % (m.group(1), lhs))
            if rhs.startswith('"'):
                expect[key] = rhs.strip('"')
            else:
                assert re.fullmatch(r"[-+*\d\su ]+", rhs), rhs
                expect[key] = int(eval(rhs.replace("u", "")))
        assert "BOOST_REQUIRE(" not in body and "BOOST_CHECK" not in body
        cases.append(dict(source="%s:%d" % (os.path.relpath(TEST_SRC, REF), line), name=m.group(1), helper=call.group(1),
                          scores=[match, mismatch, open_, extend, off_edge, 0], jump=jump, intron_open=splice_open,
                          intron_off_edge=splice_off_edge, ref1_fw=fw1, ref2_fw=fw2, stranded=stranded, query=seqs[args[0]], ref1=seqs[args[1]],
                          ref2=seqs[args[2]], expect=expect))
    assert len(cases) == 16, len(cases)
    return cases


def flags_of(c):
    return (1 if c["ref1_fw"] else 0) | (2 if c["ref2_fw"] else 0) | (4 if c["stranded"] else 0)


def scores8(c):
    return c["scores"][:5] + [c["jump"], c["intron_open"], c["intron_off_edge"]]


RNA = dict(scores=[2, -8, -19, -1, -1, 0], jump=-100, intron_open=-15, intron_off_edge=-1)  # options/SVRefinerOptions.hpp:46-49
TEST = dict(scores=[2, -4, -5, -1, -1, 0], jump=-3, intron_open=-4, intron_off_edge=-1)     # the reference test file's testAlignSplice
STRANDS = [dict(ref1_fw=True, ref2_fw=True, stranded=True), dict(ref1_fw=False, ref2_fw=False, stranded=True),
           dict(ref1_fw=True, ref2_fw=True, stranded=False), dict(ref1_fw=True, ref2_fw=False, stranded=True),
           dict(ref1_fw=False, ref2_fw=True, stranded=True)]


def generated_cases():
    import numpy as np
    rs = np.random.RandomState(20240611)
    out = []
    seed = [1000]

    def add(family, tier, spec, sc, strand):
        seed[0] += 1
        c = dict(family=family, tier=tier, spec=dict(spec, seed=seed[0]))
        c.update(sc)
        c.update(strand)
        out.append(c)

    def rand_scores():
        return dict(scores=[int(rs.randint(1, 4)), -int(rs.randint(1, 9)), -int(rs.randint(0, 20)), -int(rs.randint(0, 3)), -int(rs.randint(0, 3)), 0],
                    jump=-int(rs.randint(0, 40)), intron_open=-int(rs.randint(0, 16)), intron_off_edge=-int(rs.randint(0, 3)))

    def ref(exons, introns, motif, lflank=None, rflank=None, **kw):
        return dict(exons=exons, introns=introns, motif=motif, lflank=int(rs.randint(0, 30)) if lflank is None else lflank,
                    rflank=int(rs.randint(0, 30)) if rflank is None else rflank, **kw)

    def ex(n, lo=8, hi=30):
        return [int(rs.randint(lo, hi)) for _ in range(n)]

    # (a) short, planted canonical and wrong-strand introns in ref1, ref2, both, with and without a jump
    for strand in STRANDS:
        for motif in ("fw", "rev", "none", "half"):
            for use, n1, n2 in (("1", 2, 1), ("2", 1, 2), ("12", 2, 2), ("12", 3, 1), ("12", 1, 1)):
                for sc in (TEST, RNA):
                    add("a", "cpu", dict(ref1=ref(ex(n1), ex(n1 - 1, 6, 40), motif), ref2=ref(ex(n2), ex(n2 - 1, 6, 40), motif), use=use,
                                         subst=int(rs.randint(0, 2)), jump_insert=int(rs.randint(0, 2)) * int(rs.randint(1, 5))), sc, strand)
    # (b) random score sets on planted cases (the RNA defaults are used throughout the other families)
    for i in range(60):
        add("b", "cpu", dict(ref1=ref(ex(2), ex(1, 4, 30), ["fw", "rev"][i & 1]), ref2=ref(ex(2), ex(1, 4, 30), ["fw", "rev"][(i >> 1) & 1]),
                             use=["12", "1", "2"][i % 3], subst=int(rs.randint(0, 3)), indel=int(rs.randint(0, 2))), rand_scores(), STRANDS[i % 5])
    # (c) motifs at a reference's first / last two bases, introns running off either edge, and off-edge ties
    for strand in STRANDS:
        for sc in (TEST, RNA, dict(RNA, intron_open=-3), dict(TEST, scores=[2, -4, -5, -1, -2, 0], intron_off_edge=-2)):
            e, it = ex(2, 10, 20), ex(1, 8, 20)
            for lt in (0, e[0], e[0] + 1, e[0] + 2, e[0] + it[0] - 3, e[0] + it[0] - 2, e[0] + it[0] - 1):  # left edge inside / at the intron
                add("c", "cpu", dict(ref1=ref(e, it, "fw", lflank=0, ltrim=lt), ref2=ref(ex(1), [], "fw"), use="1"), sc, strand)
                add("c", "cpu", dict(ref1=ref(ex(1), [], "fw"), ref2=ref(e, it, "rev", lflank=0, ltrim=lt), use="2"), sc, strand)
            for rt in (0, e[1], e[1] + 1, e[1] + 2, e[1] + it[0] - 2, e[1] + it[0] - 1):  # right edge
                add("c", "cpu", dict(ref1=ref(e, it, "fw", rflank=0, rtrim=rt), ref2=ref(ex(1), [], "fw"), use="1"), sc, strand)
                add("c", "cpu", dict(ref1=ref(ex(1), [], "fw"), ref2=ref(e, it, "fw", rflank=0, rtrim=rt), use="2"), sc, strand)
    for i in range(400):  # plain random sequences over few letters: chance motifs everywhere, many ties with small scores
        sc = rand_scores() if i % 4 else [TEST, RNA][(i >> 2) & 1]
        add("c", "cpu", dict(random=[int(rs.randint(1, 24)), int(rs.randint(1, 30)), int(rs.randint(1, 30))], alphabet=["AGT", "ACGT", "ACT", "AG"][i % 4]),
            sc, STRANDS[i % 5])
    # (d) N, lower case and arbitrary bytes; lower-case gt..ag must not splice
    for i, strand in enumerate(STRANDS):
        for motif in ("lower", "lowrev", "fw"):
            add("d", "cpu", dict(ref1=ref(ex(2), ex(1, 6, 30), motif), ref2=ref(ex(2), ex(1, 6, 30), motif), use="12"), [TEST, RNA][i & 1], strand)
            add("d", "cpu", dict(ref1=ref(ex(2), ex(1, 6, 30), motif), ref2=ref(ex(1), [], motif), use="1", alphabet="ACGTN", subst=3, noise="NX\x00\xff"),
                RNA, strand)
            add("d", "cpu", dict(ref1=ref(ex(2), ex(1, 6, 30), motif), ref2=ref(ex(2), ex(1, 6, 30), motif), use="12", alphabet="ACGTacgtN", lower_query=(i & 1) == 1),
                TEST, strand)
        add("d", "cpu", dict(random=[20, 40, 40], alphabet="".join(chr(b) for b in range(256))), RNA, strand)
    # (e) several query columns per lane, and strips
    for i, qlen in enumerate((65, 66, 127, 128, 129, 200, 257, 320, 385, 420, 640, 1100, 2049, 2100, 4200)):
        n = 3
        e = [qlen // n + (1 if k < qlen % n else 0) for k in range(n)]
        add("e", "cpu", dict(ref1=ref(e[:2], ex(1, 20, 60), ["fw", "rev"][i & 1]), ref2=ref(e[2:], [], "fw"), use="12", subst=int(rs.randint(0, 6)),
                             indel=int(rs.randint(0, 3))), RNA, STRANDS[i % 5])
    # references beyond 16-bit rows (a short query keeps the emulator affordable)
    add("rows", "cpu", dict(ref1=ref([12, 14], [40000], "fw", lflank=300, rflank=200), ref2=ref([15], [], "fw", lflank=30100, rflank=50), use="12"),
        RNA, STRANDS[0])
    add("rows", "cpu", dict(ref1=ref([16], [], "fw", lflank=100, rflank=50), ref2=ref([12, 14], [66000], "rev", lflank=300, rflank=200), use="12"),
        RNA, STRANDS[3])
    # (f) RNA-shaped: two reduced cases for the emulator, the rest at full size
    add("f", "cpu", dict(ref1=ref([60, 50], [1500], "fw", lflank=700, rflank=400), ref2=ref([40], [], "fw", lflank=900, rflank=1500), use="12", subst=2),
        RNA, STRANDS[0])
    add("f", "cpu", dict(ref1=ref([70], [], "rev", lflank=1200, rflank=900), ref2=ref([50, 30], [1100], "rev", lflank=500, rflank=800), use="12", subst=2),
        RNA, STRANDS[1])
    for i in range(12):
        q = int(rs.randint(150, 601))
        two = bool(i & 1)
        cut = sorted(int(x) for x in rs.randint(30, q - 30, size=3 if two else 2))
        e1 = [cut[0], cut[1] - cut[0]] + ([cut[2] - cut[1]] if two else [])
        i1 = [int(rs.randint(1000, 20001)) for _ in range(len(e1) - 1)]
        w1, w2 = int(rs.randint(5000, 50001)), int(rs.randint(5000, 50001))
        pad1 = max(w1 - sum(e1) - sum(i1), 200)
        e2 = [q - cut[-1]]
        lf1, lf2 = int(rs.randint(50, pad1 - 50)), int(rs.randint(50, w2 - e2[0] - 50))
        motif = ["fw", "rev"][i % 2] if i < 10 else "none"
        add("f", "gpu", dict(ref1=ref(e1, i1, motif, lflank=lf1, rflank=pad1 - lf1), ref2=ref(e2, [], "fw", lflank=lf2, rflank=w2 - e2[0] - lf2),
                             use="12", subst=int(rs.randint(0, 8)), indel=int(rs.randint(0, 3))), RNA, STRANDS[i % 5])
    return out


def main():
    ref = Reference()
    tests = parse_reference_tests()
    inputs = [(scores8(c), flags_of(c), c["query"].encode(), c["ref1"].encode(), c["ref2"].encode()) for c in tests]
    as_int, _ = ref.run(inputs)
    as_short, _ = ref.run(inputs, short=True)
    differ = 0
    for c, a, b in zip(tests, as_int, as_short):
        c["ref_text"] = a
        if a != b:
            c["ref_text_short"] = b
            differ += 1
    json.dump(tests, open(os.path.join(HERE, "intron_aligner_reference_tests.json"), "w"), indent=1)
    print("reference test cases: %d (%d differ between int and short)" % (len(tests), differ))

    cases = generated_cases()
    seqs = [intron_cases.make_case(c["spec"]) for c in cases]
    lines, secs = ref.run([(scores8(c), flags_of(c), q, r1, r2) for c, (q, r1, r2) in zip(cases, seqs)])
    assert len(lines) == len(cases)
    cells = sec = 0.0
    for c, (q, r1, r2), line, s in zip(cases, seqs, lines, secs):
        c["lens"] = [len(q), len(r1), len(r2)]
        c["digest"] = intron_cases.digest(q, r1, r2)
        c["ref_text"] = line
        if c["family"] == "f" and c["tier"] == "gpu":
            cells += len(q) * (len(r1) + len(r2))
            sec += s
    out = os.path.join(HERE, "intron_aligner_cases.json.xz")
    with lzma.open(out, "wt") as f:
        json.dump(cases, f, separators=(",", ":"))
    fam = {}
    for c in cases:
        fam[c["family"]] = fam.get(c["family"], 0) + 1
        if "N" in c["ref_text"]:
            fam[c["family"] + " with N"] = fam.get(c["family"] + " with N", 0) + 1
    print("generated cases: %d %s, %d bytes" % (len(cases), json.dumps(fam, sort_keys=True), os.path.getsize(out)))
    print("reference, family (f) at full size, one thread: %.3g cells in %.2f s = %.3g cells/s" % (cells, sec, cells / sec))


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("%.1f s" % (time.time() - t0))
