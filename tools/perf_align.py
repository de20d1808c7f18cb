"""Quick aligner throughput probe (GPU box): config-2 shaped LargeIndel alignments, contig ~270 bp vs ~1.5 kb.

`perf_align.py --intron [n]`: the RNA shape instead (query 150-600, two windows of 5-50 kb, one or two introns of 1-20 kb; n >= 256
alignments): GlobalJumpIntronAligner (align_kernel<3, E>) and, on the same sequences in the same process, alternated run by run,
GlobalJumpAligner on its int32 kernel (align_kernel<2, E>; the packed pairs are switched off), both host-timed with staging inside the clock."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from manta_amd._capi import Lib
from synth import rand_seq, mutate



def intron_leg(n):
    os.environ["MANTA_AMD_NO_JUMP_PAIRS"] = "1"  # KIND 2 as the unpaired int32 kernel (read once, at the first call)
    import intron_cases as ic
    rs = np.random.RandomState(11)
    base = []
    for i in range(32):
        q = int(rs.randint(150, 601))
        two = bool(i & 1)
        cut = sorted(int(x) for x in rs.randint(30, q - 30, size=3 if two else 2))
        e1 = [cut[0], cut[1] - cut[0]] + ([cut[2] - cut[1]] if two else [])
        i1 = [int(rs.randint(1000, 20001)) for _ in e1[1:]]
        w1, w2 = int(rs.randint(5000, 50001)), int(rs.randint(5000, 50001))
        pad = max(w1 - sum(e1) - sum(i1), 200)
        spec = dict(seed=5000 + i, ref1=dict(exons=e1, introns=i1, motif=["fw", "rev"][i % 2], lflank=pad // 2, rflank=pad - pad // 2),
                    ref2=dict(exons=[q - cut[-1]], introns=[], lflank=(w2 - q) // 2, rflank=w2 - (w2 - q) // 2), use="12", subst=3)
        base.append(ic.make_case(spec) + (i % 2 == 0, i % 2 == 0, True))
    probs = [base[i % len(base)] for i in range(n)]
    cells = sum(len(p[0]) * (len(p[1]) + len(p[2])) for p in probs)
    lib = Lib()
    print(lib.device_name())
    sc = [2, -8, -19, -1, -1, 0]  # SVRefinerOptions.hpp:46-49
    print("n=%d alignments, %.3g cells, query %d..%d, rows %d..%d" % (n, cells, min(len(p[0]) for p in base), max(len(p[0]) for p in base),
                                                                        min(len(p[1]) + len(p[2]) for p in base), max(len(p[1]) + len(p[2]) for p in base)))
    lib.align_intron_batch(sc, -100, -15, -1, probs[:32])
    lib.align_batch(2, sc, -100, [p[:3] for p in probs[:32]])
    for rep in range(4):
        t0 = time.time()
        r3 = lib.align_intron_batch(sc, -100, -15, -1, probs)
        t1 = time.time()
        r2 = lib.align_batch(2, sc, -100, [p[:3] for p in probs])
        t2 = time.time()
        print("rep %d  KIND 3 intron %.1f ms %.2f GCUPS | KIND 2 jump int32 %.1f ms %.2f GCUPS | ratio %.2f" % (
            rep, (t1 - t0) * 1e3, cells / (t1 - t0) / 1e9, (t2 - t1) * 1e3, cells / (t2 - t1) / 1e9, (t2 - t1) / (t1 - t0)))
    print("intron:", r3[0]["cigar1"], r3[0]["cigar2"], "| jump:", r2[0]["cigar1"], r2[0]["cigar2"])
    print("alignments with an N segment: %d of %d" % (sum("N" in r["cigar1"] + r["cigar2"] for r in r3), n))


if len(sys.argv) > 1 and sys.argv[1] == "--intron":
    intron_leg(max(256, int(sys.argv[2])) if len(sys.argv) > 2 else 256)
    sys.exit(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
kind = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(5)
probs = []
base = []
for i in range(64):
    ref = rand_seq(rng, 1500)
    alt = np.concatenate([ref[:750], ref[790:]])
    q = mutate(rng, alt[620:890], 0.003).tobytes()
    base.append((q, ref.tobytes(), rand_seq(rng, 700).tobytes()) if kind == 2 else (q, ref.tobytes()))
probs = [base[i % 64] for i in range(n)]
lib = Lib()
print(lib.device_name())
sc = [2, -8, -24, -1, -1, 0] if kind != 2 else [2, -8, -12, -1, -1, 0]
lib.align_batch(kind, sc, -100, probs[:256])
for rep in range(3):
    t0 = time.time()
    res = lib.align_batch(kind, sc, -100, probs)
    dt = time.time() - t0
    cells = sum(len(p[0]) * (len(p[1]) + (len(p[2]) if kind == 2 else 0)) for p in probs)
    print("n=%d  %.3f s  %.0f aln/s  %.1f GCUPS (host-timed incl. staging)" % (n, dt, n / dt, cells / dt / 1e9))
print(res[0])
