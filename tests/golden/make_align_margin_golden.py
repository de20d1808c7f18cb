#!/usr/bin/env python3
"""Records the reference aligners' outputs on the cases of tests/align_margin_cases.py (run on the authoring machine only: it needs
oracle/_ref/libmanta_ref.so, the unmodified reference sources behind oracle/ref_driver.cpp, as `make -C oracle ref` builds it).

Writes tests/golden/align_margin_cases.json.xz:

  buckets[]  one per (kind, E): `seq` -- the cases that do not depend on the scores (spec, lengths, digest of the sequences), the bucket's
             shortest task last -- and `sets` -- per score set its name, the scores, the tie cases drawn for these scores, and `text`: the
             reference's output for every case of the set in the order of align_margin_cases.set_cases(), the shortest task last
  rows[]     the row-limit batches: per case spec, lengths, digest and output

No sequences are stored: the test regenerates them from the specs and checks the digests first."""
import json
import lzma
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import align_margin_cases as mc  # noqa: E402
from oracle_lib import RefLib  # noqa: E402


def entry(kind, spec, seqs):
    q, r1, r2 = seqs
    return dict(spec=spec, lens=[len(q), len(r1), len(r2 or b"")], digest=mc.digest(q, r1, r2))


def main():
    ref = RefLib()
    buckets, rows = [], []
    n = cells = 0
    fam = {}
    for kind in (mc.LARGE_INDEL, mc.JUMP):
        for E in mc.PACKED_E[kind]:
            shared = mc.sequence_cases(kind, E) + [mc.shortest_case(kind, E)]
            seqs = {json.dumps(c, sort_keys=True): mc.make_case(kind, c) for c in shared}
            b = dict(kind=kind, E=E, seq=[entry(kind, c, seqs[json.dumps(c, sort_keys=True)]) for c in shared], sets=[])
            for s in mc.score_sets(kind, E):
                cs = mc.set_cases(kind, E, s) + [mc.shortest_case(kind, E)]
                tie = [c for c in cs if c["f"].startswith("tie-")]
                for c in tie:
                    seqs[json.dumps(c, sort_keys=True)] = mc.make_case(kind, c)
                text = []
                for c in cs:
                    q, r1, r2 = seqs[json.dumps(c, sort_keys=True)]
                    assert mc.pick_e(len(q)) == E, c
                    text.append(ref.align(kind, s["sc"], s["extra"], q, r1, r2))
                    n += 1
                    cells += len(q) * (len(r1) + len(r2 or b""))
                    fam[c["f"]] = fam.get(c["f"], 0) + 1
                b["sets"].append(dict(name=s["name"], sc=s["sc"], extra=s["extra"], slack=s["slack"], eligible=s["eligible"],
                                      tie=[entry(kind, c, seqs[json.dumps(c, sort_keys=True)]) for c in tie], text=text))
            buckets.append(b)
        for name, packed, sc, extra, specs in mc.row_limit_batches(kind):
            cases = []
            for c in specs:
                seqs1 = mc.make_any(kind, c)
                e = entry(kind, c, seqs1)
                e["text"] = ref.align(kind, sc, extra, *seqs1)
                cases.append(e)
                n += 1
                fam["rows"] = fam.get("rows", 0) + 1
            rows.append(dict(kind=kind, name=name, packed=packed, sc=sc, extra=extra, cases=cases))
    out = os.path.join(HERE, "align_margin_cases.json.xz")
    with lzma.open(out, "wt", preset=9 | lzma.PRESET_EXTREME) as f:
        json.dump(dict(buckets=buckets, rows=rows), f, separators=(",", ":"), sort_keys=True)
    print("cases: %d %s, %.3g DP cells, %d bytes" % (n, json.dumps(fam, sort_keys=True), cells, os.path.getsize(out)))
    for b in buckets:
        print("kind %d E=%d:" % (b["kind"], b["E"]), "; ".join("%s %s/%d slack %d%s" % (s["name"], s["sc"], s["extra"], s["slack"], "" if s["eligible"] else " (ineligible)")
                                                             for s in b["sets"]))


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("%.1f s" % (time.time() - t0))
