"""Inputs of the GlobalJumpIntronAligner cases whose reference outputs are stored in tests/golden/intron_aligner_cases.json.xz.

The golden file holds, per case, only a `spec` (seed, shape parameters), the scores and the reference's output text; the sequences are
regenerated here, so that references of 50 000 bases cost nothing in the repository.  The generator draws from numpy's legacy
``RandomState`` (its stream is frozen by numpy's compatibility policy).  Changing anything in this file invalidates the golden file:
tests/golden/make_intron_golden.py writes it again, and stores a digest of every case's sequences that the test checks first.

A spec describes each reference as  lflank | exon | intron | exon | ... | rflank  with the introns' first and last two bases set to a
motif, then trims the reference (so that an intron can touch or run over its edge), and builds the query from the exons."""
import hashlib

import numpy as np

MOTIFS = {"fw": (b"GT", b"AG"), "rev": (b"CT", b"AC"), "lower": (b"gt", b"ag"), "lowrev": (b"ct", b"ac"), "half": (b"GT", b"GG")}


def _rnd(rs, alphabet, n):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rs.randint(0, len(a), size=n)].tobytes() if n else b""


def _reference(rs, alphabet, r):
    """-> (reference bytes before trimming, list of exon byte strings)"""
    out = [_rnd(rs, alphabet, r.get("lflank", 0))]
    exons = []
    introns = r.get("introns", [])
    for i, n in enumerate(r["exons"]):
        e = _rnd(rs, alphabet, n)
        exons.append(e)
        out.append(e)
        if i < len(introns):
            body = bytearray(_rnd(rs, alphabet, introns[i]))
            motif = r.get("motif", "fw")
            motif = motif[i] if isinstance(motif, list) else motif
            if motif != "none" and len(body) >= 4:
                body[:2], body[-2:] = MOTIFS[motif]
            out.append(bytes(body))
    out.append(_rnd(rs, alphabet, r.get("rflank", 0)))
    return b"".join(out), exons


def make_case(spec):
    """-> (query, ref1, ref2) as bytes"""
    rs = np.random.RandomState(spec["seed"])
    alphabet = spec.get("alphabet", "ACGT").encode("latin-1")
    if spec.get("random"):  # plain random sequences over a small alphabet: motifs, ties and edge starts arise by chance
        q, r1, r2 = (_rnd(rs, alphabet, spec["random"][k]) for k in range(3))
        return q, r1, r2
    refs, exons = [], []
    for key in ("ref1", "ref2"):
        ref, ex = _reference(rs, alphabet, spec[key])
        lt, rt = spec[key].get("ltrim", 0), spec[key].get("rtrim", 0)
        refs.append(ref[lt:len(ref) - rt])
        exons.append(ex)
    use = spec.get("use", "12")
    parts = []
    if "1" in use:
        parts += exons[0]
    if use == "12":
        parts.append(_rnd(rs, alphabet, spec.get("jump_insert", 0)))
    if "2" in use:
        parts += exons[1]
    q = bytearray(b"".join(parts))
    noise = spec.get("noise", spec.get("alphabet", "ACGT")).encode("latin-1")
    for _ in range(spec.get("subst", 0)):
        q[rs.randint(0, len(q))] = noise[rs.randint(0, len(noise))]
    for _ in range(spec.get("indel", 0)):
        p = rs.randint(1, len(q) - 1)
        if rs.randint(0, 2):
            del q[p:p + rs.randint(1, 4)]
        else:
            q[p:p] = _rnd(rs, noise, rs.randint(1, 4))
    q = _rnd(rs, noise, spec.get("qclip_l", 0)) + bytes(q) + _rnd(rs, noise, spec.get("qclip_r", 0))
    q = q[spec.get("qtrim_l", 0):len(q) - spec.get("qtrim_r", 0)]
    if spec.get("lower_query"):
        q = q.lower()
    return q, refs[0], refs[1]


def digest(q, r1, r2):
    return hashlib.sha1(b"|".join((q, r1, r2))).hexdigest()[:16]


def result_text(r):
    """an ABI result (manta_amd._capi) in the layout of the stored reference text"""
    return "score %d align1 %d:%s align2 %d:%s jumpInsertSize %d jumpRange %d" % (
        r["score"], r["begin1"], r["cigar1"], r["begin2"], r["cigar2"], r["jump_insert_size"], r["jump_range"])
