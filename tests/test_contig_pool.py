"""contig_pool_kernel (asm_contig.hpp): the small LDS class' loci share their workgroup's LDS as a pool and are taken largest graph
first.  One call with more config-2 loci than a pool holds at once (24 graphs of 12-19 KB against 160 KB for 12 waves), so that waves
take shares, wait for room, give shares back and take a second one in a hole a released share left; every locus must equal the
oracle, and the single-wave contig_kernel (MANTA_AMD_NO_CONTIG_POOL) must give the same results.  MANTA_AMD_DEBUG's pool line shows
that the waits and the second takes happened."""
import re

import pytest

from manta_amd._capi import assembly_text
from oracle_lib import asm_opts
from synth import small_indel_locus

N_LOCI = 24


def _pool_batch():
    piles = [small_indel_locus(900 + i, sub_rate=0.003 * (i % 4))[0] for i in range(N_LOCI)]
    return asm_opts(minWordLength=31), piles


def _pool_line(err):
    m = re.search(r"contig_pool_kernel: (\d+) shares taken, ([\d.]+) loci resident per CU on average at a take, (\d+) takes waited", err)
    assert m, err[-2000:]
    return int(m.group(1)), float(m.group(2)), int(m.group(3))


def _check_pool(lib, oracle, monkeypatch, capfd, waves):
    monkeypatch.setenv("MANTA_AMD_ASM_PATH", "fast")
    monkeypatch.setenv("MANTA_AMD_DEBUG", "1")
    o, piles = _pool_batch()
    capfd.readouterr()
    pooled = [assembly_text(r) for r in lib.assemble_batch(o, piles)]
    taken, resident, waited = _pool_line(capfd.readouterr().err)
    for reads, got in zip(piles, pooled):
        assert got == oracle.assemble(o, reads)
    assert taken > waves  # some wave took a second share
    assert resident > 1.0
    return pooled, waited


def test_emulated_contig_pool_matches_oracle(emu, oracle, monkeypatch, capfd):
    # the emulator runs the first workgroup's 12 waves alone: they take every locus, and 12 config-2 graphs do not fit 160 KB
    _, waited = _check_pool(emu, oracle, monkeypatch, capfd, waves=12)
    assert waited > 0


@pytest.mark.gpu
def test_gpu_contig_pool_matches_oracle(gpu, oracle, monkeypatch, capfd):
    pooled, _ = _check_pool(gpu, oracle, monkeypatch, capfd, waves=0)
    monkeypatch.setenv("MANTA_AMD_NO_CONTIG_POOL", "1")
    o, piles = _pool_batch()
    assert [assembly_text(r) for r in gpu.assemble_batch(o, piles)] == pooled
