// Test-only: the C surface of host_refiner_full_capi.cpp (the product's SVCandidateAssemblyRefiner behind the reference driver's POD
// interface) plus what tests/test_spanning_select.py needs of the device contig selection: the host restatement of a contig's
// verdicts, the selection of constructed loci by the free host functions or by the adapter selectJumpContigBatch, and the batched
// refiner call with the switch given.
#include "host_refiner_full_capi.cpp"

#include "contig_qc.hpp"

namespace {
AlignmentScores<int> spanScores(const int32_t* s) { return AlignmentScores<int>(s[0], s[1], s[2], s[3], s[4], s[5] != 0); }

JumpAlignmentResult<int> jumpOf(const char* c1, const char* c2, const int score)
{
  JumpAlignmentResult<int> ja;
  ja.score        = score;
  ja.align1.apath = ALIGNPATH::cigar_to_apath(c1);
  ja.align2.apath = ALIGNPATH::cigar_to_apath(c2);
  return ja;
}
}  // namespace

/// isJumpAlignmentQCFail and isLowQualityJumpAlignment (refiner_util.hpp) of one contig alignment, verdict by verdict ->
/// out[0..7]: qc_fail, ref_length1, ref_length2, read_length1, read_length2, span_low (bit s: align1 at span s, bit 3 + s: align2),
/// low1, low2.  Returns isLowQualityJumpAlignment's own value.
MINE_EXPORT int mine_jump_contig_verdict(const int32_t* scores, const char* c1, const char* c2, int isRNA, int* out)
{
  const AlignmentScores<int>     sc(spanScores(scores));
  const JumpAlignmentResult<int> ja(jumpOf(c1, c2, 0));
  out[0] = isJumpAlignmentQCFail(ja);
  out[1] = int(ALIGNPATH::apath_ref_length(ja.align1.apath));
  out[2] = int(ALIGNPATH::apath_ref_length(ja.align2.apath));
  out[3] = int(ALIGNPATH::apath_read_length(ja.align1.apath));
  out[4] = int(ALIGNPATH::apath_read_length(ja.align2.apath));
  const unsigned dna[] = {75, 100, 200}, rna[] = {36, 75, 100};
  unsigned       bits = 0;
  for (int s = 0; s < 3; ++s) {
    const unsigned span = isRNA ? rna[s] : dna[s];
    const unsigned s1   = span + (isRNA ? ALIGNPATH::apath_spliced_length(ja.align1.apath) : 0u);
    const unsigned s2   = span + (isRNA ? ALIGNPATH::apath_spliced_length(ja.align2.apath) : 0u);
    if (isLowQualitySpanningSVAlignment(s1, sc, true, isRNA != 0, ja.align1.apath)) bits |= 1u << s;
    if (isLowQualitySpanningSVAlignment(s2, sc, false, isRNA != 0, ja.align2.apath)) bits |= 8u << s;
  }
  out[5] = int(bits);
  out[6] = (bits & 7u) == 7u;
  out[7] = (bits >> 3) == 7u;
  return isLowQualityJumpAlignment(ja, sc, isRNA != 0);
}

/// The selection of n loci given as text, contigs flattened over the loci (nContigs[l] of them each); support[i]: the size of contig
/// i's supportReads (reads 0 .. support[i] - 1).  use_device == 0: selectJumpContigDNA / selectJumpContigRNA; 1: the adapter
/// selectJumpContigBatch.  Per locus one line "<device status> <best contig or -1>".
MINE_EXPORT int mine_select_jump_contig_loci(
    const int32_t* scores, int isRNA, int n, const int* nContigs, const char* const* cigars1, const char* const* cigars2, const int* contigScores,
    const int* support, int use_device, char* out, int cap)
{
  try {
    const AlignmentScores<int>                         sc(spanScores(scores));
    std::vector<std::vector<JumpAlignmentResult<int>>> aligns(n);
    std::vector<Assembly>                              contigs(n);
    std::vector<JumpContigLocusInput>                  items(n);
    int                                                at = 0;
    for (int l = 0; l < n; ++l) {
      contigs[l].resize(nContigs[l]);
      for (int c = 0; c < nContigs[l]; ++c, ++at) {
        aligns[l].push_back(jumpOf(cigars1[at], cigars2[at], contigScores[at]));
        for (int r = 0; r < support[at]; ++r) contigs[l][c].supportReads.insert(unsigned(r));
      }
      items[l] = JumpContigLocusInput{&aligns[l], &contigs[l]};
    }
    std::vector<JumpContigSelection> res(n);
    if (use_device) {
      selectJumpContigBatch(sc, isRNA != 0, items, res);
    } else {
      for (int l = 0; l < n; ++l) res[l].best = selectJumpContigHost(sc, isRNA != 0, items[l]);
    }
    std::ostringstream os;
    for (int l = 0; l < n; ++l) os << res[l].deviceStatus << " " << res[l].best << "\n";
    return emit(os.str(), out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}

/// mine_get_candidate_assembly_data_multi's one batched call (is_batched == 1) on a refiner with setDeviceSpanningSelect(device_select);
/// counters: spanning loci, loci whose selection the device decided, loci it left to the host function
MINE_EXPORT int mine_get_candidate_assembly_data_batch_select(const ref_refine_input_t* inputs, int n, int device_select, uint64_t* counters, char* out,
                                                              int cap)
{
  try {
    MemorySource    source;
    bam_header_info header;
    for (int i = 0; i < inputs[0].n_chrom; ++i) {
      source.chroms.emplace_back(inputs[0].chrom_seq[i]);
      header.chrom_data.emplace_back(std::to_string(i).c_str(), unsigned(source.chroms.back().size()));
    }
    GSCOptions options;
    setOptions(inputs[0], options);
    std::vector<SVCandidate> svs;
    for (int k = 0; k < n; ++k) {
      const ref_refine_input_t& in(inputs[k]);
      MemorySource::Pile        pile;
      pile.tid = in.bp_tid[0];
      pile.pos = in.bp_begin[0];
      for (int i = 0; i < in.n_reads; ++i) pile.reads.emplace_back(in.reads[i]);
      source.piles.push_back(pile);
      for (int c = 0; c < std::max(1, in.n_calls); ++c) svs.push_back(makeSV(in));
    }
    SVCandidateAssemblyRefiner refiner(options, header, source);
    refiner.setDeviceSpanningSelect(device_select != 0);
    std::vector<SVCandidateAssemblyData> data;
    refiner.getCandidateAssemblyDataBatch(svs, inputs[0].is_find_large_insertions != 0, data);
    std::string text;
    for (const auto& d : data) text += dumpAssemblyData(d);
    counters[0] = refiner.stats().spanningLoci;
    counters[1] = refiner.stats().deviceSpanningSelectLoci;
    counters[2] = refiner.stats().deviceSpanningSelectFallbacks;
    return emit(text, out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}
