// C-ABI implementation, part 3 (see api.cpp, api_internal.hpp): split-read scoring and read gathering.
#include "api_internal.hpp"


// ------------------------------------------------------------------------------------------------------
// split-read scoring
// ------------------------------------------------------------------------------------------------------
extern "C" int manta_split_read_batch(
    manta_ctx_t* ctx, const double* ln_comp_error_prob, const double* ln_error_prob, uint32_t n_qscores, float ln_one_third,
    float ln_random_base, uint32_t n_tasks, const manta_split_task_t* tasks, const uint8_t* arena, uint64_t arena_bytes,
    manta_split_result_t* results)
{
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (!ln_comp_error_prob || !ln_error_prob || n_qscores == 0 || (n_tasks && (!tasks || !arena || !results)))
    return fail(ctx, MANTA_E_INVALID_ARG, "manta_split_read_batch: null argument");
  if (n_tasks == 0) return MANTA_OK;
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    std::vector<SplitTaskDev> dev(n_tasks);
    uint8_t*                  dArena = ctx->dSeq.as<uint8_t>(arena_bytes + 16);
    auto outside = [&](uint64_t off, uint64_t len) { return off > arena_bytes || len > arena_bytes - off; };
    for (uint32_t i = 0; i < n_tasks; ++i) {
      const manta_split_task_t& t(tasks[i]);
      if (outside(t.query_off, t.query_len) || outside(t.qual_off, t.query_len) || outside(t.target_off, t.target_len))
        return fail(ctx, MANTA_E_INVALID_ARG, "manta_split_read_batch: task " + std::to_string(i) + " outside the arena");
      SplitTaskDev& d(dev[i]);
      d.query            = dArena + t.query_off;
      d.qual             = dArena + t.qual_off;
      d.target           = dArena + t.target_off;
      d.query_len        = t.query_len;
      d.target_len       = t.target_len;
      d.bp_begin         = t.bp_begin;
      d.bp_end           = t.bp_end;
      d.flank_score_size = t.flank_score_size;
      d.reserved         = 0;
    }
    SplitTaskDev*   dTasks = ctx->dSplitTasks.as<SplitTaskDev>(n_tasks);
    SplitResultDev* dRes   = ctx->dSplitResults.as<SplitResultDev>(n_tasks);
    double*         dTab   = ctx->dSplitTables.as<double>(2ull * n_qscores + 2);
    uint32_t*       dCount = ctx->dCounter.as<uint32_t>(kNumESet);
    rt::h2d(dArena, arena, arena_bytes);
    rt::h2d(dTasks, dev.data(), sizeof(SplitTaskDev) * n_tasks);
    rt::h2d(dTab, ln_comp_error_prob, sizeof(double) * n_qscores);
    rt::h2d(dTab + n_qscores, ln_error_prob, sizeof(double) * n_qscores);
    rt::dzero(dCount, sizeof(uint32_t));
    SplitParams P;
    P.tasks          = dTasks;
    P.results        = dRes;
    P.n_tasks        = n_tasks;
    P.n_q            = n_qscores;
    P.ln_comp_error  = dTab;
    P.ln_error       = dTab + n_qscores;
    P.ln_one_third   = ln_one_third;
    P.ln_random_base = ln_random_base;
    P.counter        = dCount;
    const int grid = rt::roundGrid(int(std::min<uint64_t>(n_tasks, uint64_t(std::max(1, ctx->cuCount * 32)))));
    rt::launch(split_read_kernel, grid, 0, P);
    std::vector<SplitResultDev> h(n_tasks);
    rt::d2h(h.data(), dRes, sizeof(SplitResultDev) * n_tasks);
    int worst = MANTA_OK;
    for (uint32_t i = 0; i < n_tasks; ++i) {
      manta_split_result_t& r(results[i]);
      std::memset(&r, 0, sizeof(r));
      const SplitResultDev& d(h[i]);
      r.status = (d.status == 0) ? MANTA_OK : (d.status == 3) ? MANTA_E_UNSUPPORTED : MANTA_E_INVALID_ARG;
      if (d.status == 1) r.status = MANTA_E_SPLIT_QUERY_NOT_SHORTER;
      if (d.status == 2) r.status = MANTA_E_SPLIT_EMPTY_SCAN;
      if (r.status != MANTA_OK) {
        worst = r.status;
        continue;
      }
      r.best_pos         = d.best_pos;
      r.best_ln_lhood    = d.best_ln_lhood;
      r.left_size        = d.left_size;
      r.hom_size         = d.hom_size;
      r.right_size       = d.right_size;
      r.left_mismatches  = d.left_mismatches;
      r.hom_mismatches   = d.hom_mismatches;
      r.right_mismatches = d.right_mismatches;
    }
    if (worst != MANTA_OK) return fail(ctx, worst, "manta_split_read_batch: one or more tasks failed; see per-task status");
    return MANTA_OK;
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" void manta_read_search_range(int32_t bp_begin, int32_t bp_end, int32_t* search_begin, int32_t* search_end)
{
  manta_read_scan_t sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.bp_begin = bp_begin;
  sc.bp_end   = bp_end;
  int sb, se;
  ReadClass::searchRange(sc, sb, se);
  if (search_begin) *search_begin = sb;
  if (search_end) *search_end = se;
}

extern "C" int manta_read_piles_batch(
    manta_ctx_t* ctx, const manta_read_class_options_t* opt, uint32_t n_loci, const manta_read_locus_t* loci, uint32_t n_scans,
    const manta_read_scan_t* scans, uint32_t n_reads, const manta_bam_read_t* reads, const uint32_t* cigars, uint64_t n_cigar_words,
    const uint8_t* names, uint64_t names_bytes, const uint8_t* seqs, uint64_t seqs_bytes, const uint8_t* quals, uint64_t quals_bytes,
    const uint8_t* refs, uint64_t refs_bytes, uint8_t* decision, uint32_t* pile_index, manta_read_locus_result_t* results,
    uint32_t* codes, uint64_t codes_cap, uint64_t* codes_used, uint32_t* nmask, uint64_t mask_cap, uint64_t* mask_used,
    uint32_t* read_len, uint64_t* read_code_off, uint64_t* read_mask_off, uint32_t* pile_read, uint64_t reads_cap,
    uint64_t* reads_used, uint32_t* locus_read_begin)
{
  static const char* fn = "manta_read_piles_batch: ";
  if (!ctx) return MANTA_E_INVALID_ARG;
  // (the two offset arrays take their "one past the last read" entry whenever there is a candidate, also with no read at all)
  if (!opt || (n_loci && (!loci || !results || !locus_read_begin || !read_code_off || !read_mask_off)) || (n_scans && !scans) ||
      (n_reads && (!reads || !decision || !pile_index)) || (n_cigar_words && !cigars) || (names_bytes && !names) || (seqs_bytes && !seqs) ||
      (quals_bytes && !quals))
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + "null argument");
  if (codes_used) *codes_used = 0;
  if (mask_used) *mask_used = 0;
  if (reads_used) *reads_used = 0;
  if (n_loci == 0) return MANTA_OK;
  // what the kernels index with must lie inside what was handed over
  uint64_t maxRange = 1, maxRecords = 1, codeBound = 0, maskBound = 0;
  std::vector<uint32_t> chunks;  // read_test_kernel's work list: 64 records of one query each (scan, first record, candidate)
  chunks.reserve(3 * (size_t(n_reads) / 64 + n_scans + 1));
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (loci[l].scan_begin > loci[l].scan_end || loci[l].scan_end > n_scans)
      return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + "candidate " + std::to_string(l) + ": scans outside the scan array");
    uint64_t recs = 0;
    for (uint32_t s = loci[l].scan_begin; s < loci[l].scan_end; ++s) {
      const manta_read_scan_t& sc(scans[s]);
      if (sc.read_begin > sc.read_end || sc.read_end > n_reads || sc.ref_off > refs_bytes || sc.ref_len > refs_bytes - sc.ref_off ||
          (sc.ref_len && !refs) || sc.bam_index >= (1u << 22))
        return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + "scan " + std::to_string(s) + " outside the arrays");
      int sb, se;
      ReadClass::searchRange(sc, sb, se);
      maxRange = std::max<uint64_t>(maxRange, uint64_t(se > sb ? se - sb : 0) + 2);
      recs += sc.read_end - sc.read_begin;
      for (uint32_t base = sc.read_begin; base < sc.read_end; base += 64) {
        chunks.push_back(s);
        chunks.push_back(base);
        chunks.push_back(l);
      }
    }
    maxRecords = std::max(maxRecords, recs);
  }
  if (maxRange > (1ull << 26)) return fail(ctx, MANTA_E_UNSUPPORTED, std::string(fn) + "a breakend interval beyond 64 M bases");
  for (uint32_t i = 0; i < n_reads; ++i) {
    const manta_bam_read_t& r(reads[i]);
    const bool bad = r.cigar_off > n_cigar_words || r.n_cigar > n_cigar_words - r.cigar_off ||
                     ((r.tags & MANTA_READ_TAG_MC) && (r.mate_cigar_off > n_cigar_words || r.n_mate_cigar > n_cigar_words - r.mate_cigar_off)) ||
                     r.qname_off > names_bytes || r.qname_len > names_bytes - r.qname_off || r.seq_off > seqs_bytes ||
                     (uint64_t(r.read_len) + 1) / 2 > seqs_bytes - r.seq_off || r.qual_off > quals_bytes || r.read_len > quals_bytes - r.qual_off;
    if (bad) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + "record " + std::to_string(i) + " outside the arenas");
    codeBound += (uint64_t(r.read_len) + 15) / 16;
    maskBound += (uint64_t(r.read_len) + 31) / 32;
  }
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    uint64_t tableCap = 64;
    while (tableCap < 2 * maxRecords) tableCap *= 2;
    const uint64_t stride = 2 * maxRange + 1 + tableCap;
    // one workspace per wave, sized for the widest breakend interval of the batch: a multi-megabase interval shrinks the grid instead
    // of asking for (waves x that interval) bytes (the reference allocates searchRange.size() counters for the one candidate)
    const uint64_t wsFit  = std::max<uint64_t>(1, workspaceBudget(size_t(16) << 30) / (stride * 4));
    const int      grid   = rt::roundGrid(int(std::min<uint64_t>(std::min<uint64_t>(n_loci, wsFit), uint64_t(std::max(1, ctx->cuCount * 8)))));
    ReadClassParams P;
    std::memset(&P, 0, sizeof(P));
    P.opt    = *opt;
    P.n_loci = n_loci;
    auto up  = [&](DevBuf& b, const void* src, uint64_t bytes) {
      uint8_t* d = b.as<uint8_t>(bytes + 16);
      rt::h2d(d, src, bytes);
      return d;
    };
    P.loci   = reinterpret_cast<const manta_read_locus_t*>(up(ctx->dRc[0], loci, sizeof(manta_read_locus_t) * uint64_t(n_loci)));
    P.scans  = reinterpret_cast<const manta_read_scan_t*>(up(ctx->dRc[1], scans, sizeof(manta_read_scan_t) * uint64_t(n_scans)));
    P.reads  = reinterpret_cast<const manta_bam_read_t*>(up(ctx->dRc[2], reads, sizeof(manta_bam_read_t) * uint64_t(n_reads)));
    P.cigars = reinterpret_cast<const uint32_t*>(up(ctx->dRc[3], cigars, 4 * n_cigar_words));
    P.names  = up(ctx->dRc[4], names, names_bytes);
    P.seqs   = up(ctx->dRc[5], seqs, seqs_bytes);
    P.quals  = up(ctx->dRc[6], quals, quals_bytes);
    P.refs   = up(ctx->dRc[7], refs, refs_bytes);
    // outputs and workspace in one allocation each
    uint8_t* dOut = ctx->dRc[8].as<uint8_t>(uint64_t(n_reads) * 13 + uint64_t(n_loci) * (sizeof(manta_read_locus_result_t) + 16 + 32) + 256 +
                                            4 * (uint64_t(n_loci) + 1));
    P.pile_index   = reinterpret_cast<uint32_t*>(dOut);
    P.tmp          = P.pile_index + n_reads;
    P.results      = reinterpret_cast<manta_read_locus_result_t*>(P.tmp + n_reads);
    P.locus_counts = reinterpret_cast<uint32_t*>(P.results + n_loci);
    P.locus_base   = reinterpret_cast<unsigned long long*>(P.locus_counts + 4 * uint64_t(n_loci));
    P.locus_read_begin = reinterpret_cast<uint32_t*>(P.locus_base + 4 * (uint64_t(n_loci) + 1));
    P.counter      = P.locus_read_begin + n_loci + 1;  // four queue heads
    P.decision     = reinterpret_cast<uint8_t*>(P.counter + 4);
    P.pre          = P.decision + n_reads;
    P.chunks       = reinterpret_cast<const uint32_t*>(up(ctx->dRc[14], chunks.data(), 4 * chunks.size()));
    P.n_chunks     = uint32_t(chunks.size() / 3);
    P.ws           = ctx->dRc[9].as<uint32_t>(stride * uint64_t(grid));
    P.ws_stride    = stride;
    P.range_cap    = uint32_t(maxRange);
    P.table_cap    = uint32_t(tableCap);
    P.codes        = ctx->dRc[10].as<uint32_t>(codeBound + 4);
    P.nmask        = ctx->dRc[11].as<uint32_t>(maskBound + 4);
    P.read_len     = ctx->dRc[12].as<uint32_t>(2 * uint64_t(n_reads) + 4);
    P.pile_read    = P.read_len + n_reads + 1;
    P.read_code_off = ctx->dRc[13].as<unsigned long long>(2 * (uint64_t(n_reads) + 2));
    P.read_mask_off = P.read_code_off + n_reads + 1;
    rt::dzero(P.counter, 4 * sizeof(uint32_t));
    const int wide    = rt::roundGrid(std::max(1, ctx->cuCount * 16));
    auto      gridFor = [&](uint64_t items) { return std::min(wide, rt::roundGrid(int(std::max<uint64_t>(1, std::min<uint64_t>(items, 1u << 20))))); };
    rt::launch(read_test_kernel, gridFor(P.n_chunks), 0, P);
    rt::launch(read_class_kernel, grid, 0, P);
    rt::launch(read_pile_offsets_kernel, rt::roundGrid(1), 0, P);
    rt::launch(read_pile_pack_kernel, grid, 0, P);
    rt::launch(read_pile_bases_kernel, gridFor(uint64_t(n_reads) / 8 + 1), 0, P);
    unsigned long long totals[4] = {0, 0, 0, 0};
    rt::d2h(totals, P.locus_base + 4 * uint64_t(n_loci), sizeof(totals));  // (synchronizes)
    if (reads_used) *reads_used = totals[0];
    if (codes_used) *codes_used = totals[1];
    if (mask_used) *mask_used = totals[2];
    rt::d2hAsync(decision, P.decision, n_reads);
    rt::d2hAsync(pile_index, P.pile_index, 4 * uint64_t(n_reads));
    rt::d2hAsync(results, P.results, sizeof(manta_read_locus_result_t) * uint64_t(n_loci));
    rt::d2hAsync(locus_read_begin, P.locus_read_begin, 4 * (uint64_t(n_loci) + 1));
    const bool fits = totals[0] <= reads_cap && totals[1] <= codes_cap && totals[2] <= mask_cap &&
                      (totals[0] == 0 || (codes && nmask && read_len && pile_read));
    if (fits) {
      rt::d2hAsync(codes, P.codes, 4 * totals[1]);
      rt::d2hAsync(nmask, P.nmask, 4 * totals[2]);
      rt::d2hAsync(read_len, P.read_len, 4 * totals[0]);
      rt::d2hAsync(pile_read, P.pile_read, 4 * totals[0]);
      rt::d2hAsync(read_code_off, P.read_code_off, 8 * (totals[0] + 1));
      rt::d2hAsync(read_mask_off, P.read_mask_off, 8 * (totals[0] + 1));
    }
    rt::sync();
    if (!fits) return fail(ctx, MANTA_E_CAPACITY, std::string(fn) + "pile arrays too small (see *_used)");
    int worst = MANTA_OK;
    for (uint32_t l = 0; l < n_loci; ++l)
      if (results[l].status != MANTA_OK) worst = results[l].status;
    if (worst != MANTA_OK) return fail(ctx, worst, std::string(fn) + "one or more candidates failed; see per-candidate status");
    return MANTA_OK;
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

// ------------------------------------------------------------------------------------------------------
// small-SV contig QC (smallsv_qc_kernels.hpp)
// ------------------------------------------------------------------------------------------------------
extern "C" int manta_smallsv_qc_batch(
    manta_ctx_t* ctx, const manta_align_scores_t* filter_scores, uint32_t min_candidate_indel_size, uint32_t n_loci,
    const manta_asm_locus_result_t* loci, const manta_asm_contig_t* contigs, const manta_smallsv_alignment_t* alignments,
    const uint8_t* seq_arena, const uint32_t* cigar_arena, const uint8_t* refs, const uint64_t* ref_off, manta_smallsv_qc_t* qc_out,
    uint32_t* seg_arena, uint64_t seg_cap, uint64_t* seg_used)
{
  static const char* fn = "manta_smallsv_qc_batch";
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (seg_used) *seg_used = 0;
  if (!filter_scores || (n_loci && (!loci || !ref_off))) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  // the records the loci refer to, and how much of every arena they reach
  uint64_t nContigs = 0, seqBytes = 0, cigarWords = 0;
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (ref_off[l + 1] < ref_off[l]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": ref_off not monotone");
    if (loci[l].status != MANTA_OK || loci[l].n_contigs == 0) continue;
    nContigs = std::max<uint64_t>(nContigs, uint64_t(loci[l].first_contig) + loci[l].n_contigs);
  }
  if (nContigs == 0) return MANTA_OK;
  if (!contigs || !alignments || !seq_arena || !cigar_arena || !refs || !qc_out)
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  std::vector<QcTaskDev> host(nContigs);
  std::vector<uint8_t>   seen(nContigs, 0);
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (loci[l].status != MANTA_OK) continue;
    for (uint32_t c = 0; c < loci[l].n_contigs; ++c) {
      const uint64_t i = uint64_t(loci[l].first_contig) + c;
      if (seen[i]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": contig record " + std::to_string(i) + " belongs to two loci");
      seen[i] = 1;
      const manta_align_result_t& a(alignments[i].align);
      seqBytes = std::max<uint64_t>(seqBytes, contigs[i].seq_off + contigs[i].seq_len);
      if (a.status == MANTA_OK) cigarWords = std::max<uint64_t>(cigarWords, a.cigar1_off + a.cigar1_len);
    }
  }
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    const uint64_t refBytes = ref_off[n_loci];
    uint8_t*       dSeq  = ctx->dQc[5].as<uint8_t>(seqBytes + 16);
    uint32_t*      dCig  = ctx->dCigar.as<uint32_t>(cigarWords + 4);
    uint8_t*       dRefs = ctx->dQc[4].as<uint8_t>(refBytes + 16);
    for (uint32_t l = 0; l < n_loci; ++l) {
      if (loci[l].status != MANTA_OK) continue;
      for (uint32_t c = 0; c < loci[l].n_contigs; ++c) {
        const uint64_t              i = uint64_t(loci[l].first_contig) + c;
        const manta_align_result_t& a(alignments[i].align);
        QcTaskDev&                  t(host[i]);
        t.contig     = dSeq + contigs[i].seq_off;
        t.contig_len = contigs[i].seq_len;
        t.cigar      = dCig + ((a.status == MANTA_OK) ? a.cigar1_off : 0);
        t.n_cigar    = (a.status == MANTA_OK) ? a.cigar1_len : 0u;
        t.ref        = dRefs + ref_off[l];
        t.ref_len    = uint32_t(std::min<uint64_t>(ref_off[l + 1] - ref_off[l], 0xffffffffull));
        t.begin_pos  = a.begin_pos1;
        t.status     = a.status;
        t.reserved   = 0;
      }
    }
    const uint64_t segCap = std::min<uint64_t>(nContigs * QC_SEG_PAIRS, 0xffffffffull);
    QcParams       Q;
    std::memset(&Q, 0, sizeof(Q));
    QcTaskDev* dTasks = ctx->dQc[0].as<QcTaskDev>(nContigs);
    Q.tasks    = dTasks;
    Q.n_units  = uint32_t(nContigs);
    qcSetScores(Q, *filter_scores, min_candidate_indel_size);
    Q.out      = ctx->dQc[1].as<QcRecordDev>(nContigs);
    Q.segs     = ctx->dQc[2].as<uint32_t>(2 * segCap);
    Q.seg_cap  = uint32_t(segCap);
    Q.seg_used = ctx->dQc[3].as<uint32_t>(4);
    Q.counter  = Q.seg_used + 1;
    rt::h2d(dSeq, seq_arena, seqBytes);
    rt::h2d(dCig, cigar_arena, 4 * cigarWords);
    rt::h2d(dRefs, refs, refBytes);
    rt::h2d(dTasks, host.data(), sizeof(QcTaskDev) * nContigs);
    rt::dzero(Q.seg_used, 16);
    rt::launch(smallsv_qc_kernel, qcGrid(ctx, nContigs), QC_LDS_BYTES, Q);
    uint32_t cnt[4];
    rt::d2h(cnt, Q.seg_used, sizeof(cnt));
    std::vector<QcRecordDev> hRec(nContigs);
    const uint64_t           devUsed = std::min<uint64_t>(cnt[0], segCap);
    std::vector<uint32_t>    hSegs(2 * devUsed + 2);
    rt::d2hAsync(hRec.data(), Q.out, sizeof(QcRecordDev) * nContigs);
    rt::d2hAsync(hSegs.data(), Q.segs, 8 * devUsed);
    rt::sync();
    return qcCompact(ctx, nContigs, [&](uint64_t i) { return seen[i] ? &hRec[i] : nullptr; }, hSegs.data(), devUsed, qc_out, seg_arena,
                     seg_cap, seg_used, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" int manta_smallsv_set_qc(manta_smallsv_t* b, const manta_align_scores_t* filter_scores, uint32_t min_candidate_indel_size)
{
  if (!b) return MANTA_E_INVALID_ARG;
  b->qcOn  = filter_scores != nullptr;
  b->qcRan = false;
  if (filter_scores) b->qcScores = *filter_scores;
  b->qcMinIndel = min_candidate_indel_size;
  return MANTA_OK;
}

extern "C" int manta_smallsv_download_qc(manta_smallsv_t* b, manta_smallsv_qc_t* qc, uint64_t cap, uint32_t* seg_arena, uint64_t seg_cap,
                                         uint64_t* seg_used)
{
  static const char* fn = "manta_smallsv_download_qc";
  if (!b) return MANTA_E_INVALID_ARG;
  manta_ctx_t* ctx = b->ctx;
  if (seg_used) *seg_used = 0;
  if (!b->ran || !b->qcRan) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": no run with QC set (manta_smallsv_set_qc, then manta_smallsv_run)");
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(b->main);
    const uint32_t nLoci  = b->nLoci, maxAsm = b->opt.max_assembly_count;
    const uint64_t nSlots = uint64_t(nLoci) * maxAsm;
    std::vector<AsmLocusOut> hLoci(nLoci);
    std::vector<QcRecordDev> hRec(nSlots);
    uint32_t                 cnt[4];
    rt::d2hAsync(hLoci.data(), b->asmStage.dLoci, sizeof(AsmLocusOut) * nLoci);
    rt::d2hAsync(hRec.data(), b->dQc.p, sizeof(QcRecordDev) * nSlots);
    rt::d2h(cnt, b->dQcCnt.p, sizeof(cnt));
    const uint64_t        devUsed = std::min<uint64_t>(cnt[0], b->dQcSegs.cap / 8);
    std::vector<uint32_t> hSegs(2 * devUsed + 2);
    rt::d2h(hSegs.data(), b->dQcSegs.p, 8 * devUsed);
    // contigs[] of manta_smallsv_download: the loci in order, every locus' contigs in order (AsmStage::compact)
    std::vector<uint64_t> slotOf;
    for (uint32_t l = 0; l < nLoci; ++l)
      if (hLoci[l].status == ASM_OK)
        for (uint32_t c = 0; c < hLoci[l].n_contigs; ++c) slotOf.push_back(uint64_t(l) * maxAsm + c);
    if (slotOf.size() > cap || (!slotOf.empty() && !qc)) return fail(ctx, MANTA_E_CAPACITY, std::string(fn) + ": record array too small");
    return qcCompact(ctx, slotOf.size(), [&](uint64_t i) { return &hRec[slotOf[i]]; }, hSegs.data(), devUsed, qc, seg_arena, seg_cap, seg_used, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

// ------------------------------------------------------------------------------------------------------
// small-SV large-insertion search (smallsv_li_kernels.hpp)
// ------------------------------------------------------------------------------------------------------
extern "C" int manta_smallsv_large_insertion_batch(
    manta_ctx_t* ctx, const manta_align_scores_t* edge_scores, const manta_align_scores_t* complete_scores, uint32_t n_loci,
    const manta_asm_locus_result_t* loci, const manta_asm_contig_t* contigs, const manta_smallsv_alignment_t* alignments,
    const uint8_t* seq_arena, const uint32_t* cigar_arena, const uint8_t* refs, const uint64_t* ref_off, const manta_ref_cuts_t* cuts,
    manta_large_insert_edge_t* edge_out, manta_large_insertion_t* li_out, uint32_t* cigar_out, uint64_t cigar_cap, uint64_t* cigar_used)
{
  static const char* fn = "manta_smallsv_large_insertion_batch";
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (cigar_used) *cigar_used = 0;
  if (!edge_scores || !complete_scores || (n_loci && (!loci || !ref_off || !cuts || !li_out)))
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  if (n_loci == 0) return MANTA_OK;
  // the records the loci refer to, and how much of every arena they reach
  uint64_t nContigs = 0, seqBytes = 0, cigarWords = 0, maxContigLen = 0;
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (ref_off[l + 1] < ref_off[l]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": ref_off not monotone");
    if (loci[l].status != MANTA_OK || loci[l].n_contigs == 0) continue;
    nContigs = std::max<uint64_t>(nContigs, uint64_t(loci[l].first_contig) + loci[l].n_contigs);
  }
  if (nContigs && (!contigs || !alignments || !seq_arena || !cigar_arena || !refs || !edge_out))
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  std::vector<LiTaskDev>  hTasks(nContigs + 1);
  std::vector<LiLocusDev> hLoci(n_loci);
  std::vector<uint8_t>    seen(nContigs + 1, 0);
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (loci[l].status != MANTA_OK) continue;
    for (uint32_t c = 0; c < loci[l].n_contigs; ++c) {
      const uint64_t i = uint64_t(loci[l].first_contig) + c;
      if (seen[i]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": contig record " + std::to_string(i) + " belongs to two loci");
      seen[i] = 1;
      const manta_align_result_t& a(alignments[i].align);
      seqBytes     = std::max<uint64_t>(seqBytes, contigs[i].seq_off + contigs[i].seq_len);
      maxContigLen = std::max<uint64_t>(maxContigLen, contigs[i].seq_len);
      if (a.status == MANTA_OK) cigarWords = std::max<uint64_t>(cigarWords, a.cigar1_off + a.cigar1_len);
    }
  }
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    DevBuf* const  B        = ctx->dLi;
    const uint64_t refBytes = ref_off[n_loci];
    uint8_t*       dSeq  = B[LI_BUF_COUNT + 0].as<uint8_t>(seqBytes + 16);
    uint32_t*      dCig  = B[LI_BUF_COUNT + 1].as<uint32_t>(cigarWords + 4);
    uint8_t*       dRefs = B[LI_BUF_COUNT + 2].as<uint8_t>(refBytes + 16);
    for (uint32_t l = 0; l < n_loci; ++l) {
      LiLocusDev& u(hLoci[l]);
      u.ref          = dRefs + ref_off[l];
      u.ref_len      = uint32_t(std::min<uint64_t>(ref_off[l + 1] - ref_off[l], 0xffffffffull));
      u.first        = loci[l].first_contig;
      u.n            = (loci[l].status == MANTA_OK) ? loci[l].n_contigs : 0u;
      u.leading_cut  = cuts[l].leading_cut;
      u.trailing_cut = cuts[l].trailing_cut;
      u.status       = loci[l].status;
      for (uint32_t c = 0; c < u.n; ++c) {
        const uint64_t              i = uint64_t(u.first) + c;
        const manta_align_result_t& a(alignments[i].align);
        LiTaskDev&                  t(hTasks[i]);
        t.contig     = dSeq + contigs[i].seq_off;
        t.contig_len = contigs[i].seq_len;
        t.cigar      = dCig + ((a.status == MANTA_OK) ? a.cigar1_off : 0);
        t.n_cigar    = (a.status == MANTA_OK) ? a.cigar1_len : 0u;
        t.begin_pos  = a.begin_pos1;
        t.cons_begin = contigs[i].conservative_begin;
        t.cons_end   = contigs[i].conservative_end;
        t.status     = a.status;
      }
    }
    LiParams L;
    std::memset(&L, 0, sizeof(L));
    LiTaskDev*  dTasks = B[LI_BUF_COUNT + 3].as<LiTaskDev>(nContigs + 1);
    LiLocusDev* dLoci  = B[LI_BUF_COUNT + 4].as<LiLocusDev>(n_loci);
    L.tasks    = dTasks;
    L.units    = dLoci;
    L.n_units  = n_loci;
    L.edge     = liScoresOf(*edge_scores);
    L.complete = liScoresOf(*complete_scores);
    rt::h2d(dSeq, seq_arena, seqBytes);
    rt::h2d(dCig, cigar_arena, 4 * cigarWords);
    rt::h2d(dRefs, refs, refBytes);
    rt::h2d(dTasks, hTasks.data(), sizeof(LiTaskDev) * nContigs);
    rt::h2d(dLoci, hLoci.data(), sizeof(LiLocusDev) * n_loci);
    liLaunch(ctx, L, nContigs, maxContigLen, *complete_scores, B);
    LiHost H;
    H.fetch(L, nContigs);
    return liCompact(ctx, H, nContigs, [&](uint64_t i) { return seen[i] ? int64_t(i) : int64_t(-1); },
                     [&](uint64_t) { return int(MANTA_OK); }, edge_out, li_out, cigar_out, cigar_cap, cigar_used, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" int manta_smallsv_set_large_insertion(manta_smallsv_t* b, const manta_align_scores_t* edge_scores, const manta_align_scores_t* complete_scores)
{
  if (!b) return MANTA_E_INVALID_ARG;
  if (edge_scores && !complete_scores) return fail(b->ctx, MANTA_E_INVALID_ARG, "manta_smallsv_set_large_insertion: complete_scores is null");
  b->liOn  = edge_scores != nullptr;
  b->liRan = false;
  if (edge_scores) {
    b->liEdgeScores     = *edge_scores;
    b->liCompleteScores = *complete_scores;
  }
  return MANTA_OK;
}

extern "C" int manta_smallsv_download_large_insertion(manta_smallsv_t* b, manta_large_insert_edge_t* edge_out, uint64_t edge_cap,
                                                      manta_large_insertion_t* li_out, uint64_t li_cap, uint32_t* cigar_out, uint64_t cigar_cap,
                                                      uint64_t* cigar_used)
{
  static const char* fn = "manta_smallsv_download_large_insertion";
  if (!b) return MANTA_E_INVALID_ARG;
  manta_ctx_t* ctx = b->ctx;
  if (cigar_used) *cigar_used = 0;
  if (!b->ran || !b->liRan)
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": no run with the stage set (manta_smallsv_set_large_insertion, then manta_smallsv_run)");
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(b->main);
    const uint32_t nLoci  = b->nLoci, maxAsm = b->opt.max_assembly_count;
    const uint64_t nSlots = uint64_t(nLoci) * maxAsm;
    std::vector<AsmLocusOut> hLoci(nLoci);
    rt::d2h(hLoci.data(), b->asmStage.dLoci, sizeof(AsmLocusOut) * nLoci);
    LiHost H;
    H.fetch(b->liParams, nSlots);
    // contigs[] of manta_smallsv_download: the loci in order, every locus' contigs in order (AsmStage::compact)
    std::vector<uint64_t> slotOf;
    for (uint32_t l = 0; l < nLoci; ++l)
      if (hLoci[l].status == ASM_OK)
        for (uint32_t c = 0; c < hLoci[l].n_contigs; ++c) slotOf.push_back(uint64_t(l) * maxAsm + c);
    if (slotOf.size() > edge_cap || (!slotOf.empty() && !edge_out) || nLoci > li_cap || (nLoci && !li_out))
      return fail(ctx, MANTA_E_CAPACITY, std::string(fn) + ": record array too small");
    return liCompact(ctx, H, slotOf.size(), [&](uint64_t i) { return int64_t(slotOf[i]); },
                     [&](uint64_t l) { return asmStatusToAbi(hLoci[l].status); }, edge_out, li_out, cigar_out, cigar_cap, cigar_used, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

// ------------------------------------------------------------------------------------------------------
// spanning jump-alignment QC and contig selection (spanning_select_kernels.hpp)
// ------------------------------------------------------------------------------------------------------
extern "C" int manta_spanning_select_batch(
    manta_ctx_t* ctx, const manta_align_scores_t* filter_scores, int32_t is_rna, uint32_t n_loci, const manta_asm_locus_result_t* loci,
    const manta_asm_contig_t* contigs, const manta_spanning_alignment_t* alignments, const uint32_t* cigar_arena, uint64_t cigar_arena_words,
    const uint64_t* bits_arena, uint64_t bits_arena_words, manta_spanning_select_contig_t* contig_out, manta_spanning_select_t* locus_out)
{
  static const char* fn = "manta_spanning_select_batch";
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (!filter_scores || (n_loci && (!loci || !locus_out))) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  // (the reference asserts optimalScore > 0: the score fraction divides by clipped length x match)
  if (filter_scores->match <= 0) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": filter_scores->match must be positive");
  if (is_rna && !bits_arena) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": bits_arena is null in RNA mode");
  if (n_loci == 0) return MANTA_OK;
  uint64_t nContigs = 0;
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (loci[l].status != MANTA_OK || loci[l].n_contigs == 0) continue;
    nContigs = std::max<uint64_t>(nContigs, uint64_t(loci[l].first_contig) + loci[l].n_contigs);
  }
  if (nContigs && (!contigs || !alignments || !contig_out || (cigar_arena_words && !cigar_arena)))
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  std::vector<uint8_t> seen(nContigs + 1, 0);
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (loci[l].status != MANTA_OK) continue;
    for (uint32_t c = 0; c < loci[l].n_contigs; ++c) {
      const uint64_t i = uint64_t(loci[l].first_contig) + c;
      if (seen[i]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": contig record " + std::to_string(i) + " belongs to two loci");
      seen[i] = 1;
    }
  }
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    DevBuf* const   B     = ctx->dSel;
    const uint64_t  nBits = is_rna ? bits_arena_words : 0;
    const uint32_t* dCig  = B[2].as<uint32_t>(cigar_arena_words + 4);
    const uint64_t* dBits = B[3].as<uint64_t>(nBits + 2);
    std::vector<SelTaskDev>  hTasks(nContigs + 1);
    std::vector<SelLocusDev> hLoci(n_loci);
    auto outside = [](uint64_t off, uint64_t len, uint64_t size) { return off > size || len > size - off; };
    for (uint32_t l = 0; l < n_loci; ++l) {
      SelLocusDev& u(hLoci[l]);
      u.first    = loci[l].first_contig;
      u.n        = (loci[l].status == MANTA_OK) ? loci[l].n_contigs : 0u;
      u.status   = loci[l].status;
      u.reserved = 0;
      for (uint32_t c = 0; c < u.n; ++c) {
        const uint64_t              i = uint64_t(u.first) + c;
        const manta_align_result_t& a(alignments[i].align);
        SelTaskDev&                 t(hTasks[i]);
        std::memset(&t, 0, sizeof(t));
        t.status = a.status;
        t.score  = a.score;
        t.cigar1 = t.cigar2 = dCig;
        t.support           = is_rna ? dBits : nullptr;
        if (a.status != MANTA_OK) continue;
        // nothing outside the caller's arenas is ever read
        if (outside(a.cigar1_off, a.cigar1_len, cigar_arena_words) || outside(a.cigar2_off, a.cigar2_len, cigar_arena_words) ||
            (is_rna && outside(contigs[i].support_off, loci[l].n_words, nBits))) {
          t.status = MANTA_E_INVALID_ARG;
          continue;
        }
        t.cigar1   = dCig + a.cigar1_off;
        t.n_cigar1 = a.cigar1_len;
        t.cigar2   = dCig + a.cigar2_off;
        t.n_cigar2 = a.cigar2_len;
        if (is_rna) {
          t.support = dBits + contigs[i].support_off;
          t.n_words = loci[l].n_words;
        }
      }
    }
    SelParams S;
    std::memset(&S, 0, sizeof(S));
    SelTaskDev*  dTasks = B[0].as<SelTaskDev>(nContigs + 1);
    SelLocusDev* dLoci  = B[1].as<SelLocusDev>(n_loci);
    S.tasks   = dTasks;
    S.units   = dLoci;
    S.n_units = n_loci;
    S.is_rna  = is_rna ? 1u : 0u;
    S.sc      = QcScores{filter_scores->match, filter_scores->mismatch, filter_scores->open, filter_scores->extend};
    if (cigar_arena_words) rt::h2d(const_cast<uint32_t*>(dCig), cigar_arena, 4 * cigar_arena_words);
    if (nBits) rt::h2d(const_cast<uint64_t*>(dBits), bits_arena, 8 * nBits);
    rt::h2d(dTasks, hTasks.data(), sizeof(SelTaskDev) * (nContigs + 1));
    rt::h2d(dLoci, hLoci.data(), sizeof(SelLocusDev) * n_loci);
    selLaunch(ctx, S, nContigs, B[4], B[5], B[6]);
    std::vector<SelContigDev>   hC(nContigs + 1);
    std::vector<SelLocusRecDev> hL(n_loci);
    rt::d2hAsync(hC.data(), S.contig_out, sizeof(SelContigDev) * (nContigs + 1));
    rt::d2hAsync(hL.data(), S.locus_out, sizeof(SelLocusRecDev) * n_loci);
    rt::sync();
    selReport(ctx, S, fn);
    return selCompact(ctx, hC, hL, nContigs, [&](uint64_t i) { return seen[i] ? int64_t(i) : int64_t(-1); }, [&](uint64_t) { return int(MANTA_OK); },
                      contig_out, locus_out, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" int manta_spanning_set_select(manta_spanning_t* b, const manta_align_scores_t* filter_scores)
{
  if (!b) return MANTA_E_INVALID_ARG;
  if (filter_scores && filter_scores->match <= 0) return fail(b->ctx, MANTA_E_INVALID_ARG, "manta_spanning_set_select: filter_scores->match must be positive");
  b->selOn  = filter_scores != nullptr;
  b->selRan = false;
  if (filter_scores) b->selScores = *filter_scores;
  return MANTA_OK;
}

extern "C" int manta_spanning_download_select(manta_spanning_t* b, manta_spanning_select_contig_t* contig_out, uint64_t contig_cap,
                                              manta_spanning_select_t* locus_out, uint64_t locus_cap)
{
  static const char* fn = "manta_spanning_download_select";
  if (!b) return MANTA_E_INVALID_ARG;
  manta_ctx_t* ctx = b->ctx;
  if (!b->ran || !b->selOn || !b->selRan)
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": no run with the stage set (manta_spanning_set_select, then manta_spanning_run)");
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(b->main);
    const uint32_t nLoci  = b->nLoci, maxAsm = b->opt.max_assembly_count;
    const uint64_t nSlots = uint64_t(nLoci) * maxAsm;
    std::vector<AsmLocusOut>    hLoci(nLoci);
    std::vector<SelContigDev>   hC(nSlots + 1);
    std::vector<SelLocusRecDev> hL(nLoci);
    rt::d2hAsync(hLoci.data(), b->asmStage.dLoci, sizeof(AsmLocusOut) * nLoci);
    rt::d2hAsync(hC.data(), b->dSelContigs.p, sizeof(SelContigDev) * nSlots);
    rt::d2hAsync(hL.data(), b->dSelLoci.p, sizeof(SelLocusRecDev) * nLoci);
    rt::sync();
    // contigs[] of manta_spanning_download: the loci in order, every locus' contigs in order (AsmStage::compact)
    std::vector<uint64_t> slotOf;
    for (uint32_t l = 0; l < nLoci; ++l)
      if (hLoci[l].status == ASM_OK)
        for (uint32_t c = 0; c < hLoci[l].n_contigs; ++c) slotOf.push_back(uint64_t(l) * maxAsm + c);
    if (slotOf.size() > contig_cap || (!slotOf.empty() && !contig_out) || nLoci > locus_cap || (nLoci && !locus_out))
      return fail(ctx, MANTA_E_CAPACITY, std::string(fn) + ": record array too small");
    return selCompact(ctx, hC, hL, slotOf.size(), [&](uint64_t i) { return int64_t(slotOf[i]); },
                      [&](uint64_t l) { return asmStatusToAbi(hLoci[l].status); }, contig_out, locus_out, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

// ------------------------------------------------------------------------------------------------------
// small-SV contig ranking and refined candidate ranges (smallsv_select_kernels.hpp)
// ------------------------------------------------------------------------------------------------------
extern "C" int manta_smallsv_select_batch(
    manta_ctx_t* ctx, uint32_t n_loci, const manta_asm_locus_result_t* loci, const manta_asm_contig_t* contigs,
    const manta_smallsv_alignment_t* alignments, const manta_smallsv_qc_t* qc, const uint32_t* seg_arena, uint64_t seg_pairs_used,
    const uint8_t* seq_arena, uint64_t seq_arena_used, const uint32_t* cigar_arena, uint64_t cigar_arena_used, const uint64_t* bits_arena,
    uint64_t bits_arena_used, const uint8_t* refs, const uint64_t* ref_off, manta_smallsv_select_t* locus_out,
    manta_small_cand_sv_t* cand_out, uint64_t cand_cap, uint64_t* cand_used)
{
  static const char* fn = "manta_smallsv_select_batch";
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (cand_used) *cand_used = 0;
  if (n_loci && (!loci || !ref_off || !locus_out)) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  if (n_loci == 0) return MANTA_OK;
  uint64_t nContigs = 0;
  for (uint32_t l = 0; l < n_loci; ++l) {
    if (ref_off[l + 1] < ref_off[l]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": ref_off not monotone");
    if (loci[l].status != MANTA_OK || loci[l].n_contigs == 0) continue;
    nContigs = std::max<uint64_t>(nContigs, uint64_t(loci[l].first_contig) + loci[l].n_contigs);
  }
  const uint64_t refBytes = ref_off[n_loci];
  if (nContigs && (!contigs || !alignments || !qc || (seg_pairs_used && !seg_arena) || (seq_arena_used && !seq_arena) ||
                   (cigar_arena_used && !cigar_arena) || (bits_arena_used && !bits_arena) || (refBytes && !refs)))
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  try {  // (every allocation sized by the caller's records is inside: nothing may leave through the C boundary)
    std::vector<uint8_t> seen(nContigs + 1, 0);
    for (uint32_t l = 0; l < n_loci; ++l) {
      if (loci[l].status != MANTA_OK) continue;
      for (uint32_t c = 0; c < loci[l].n_contigs; ++c) {
        const uint64_t i = uint64_t(loci[l].first_contig) + c;
        if (seen[i]) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": contig record " + std::to_string(i) + " belongs to two loci");
        seen[i] = 1;
      }
    }
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    DevBuf* const   B     = ctx->dSs;
    const uint32_t* dCig  = B[2].as<uint32_t>(cigar_arena_used + 4);
    const uint64_t* dBits = B[3].as<uint64_t>(bits_arena_used + 2);
    const uint32_t* dSegs = B[4].as<uint32_t>(2 * seg_pairs_used + 4);
    const uint8_t*  dSeq  = B[5].as<uint8_t>(seq_arena_used + 16);
    const uint8_t*  dRefs = B[6].as<uint8_t>(refBytes + 16);
    std::vector<SsTaskDev>  hTasks(nContigs + 1);
    std::vector<SsLocusDev> hLoci(n_loci);
    auto outside = [](uint64_t off, uint64_t len, uint64_t size) { return off > size || len > size - off; };
    for (uint32_t l = 0; l < n_loci; ++l) {
      SsLocusDev& u(hLoci[l]);
      u.first   = loci[l].first_contig;
      u.n       = (loci[l].status == MANTA_OK) ? loci[l].n_contigs : 0u;
      u.status  = loci[l].status;
      u.ref     = dRefs + ref_off[l];
      u.ref_len = uint32_t(std::min<uint64_t>(ref_off[l + 1] - ref_off[l], 0xffffffffull));
      for (uint32_t c = 0; c < u.n; ++c) {
        const uint64_t              i = uint64_t(u.first) + c;
        const manta_align_result_t& a(alignments[i].align);
        SsTaskDev&                  t(hTasks[i]);
        std::memset(&t, 0, sizeof(t));
        t.contig  = dSeq;
        t.cigar   = dCig;
        t.support = dBits;
        t.segs    = dSegs;
        t.status  = (a.status != MANTA_OK) ? a.status : qc[i].status;
        if (t.status != MANTA_OK) continue;
        // nothing outside the caller's arenas is ever read
        if (outside(a.cigar1_off, a.cigar1_len, cigar_arena_used) || outside(qc[i].seg_off, qc[i].n_segments, seg_pairs_used) ||
            qc[i].n_segments > SS_MAX_CANDS || outside(contigs[i].support_off, loci[l].n_words, bits_arena_used) ||
            outside(contigs[i].seq_off, contigs[i].seq_len, seq_arena_used)) {
          t.status = MANTA_E_INVALID_ARG;
          continue;
        }
        t.contig        = dSeq + contigs[i].seq_off;
        t.contig_len    = contigs[i].seq_len;
        t.cigar         = dCig + a.cigar1_off;
        t.n_cigar       = a.cigar1_len;
        t.support       = dBits + contigs[i].support_off;
        t.n_words       = loci[l].n_words;
        t.segs          = dSegs + 2 * qc[i].seg_off;
        t.n_segs        = qc[i].n_segments;
        t.begin_pos     = a.begin_pos1;
        t.score         = a.score;
        t.is_jumped     = a.is_jumped ? 1u : 0u;
        t.is_candidate  = qc[i].is_candidate;
        t.largest_indel = qc[i].largest_indel;
      }
    }
    SsParams S;
    std::memset(&S, 0, sizeof(S));
    SsTaskDev*  dTasks = B[0].as<SsTaskDev>(nContigs + 1);
    SsLocusDev* dLoci  = B[1].as<SsLocusDev>(n_loci);
    S.tasks   = dTasks;
    S.units   = dLoci;
    S.n_units = n_loci;
    if (cigar_arena_used) rt::h2d(const_cast<uint32_t*>(dCig), cigar_arena, 4 * cigar_arena_used);
    if (bits_arena_used) rt::h2d(const_cast<uint64_t*>(dBits), bits_arena, 8 * bits_arena_used);
    if (seg_pairs_used) rt::h2d(const_cast<uint32_t*>(dSegs), seg_arena, 8 * seg_pairs_used);
    if (seq_arena_used) rt::h2d(const_cast<uint8_t*>(dSeq), seq_arena, seq_arena_used);
    if (refBytes) rt::h2d(const_cast<uint8_t*>(dRefs), refs, refBytes);
    rt::h2d(dTasks, hTasks.data(), sizeof(SsTaskDev) * (nContigs + 1));
    rt::h2d(dLoci, hLoci.data(), sizeof(SsLocusDev) * n_loci);
    ssLaunch(ctx, S, B[7], B[8], B[9]);
    std::vector<SsLocusRecDev> hL(n_loci);
    std::vector<SsCandDev>     hC(uint64_t(n_loci) * SS_MAX_CANDS);
    rt::d2hAsync(hL.data(), S.locus_out, sizeof(SsLocusRecDev) * n_loci);
    rt::d2hAsync(hC.data(), S.cand_out, sizeof(SsCandDev) * hC.size());
    rt::sync();
    ssReport(ctx, S, fn);
    return ssCompact(ctx, hL, hC, [&](uint64_t) { return int(MANTA_OK); }, locus_out, cand_out, cand_cap, cand_used, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" int manta_small_cand_sv_batch(
    manta_ctx_t* ctx, uint32_t n_tasks, const manta_small_cand_sv_task_t* tasks, const uint8_t* seq_arena, uint64_t seq_bytes,
    const uint32_t* cigar_arena, uint64_t cigar_words, manta_small_cand_sv_t* out)
{
  static const char* fn = "manta_small_cand_sv_batch";
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (n_tasks == 0) return MANTA_OK;
  if (!tasks || !out || (seq_bytes && !seq_arena) || (cigar_words && !cigar_arena)) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    DevBuf* const   B    = ctx->dSs;
    const uint32_t* dCig = B[2].as<uint32_t>(cigar_words + 4);
    const uint8_t*  dSeq = B[5].as<uint8_t>(seq_bytes + 16);
    std::vector<SsCandTaskDev> host(n_tasks);
    auto outside = [](uint64_t off, uint64_t len, uint64_t size) { return off > size || len > size - off; };
    for (uint32_t i = 0; i < n_tasks; ++i) {
      const manta_small_cand_sv_task_t& t(tasks[i]);
      SsCandTaskDev&                    d(host[i]);
      std::memset(&d, 0, sizeof(d));
      d.ref = d.contig = dSeq;
      d.cigar     = dCig;
      d.seg_first = t.seg_first;
      d.seg_last  = t.seg_last;
      // nothing outside the caller's arenas is ever read
      if (outside(t.ref_off, t.ref_len, seq_bytes) || outside(t.contig_off, t.contig_len, seq_bytes) || outside(t.cigar_off, t.cigar_len, cigar_words)) {
        d.status = MANTA_E_INVALID_ARG;
        continue;
      }
      d.ref        = dSeq + t.ref_off;
      d.contig     = dSeq + t.contig_off;
      d.cigar      = dCig + t.cigar_off;
      d.ref_len    = t.ref_len;
      d.contig_len = t.contig_len;
      d.n_cigar    = t.cigar_len;
      d.begin_pos  = t.begin_pos;
    }
    SsCandParams P;
    std::memset(&P, 0, sizeof(P));
    SsCandTaskDev* dTasks = B[0].as<SsCandTaskDev>(n_tasks);
    P.tasks   = dTasks;
    P.n_tasks = n_tasks;
    P.out     = B[8].as<SsCandDev>(n_tasks);
    P.counter = B[9].as<uint32_t>(4);
    if (cigar_words) rt::h2d(const_cast<uint32_t*>(dCig), cigar_arena, 4 * cigar_words);
    if (seq_bytes) rt::h2d(const_cast<uint8_t*>(dSeq), seq_arena, seq_bytes);
    rt::h2d(dTasks, host.data(), sizeof(SsCandTaskDev) * n_tasks);
    rt::dzero(P.counter, 16);
    rt::launch(small_cand_sv_kernel, qcGrid(ctx, n_tasks), 0, P);
    std::vector<SsCandDev> hC(n_tasks);
    rt::d2h(hC.data(), P.out, sizeof(SsCandDev) * n_tasks);
    int worst = MANTA_OK;
    for (uint32_t i = 0; i < n_tasks; ++i) {
      ssCandToAbi(hC[i], out[i]);
      if (out[i].status != MANTA_OK) worst = out[i].status;
    }
    if (worst != MANTA_OK) return fail(ctx, worst, std::string(fn) + ": one or more tasks failed; see per-item status");
    return MANTA_OK;
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" int manta_smallsv_set_select(manta_smallsv_t* b, int32_t on)
{
  if (!b) return MANTA_E_INVALID_ARG;
  if (on && !b->qcOn) return fail(b->ctx, MANTA_E_INVALID_ARG, "manta_smallsv_set_select: contig QC is not set (manta_smallsv_set_qc first)");
  b->ssOn  = on != 0;
  b->ssRan = false;
  return MANTA_OK;
}

extern "C" int manta_smallsv_download_select(manta_smallsv_t* b, manta_smallsv_select_t* locus_out, uint64_t locus_cap,
                                             manta_small_cand_sv_t* cand_out, uint64_t cand_cap, uint64_t* cand_used)
{
  static const char* fn = "manta_smallsv_download_select";
  if (!b) return MANTA_E_INVALID_ARG;
  manta_ctx_t* ctx = b->ctx;
  if (cand_used) *cand_used = 0;
  if (!b->ran || !b->ssOn || !b->ssRan)
    return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": no run with the stage set (manta_smallsv_set_qc, manta_smallsv_set_select, then manta_smallsv_run)");
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(b->main);
    const uint32_t nLoci = b->nLoci;
    if (nLoci > locus_cap || (nLoci && !locus_out)) return fail(ctx, MANTA_E_CAPACITY, std::string(fn) + ": record array too small");
    std::vector<AsmLocusOut>   hLoci(nLoci);
    std::vector<SsLocusRecDev> hL(nLoci);
    std::vector<SsCandDev>     hC(uint64_t(nLoci) * SS_MAX_CANDS);
    rt::d2hAsync(hLoci.data(), b->asmStage.dLoci, sizeof(AsmLocusOut) * nLoci);
    rt::d2hAsync(hL.data(), b->dSsLoci.p, sizeof(SsLocusRecDev) * nLoci);
    rt::d2hAsync(hC.data(), b->dSsCands.p, sizeof(SsCandDev) * hC.size());
    rt::sync();
    return ssCompact(ctx, hL, hC, [&](uint64_t l) { return asmStatusToAbi(hLoci[l].status); }, locus_out, cand_out, cand_cap, cand_used, fn);
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

extern "C" int manta_seq_match_count_batch(
    manta_ctx_t* ctx, uint32_t n_tasks, const manta_seq_match_task_t* tasks, const uint8_t* seq_arena, uint64_t seq_bytes, uint32_t* counts)
{
  static const char* fn = "manta_seq_match_count_batch";
  if (!ctx) return MANTA_E_INVALID_ARG;
  if (n_tasks == 0) return MANTA_OK;
  if (!tasks || !counts || (seq_bytes && !seq_arena)) return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": null argument");
  try {
    rt::setDevice(ctx->deviceId);
    rt::ScopedStream onStream(ctx->stream);
    uint8_t*                     dSeq = ctx->dQc[5].as<uint8_t>(seq_bytes + 16);
    std::vector<SeqMatchTaskDev> host(n_tasks);
    auto outside = [&](uint64_t off, uint64_t len) { return off > seq_bytes || len > seq_bytes - off; };
    for (uint32_t i = 0; i < n_tasks; ++i) {
      const manta_seq_match_task_t& t(tasks[i]);
      if (outside(t.target_off, t.target_len) || outside(t.query_off, t.query_len))
        return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": task " + std::to_string(i) + " outside the arena");
      if (t.query_len == 0xffffffffu)  // (the kernel's "never abandoned" fail count is query_len + 1)
        return fail(ctx, MANTA_E_INVALID_ARG, std::string(fn) + ": task " + std::to_string(i) + ": query_len must be below 2^32 - 1");
      host[i].target            = dSeq + t.target_off;
      host[i].query             = dSeq + t.query_off;
      host[i].target_len        = t.target_len;
      host[i].query_len         = t.query_len;
      host[i].max_mismatch_rate = t.max_mismatch_rate;
      host[i].reserved          = 0;
    }
    SeqMatchParams   P;
    SeqMatchTaskDev* dTasks = ctx->dQc[0].as<SeqMatchTaskDev>(n_tasks);
    P.tasks   = dTasks;
    P.n_tasks = n_tasks;
    P.counts  = ctx->dQc[1].as<uint32_t>(n_tasks);
    P.counter = ctx->dQc[3].as<uint32_t>(4);
    rt::h2d(dSeq, seq_arena, seq_bytes);
    rt::h2d(dTasks, host.data(), sizeof(SeqMatchTaskDev) * n_tasks);
    rt::dzero(P.counter, 16);
    rt::launch(seq_match_count_kernel, qcGrid(ctx, n_tasks), QC_LDS_BYTES, P);
    rt::d2h(counts, P.counts, sizeof(uint32_t) * n_tasks);
    return MANTA_OK;
  } catch (const std::exception& e) {
    return fail(ctx, MANTA_E_HIP, e.what());
  }
}

#ifdef MANTA_WAVE_EMU
/// tests/emu only: speculation statistics of contig_kernel since the last call (loci done by it, walk rounds, walks,
/// accepted candidates, cache evictions)
extern "C" void manta_emu_fast_stats(unsigned long long* out)
{
  unsigned long long* v = manta_dev::fastStats();
  for (int i = 0; i < 8; ++i) {
    out[i] = v[i];
    v[i]   = 0;
  }
}
#endif

