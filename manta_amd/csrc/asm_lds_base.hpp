// What the two graph kernels of the LDS assembler pipeline share: LdsGraph (asm_lds.hpp, graph_kernel) and LdsGraphL (asm_lds_big.hpp,
// graph_big_kernel) derive from LdsGraphBase<their traits>.  One copy of
//   * the team helpers, the 2-bit keys and their hash, the N-window test;
//   * pack() in steps: the descriptor scan (scanPile) and the fill (fillPile: packed-pile copy or 16-byte staging + conversion).  The
//     fit test between the two is the class' own (lgPileFits / lglPileFits, the big class' pseudo reads);
//   * the first half of readOffsets(): anchors -> parent chains -> offsets, the trees' roots by pointer jumping (anchorForest).  How stray
//     trees are tied to each other afterwards differs by class and stays there;
//   * the two inner pieces of an LSD radix pass: digit bases from the waves' histograms, the scatter of one 64-element step;
//   * the tail of a locus' slab (writeSlab) and the kernels' persistent loop over the queue (lgGraphLoop).
// A class enters only through the constants of its traits (LgGraphS / LgGraphL: field widths, capacities, places in its LDS map): the
// bodies here hold no branch that picks one class' algorithm.  Table pass, records and speculation list differ by design and are not here.
// Everything is WV_DEV (force-inlined): a kernel's code is what it was with the text written out in its struct.
//
// Included by asm_lds.hpp in front of LdsGraph (it needs AsmParams, LgParams and Key from there).
#pragma once

namespace manta_dev {

/// graph_kernel's numbers for the shared bodies (the LG_OFF_* map and the header words are asm_lds.hpp's)
struct LgGraphS {
  static const unsigned CWO_BITS    = 11;  ///< read descriptor {code dword offset : CWO_BITS, length : 16, has N : 1}
  static const unsigned ANCH_BITS   = 15;  ///< anchor {packed base index there : ANCH_BITS, position here}
  static const unsigned MAX_READS   = LG_MAX_READS;
  static const unsigned JUMP_ROUNDS = 7;   ///< pointer jumping over a forest of MAX_READS reads
  static const unsigned OFF_HDR = LG_OFF_HDR, OFF_RD = LG_OFF_RD, OFF_RDM = LG_OFF_RDM, OFF_DYN = LG_OFF_DYN;
  static const unsigned OFF_RST   = LG_OFF_HDR + 256;           ///< u16[128] byte offset of a read in the staged pile
  static const unsigned OFF_PAR   = LG_OFF_HDR + 4 * LG_H_PAR;
  static const unsigned OFF_STAGE = LG_OFF_SETS;                ///< the sets' bytes, unused until the table pass
  static const unsigned OFF_ANCH = LG_OFF_ANCH, OFF_DBASE = LG_OFF_DBASE, OFF_WHIST = LG_OFF_WHIST;
  static const unsigned OFF_SIB = LG_OFF_SIB, SIDE_U16 = 4 * (LG_SIB_CAP + 2 * LG_OVF_CAP);  ///< the three side tables, back to back
  static const unsigned H_SLOT = LG_H_SLOT, H_FLAG = LG_H_FLAG, H_TOT = LG_H_TOT, H_NSIB = LG_H_NSIB, H_NSOVF = LG_H_NSOVF, H_NPOVF = LG_H_NPOVF;
};

template <class C>
struct LdsGraphBase {
  typedef C Map;
  static const unsigned RPL      = C::MAX_READS / 64;  ///< reads per lane where one wave handles all reads
  static const unsigned CWO_MASK = (1u << C::CWO_BITS) - 1u, LEN_SH = C::CWO_BITS, HASN_SH = C::CWO_BITS + 16;
  const AsmParams& P;
  const LgParams&  G;
  char*            lds;
  unsigned         tw, tn, lane;
  uint32_t *       hdr, *rd, *dbase, *whist, *codes, *nmask;
  uint16_t *       rdm, *rstart;
  unsigned         nNormal, nReads, W, k, codeWords;  ///< nReads: nNormal + the big class' pseudo reads of a later word length
  unsigned         nNodes, nFat, nEligible, lowTier;  ///< the sort's results: words, words with more than one read, seeds, first id of the low count tiers
  uint64_t         tMark;

  WV_DEV LdsGraphBase(const AsmParams& p, const LgParams& g, char* base) : P(p), G(g), lds(base)
  {
    tw     = unsigned(wv::wave_in_wg());
    tn     = unsigned(wv::wg_waves());
    lane   = unsigned(wv::lane());
    hdr    = reinterpret_cast<uint32_t*>(lds + C::OFF_HDR);
    rd     = reinterpret_cast<uint32_t*>(lds + C::OFF_RD);
    rdm    = reinterpret_cast<uint16_t*>(lds + C::OFF_RDM);
    rstart = reinterpret_cast<uint16_t*>(lds + C::OFF_RST);
    dbase  = reinterpret_cast<uint32_t*>(lds + C::OFF_DBASE);
    whist  = reinterpret_cast<uint32_t*>(lds + C::OFF_WHIST);
    codes  = reinterpret_cast<uint32_t*>(lds + C::OFF_DYN);
    nmask  = codes;
  }

  /// per-phase shader clocks of the workgroup's first wave (-DMANTA_ASM_PROFILE).  -DMANTA_LG_PROFILE_GRAPH: the eight counters
  /// split the graph kernel alone (`fine`; contig_kernel counts nothing then)
  ///   graph_kernel      0 pack, 1 table, 2 successor links, 3 counts + radix passes, 4 ties + ids, 5 slab + bitsets + record init,
  ///                     6 predecessors + siblings, 7 speculation list + slab write
  ///   graph_big_kernel  coarse (graph_kernel's slots): 0 pack, 1 table + offsets, 2 sort + records, 4 slab.  fine: 0 pack, 1 table,
  ///                     2 reads' offsets, 3 sort, 4 sets to the slab + slot rewrite + filter, 5 links, 6 speculation list, 7 slab write
  WV_DEV void tick(const int phase, const int fine)
  {
#ifdef MANTA_ASM_PROFILE
    const uint64_t now = wv::clock();
#ifdef MANTA_LG_PROFILE_GRAPH
    const int slot = fine;
#else
    const int slot = phase;
#endif
    if (P.phase_cycles && tw == 0 && lane == 0) wv::atomic_add(&P.phase_cycles[slot], (unsigned long long)(now - tMark));
    tMark = now;
#else
    (void)phase;
    (void)fine;
#endif
  }

  /// every wave of the workgroup has written what the others read next
  WV_DEV void teamSync() const
  {
    wv::sync();
    wv::wg_barrier();
  }
  WV_DEV unsigned tid() const { return 64 * tw + lane; }
  WV_DEV unsigned nThreads() const { return 64 * tn; }

  // ---- keys (2-bit codes, 16 bases per dword, MSB first: dword order == base order) ----
  template <int KW>
  WV_DEV Key<KW> keyAt(const unsigned pb) const
  {
    Key<KW>        key;
    const unsigned kw = (k + 15) >> 4;
    const unsigned wi = pb >> 4, sh = (pb & 15) * 2;
    uint32_t       raw[KW + 1];
    for (int i = 0; i <= KW; ++i) raw[i] = (unsigned(i) <= kw) ? codes[wi + i] : 0u;
    for (int i = 0; i < KW; ++i) {
      uint32_t v = 0;
      if (unsigned(i) < kw) {
        v                   = uint32_t((((uint64_t(raw[i]) << 32) | raw[i + 1]) << sh) >> 32);
        const unsigned have = k - 16u * unsigned(i);
        if (have < 16) v &= ~((1u << (32 - 2 * have)) - 1u);
      }
      key.w[i] = v;
    }
    return key;
  }
  template <int KW>
  WV_DEV static bool keyEq(const Key<KW>& a, const Key<KW>& b)
  {
    bool eq = true;
    for (int i = 0; i < KW; ++i) eq = eq && (a.w[i] == b.w[i]);
    return eq;
  }
  template <int KW>
  WV_DEV static bool keyLess(const Key<KW>& a, const Key<KW>& b)
  {
    for (int i = 0; i < KW; ++i)
      if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
    return false;
  }
  template <int KW>
  WV_DEV void keySetBase(Key<KW>& key, const unsigned i, const unsigned c) const
  {
    const unsigned sh = 30 - 2 * (i & 15);
    for (int w = 0; w < KW; ++w)
      if (unsigned(w) == (i >> 4)) key.w[w] = (key.w[w] & ~(3u << sh)) | (c << sh);
  }
  /// word[1..k-1] + c
  template <int KW>
  WV_DEV Key<KW> keyShiftAppend(const Key<KW>& key, const unsigned c) const
  {
    Key<KW> r;
    for (int w = 0; w < KW; ++w) r.w[w] = (key.w[w] << 2) | ((w + 1 < KW) ? (key.w[w + 1] >> 30) : 0u);
    keySetBase(r, k - 1, c);
    return r;
  }
  /// c + word[0..k-2]
  template <int KW>
  WV_DEV Key<KW> keyShiftPrepend(const Key<KW>& key, const unsigned c) const
  {
    Key<KW> r;
    for (int w = 0; w < KW; ++w) r.w[w] = (key.w[w] >> 2) | ((w > 0) ? (key.w[w - 1] << 30) : (c << 30));
    // drop the base that moved to position k
    const unsigned kw = (k + 15) >> 4;
    for (int w = 0; w < KW; ++w) {
      if (unsigned(w) >= kw) {
        r.w[w] = 0;
      } else if (unsigned(w) == kw - 1) {
        const unsigned have = k - 16u * unsigned(w);
        if (have < 16) r.w[w] &= ~((1u << (32 - 2 * have)) - 1u);
      }
    }
    return r;
  }
  /// hash of a key: the bucket from its low bits, the tag from its high bits (how many of each is the class' table's business)
  template <int KW>
  WV_DEV uint32_t keyHash(const Key<KW>& key) const
  {
    const unsigned kw = (k + 15) >> 4;
    uint32_t       h  = 0x811C9DC5u;
    for (int i = 0; i < KW; ++i)
      if (unsigned(i) < kw) h = hashMix(h, key.w[i]);
    h ^= h >> 13;
    h *= 0x85EBCA6Bu;
    h ^= h >> 16;
    return h;
  }
  WV_DEV uint32_t prefix32(const unsigned pb) const  // the word's first 16 bases (fewer: zero padded)
  {
    const unsigned wi = pb >> 4, sh = (pb & 15) * 2;
    uint32_t       v  = codes[wi];
    if (sh) v = (v << sh) | (codes[wi + 1] >> (32 - sh));
    if (k < 16) v &= ~((1u << (32 - 2 * k)) - 1u);
    return v;
  }
  /// byte `b` of the word at pile position pb: its bases [4 b, 4 b + 4) as eight bits, bases beyond the word length read as zero.  Comparing
  /// words byte by byte from b = 0 is comparing their text (2-bit codes, A < C < G < T): the digits of the big class' radix sorts.
  WV_DEV unsigned keyByte(const unsigned pb, const unsigned b) const
  {
    const unsigned at = pb + 4 * b, wi = at >> 4, sh = (at & 15) * 2;
    uint32_t       v  = codes[wi] << sh;
    if (sh > 24) v |= codes[wi + 1] >> (32 - sh);
    v >>= 24;
    const unsigned have = k - 4 * b;  // (callers pass b < ceil(k / 4))
    if (have < 4) v &= ~((1u << (8 - 2 * have)) - 1u);
    return v;
  }

  WV_DEV bool windowHasN(const unsigned maskWordBase, const unsigned j) const
  {
    unsigned pos = j, left = k;
    while (left > 0) {
      const unsigned wi = pos >> 5, bit = pos & 31;
      const unsigned take = (32 - bit < left) ? (32 - bit) : left;
      uint32_t       m    = nmask[maskWordBase + wi] >> bit;
      if (take < 32) m &= (1u << take) - 1u;
      if (m) return true;
      pos += take;
      left -= take;
    }
    return false;
  }

  WV_DEV uint64_t plShift(const unsigned locus, const unsigned i) const
  {
    return P.pl_chunk_shift ? P.pl_chunk_shift[3 * size_t(locus / P.chunk_loci) + i] : uint64_t(0);
  }

  // ------------------------------------------------------------------------------------------------
  // stage 0: the locus' reads -> 2 bit + N bitmap in LDS, from any of the three input forms (1 byte per base, the same
  // arriving chunk by chunk behind the running kernel, packed piles).  A class' pack() is: scanPile, its own fit test, fillPile.
  // ------------------------------------------------------------------------------------------------
  /// what the descriptor scan found: the locus' first read, code / N-bitmap dwords (with a padding dword per read) and bases of the
  /// pile, whether a read's length does not fit the descriptors' 16 bits, the packed input's chunk shifts
  struct Pile {
    unsigned rBegin, cw, mw, nb;
    bool     tooLong;
    uint64_t plR, plC, plM;
  };
  /// nNormal, W and the reads' descriptors (rd, rdm, rstart).  False: more reads than the descriptor arrays hold.
  /// (every wave computes the same offsets; wave 0 writes them)
  WV_DEV bool scanPile(const unsigned locus, Pile& s)
  {
    const unsigned rBegin = P.locus_read_begin[locus], rEnd = P.locus_read_begin[locus + 1];
    nNormal               = rEnd - rBegin;
    if (nNormal + 2 * P.opt.maxAssemblyCount > C::MAX_READS) return false;
    W = (nNormal + 2 * P.opt.maxAssemblyCount + 63) / 64;
    if (W == 0) W = 1;
    const uint64_t plR = plShift(locus, 0);
    unsigned       cw = 0, mw = 0, nb = 0;  // code dwords, N-bitmap dwords, bases so far
    bool           tooLong = false;
    for (unsigned base = 0; base < nNormal; base += 64) {
      const unsigned r   = base + lane;
      unsigned       len = 0;
      if (r < nNormal) len = P.pl_codes ? P.pl_read_len[rBegin + r + plR] : unsigned(P.read_off[rBegin + r + 1] - P.read_off[rBegin + r]);
      if (len > 0xffffu) tooLong = true;
      const unsigned myC = (r < nNormal) ? (len + 15) / 16 + 1 : 0u;  // +1 padding dword so key fetches may read one past
      const unsigned myM = (r < nNormal) ? (len + 31) / 32 + 1 : 0u;
      unsigned       sc = myC, sm = myM, sb = (r < nNormal) ? len : 0u;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned oc = wv::shfl(sc, wv::lane() - off), om = wv::shfl(sm, wv::lane() - off), ob = wv::shfl(sb, wv::lane() - off);
        if (wv::lane() >= off) {
          sc += oc;
          sm += om;
          sb += ob;
        }
      }
      const unsigned cwo = cw + sc - myC, mwo = mw + sm - myM;
      if (tw == 0 && r < nNormal && cwo <= CWO_MASK && nb + sb - len <= 0xffffu) {  // (what does not fit its field is refused by the fit test)
        rd[r]     = cwo | ((len & 0xffffu) << LEN_SH);
        rdm[r]    = uint16_t(mwo);
        rstart[r] = uint16_t(nb + sb - len);
      }
      cw += wv::readlane(sc, 63);
      mw += wv::readlane(sm, 63);
      nb += wv::readlane(sb, 63);
    }
    s = Pile{rBegin, cw, mw, nb, wv::any(tooLong), plR, plShift(locus, 1), plShift(locus, 2)};
    return true;
  }
  /// the reads' codes and N bitmaps behind the descriptors (s.cw: the code dwords of everything in the pile; the reads scanned are
  /// its first nNormal).  False: a byte outside {A,C,G,T,N}.
  WV_DEV bool fillPile(const unsigned locus, const Pile& s)
  {
    const unsigned rBegin = s.rBegin, cw = s.cw, mw = s.mw;
    const unsigned cwPad  = (cw + 2 + 3) & ~3u;
    codeWords = cw + 2;
    nmask     = codes + cwPad;
    for (unsigned i = tid(); i < mw + 2; i += nThreads()) nmask[i] = 0;
    if (tid() == 0) hdr[C::H_FLAG] = 0;
    teamSync();
    if (P.pl_codes) {  // packed piles arrive in this layout: copy, 8 lanes per read
      for (unsigned base = 8 * tw; base < nNormal; base += 8 * tn) {
        const unsigned r = base + (lane >> 3);
        if (r >= nNormal) continue;
        const unsigned  d = rd[r], cwo = d & CWO_MASK, len = (d >> LEN_SH) & 0xffffu, mwo = rdm[r];
        const unsigned  nCw = (len + 15) / 16, nMw = (len + 31) / 32;
        const uint32_t* sc  = P.pl_codes + (P.pl_code_off[rBegin + r + s.plR] + s.plC);
        const uint32_t* sm  = P.pl_nmask + (P.pl_mask_off[rBegin + r + s.plR] + s.plM);
        for (unsigned wi = (lane & 7); wi <= nCw; wi += 8) codes[cwo + wi] = (wi < nCw) ? sc[wi] : 0u;
        bool sawN = false;
        for (unsigned wi = (lane & 7); wi < nMw; wi += 8) {
          const uint32_t m = sm[wi];
          nmask[mwo + wi]  = m;
          sawN             = sawN || (m != 0);
        }
        if (sawN) wv::atomic_or(&rd[r], 1u << HASN_SH);
      }
      if (tid() < 2) codes[cw + tid()] = 0;
      teamSync();
      return true;
    }
    bool           bad   = false;
    const uint32_t shift = P.chunk_shift ? P.chunk_shift[locus / P.chunk_loci] : 0u;
    // The locus' bases are one contiguous run of the input arena: every thread fetches 16-byte pieces of it into LDS (bytes of the
    // class' map that are unused until the table pass) -- all loads in flight at once, one memory latency for the whole pile -- and
    // the conversion below reads its bytes from there.
    char* const stage = lds + C::OFF_STAGE;
    unsigned    lead  = 0;
    {
      const uintptr_t g0 = reinterpret_cast<uintptr_t>(P.bases + P.read_off[rBegin] + shift);
      lead               = unsigned(g0 & 15);
      const u32x4*   gsrc    = reinterpret_cast<const u32x4*>(g0 - lead);
      const unsigned nChunks = (lead + s.nb + 15) / 16 + 1;  // (+1: the byte funnel reads up to four bytes past a read's last dword; the arena is padded)
      for (unsigned c = tid(); c < nChunks; c += nThreads()) reinterpret_cast<u32x4*>(stage)[c] = gsrc[c];
    }
    teamSync();
    // 8 lanes per read, 8 reads per pass: lane (g, i) converts code dwords i, i+8, ... of read (base + g)
    for (unsigned base = 8 * tw; base < nNormal; base += 8 * tn) {
      const unsigned r = base + (lane >> 3);
      if (r >= nNormal) continue;
      const char*    src = stage + lead + rstart[r];
      const unsigned d = rd[r], cwo = d & CWO_MASK, len = (d >> LEN_SH) & 0xffffu, mwo = rdm[r];
      const unsigned nCw = (len + 15) / 16 + 1;
      bool           sawN = false;
      for (unsigned wi = (lane & 7); wi < nCw; wi += 8) {
        uint32_t code = 0, nbits = 0;
        if (wi * 16 < len) {
          // 16 bases = five aligned dword reads + a byte funnel
          const uintptr_t addr = reinterpret_cast<uintptr_t>(src + wi * 16);
          const uint32_t* ap   = reinterpret_cast<const uint32_t*>(addr & ~uintptr_t(3));
          const unsigned  sh   = unsigned(addr & 3) * 8;
          uint32_t        dw[5];
          for (int q = 0; q < 5; ++q) dw[q] = ap[q];
          for (unsigned q = 0; q < 4; ++q) {
            const uint32_t four = sh ? ((dw[q] >> sh) | (dw[q + 1] << (32 - sh))) : dw[q];
            for (unsigned b4 = 0; b4 < 4; ++b4) {
              const unsigned b = q * 4 + b4;
              const unsigned i = wi * 16 + b;
              unsigned       c = 0;
              if (i < len) {
                c = baseCode(uint8_t(four >> (8 * b4)));
                if (c == 5) bad = true;
                if (c >= 4) {
                  nbits |= (1u << b);
                  c = 0;
                }
              }
              code |= c << (30 - 2 * b);
            }
          }
        }
        codes[cwo + wi] = code;
        if (nbits) {
          wv::atomic_or(&nmask[mwo + (wi >> 1)], (wi & 1) ? (nbits << 16) : nbits);
          sawN = true;
        }
      }
      if (sawN) wv::atomic_or(&rd[r], 1u << HASN_SH);
    }
    if (tid() < 2) codes[cw + tid()] = 0;
    if (wv::any(bad) && lane == 0) wv::atomic_or(&hdr[C::H_FLAG], 1u);  // bytes outside {A,C,G,T,N}: the general path decides what is exact
    teamSync();
    return wv::atomic_load(&hdr[C::H_FLAG]) == 0;
  }

  // ------------------------------------------------------------------------------------------------
  // the reads' offsets on a common axis, first half (see LdsGraph::readOffsets for what they are for)
  // ------------------------------------------------------------------------------------------------
  /// read that owns packed base index pb (the reads' code offsets ascend)
  WV_DEV unsigned readOfPb(const unsigned pb) const
  {
    const unsigned cwd = pb >> 4;
    unsigned       lo = 0, hi = nReads;  // rd[lo].cwo <= cwd < rd[hi].cwo
    while (hi - lo > 1) {
      const unsigned mid = (lo + hi) >> 1;
      if ((rd[mid] & CWO_MASK) <= cwd) lo = mid; else hi = mid;
    }
    return lo;
  }
  /// the offsets' array: i32[MAX_READS] behind the anchors
  WV_DEV int32_t* readOff() const { return reinterpret_cast<int32_t*>(lds + C::OFF_ANCH) + C::MAX_READS; }
  /// the root of a read's tree: u8[MAX_READS] (the histograms are not in use before the sort)
  WV_DEV uint8_t* rootOfRead() const { return reinterpret_cast<uint8_t*>(lds + C::OFF_WHIST); }
  /// ONE wave (RPL reads per lane): the table pass' anchors -> parent chains -> the reads' offsets by pointer doubling (readOff()),
  /// then the root of every read's tree by pointer jumping (rootOfRead()).  A read without an anchor is a root at offset 0.  The lane's
  /// reads' offsets and roots are returned in registers as well.
  WV_DEV void anchorForest(int32_t (&myOff)[RPL], unsigned (&myRoot)[RPL])
  {
    const uint32_t* anch = reinterpret_cast<const uint32_t*>(lds + C::OFF_ANCH);
    int32_t*        off  = readOff();
    uint8_t*        par  = reinterpret_cast<uint8_t*>(lds + C::OFF_PAR);
    unsigned        myPar[RPL];
    for (unsigned h = 0; h < RPL; ++h) {
      const unsigned r = lane + 64 * h;
      myOff[h]  = 0;
      myPar[h]  = r;
      myRoot[h] = r;
      if (r < nReads) {
        const uint32_t a = anch[r];
        if (a != LG_NO_ANCHOR) {
          const unsigned apb = a & ((1u << C::ANCH_BITS) - 1u), j = a >> C::ANCH_BITS;
          const unsigned r0  = readOfPb(apb);
          myPar[h] = r0;
          myOff[h] = int32_t(apb - 16u * (rd[r0] & CWO_MASK)) - int32_t(j);
        }
      }
    }
    wv::sync();  // (every anchor has been read: the offsets take the second half of the same array)
    for (unsigned h = 0; h < RPL; ++h) {
      off[lane + 64 * h] = myOff[h];
      par[lane + 64 * h] = uint8_t(myPar[h]);
    }
    wv::sync();
    for (unsigned round = 0; round < C::JUMP_ROUNDS; ++round) {
      int32_t  po[RPL];
      unsigned pp[RPL];
      for (unsigned h = 0; h < RPL; ++h) {
        po[h] = off[myPar[h]];
        pp[h] = par[myPar[h]];
      }
      wv::sync();
      for (unsigned h = 0; h < RPL; ++h) {
        const unsigned r = lane + 64 * h;
        if (myPar[h] != r) {  // (a root keeps its offset)
          myOff[h] += po[h];
          if (pp[h] == myPar[h]) {  // the parent is a root: done after this addition
            off[r]    = myOff[h];
            par[r]    = uint8_t(r);
            myRoot[h] = myPar[h];
            myPar[h]  = r;
          } else {
            off[r]   = myOff[h];
            par[r]   = uint8_t(pp[h]);
            myPar[h] = pp[h];
          }
        }
      }
      wv::sync();
    }
#ifdef MANTA_WAVE_EMU
    if (std::getenv("MANTA_EMU_PROOF_TRACE"))
      for (unsigned h = 0; h < RPL; ++h)
        if (lane + 64 * h < nReads) std::fprintf(stderr, "  read %u: anchor %08x off %d par %u\n", lane + 64 * h, anch[lane + 64 * h], myOff[h], myPar[h]);
#endif
    // (myRoot is the read a read's offset was completed through: the root for the root's children, a finished inner read for the reads
    // below it.  The roots proper by pointer jumping -- the trees are told apart by them)
    uint8_t* rootOf = rootOfRead();
    for (unsigned h = 0; h < RPL; ++h) rootOf[lane + 64 * h] = uint8_t(myRoot[h]);
    wv::sync();
    for (unsigned round = 0; round < C::JUMP_ROUNDS; ++round) {
      unsigned up[RPL];
      for (unsigned h = 0; h < RPL; ++h) up[h] = rootOf[rootOf[lane + 64 * h]];
      wv::sync();
      for (unsigned h = 0; h < RPL; ++h) rootOf[lane + 64 * h] = uint8_t(up[h]);
      wv::sync();
    }
    for (unsigned h = 0; h < RPL; ++h) myRoot[h] = rootOf[lane + 64 * h];
  }

  // ------------------------------------------------------------------------------------------------
  // the inner pieces of an LSD radix pass of the workgroup over u16 elements (wave w sorts its share in order and counts its digits
  // in hist[256 * w ..]): callers count, sync, radixDigitBases, then radixScatter per 64-element step of their share
  // ------------------------------------------------------------------------------------------------
  /// per digit: running offsets over the waves' counts (left in `hist`), totals; then the digit bases `dbase` (four quarters of 64
  /// digits, dealt out to the waves).  Ends on a team barrier.
  WV_DEV void radixDigitBases(uint32_t* hist)
  {
    for (unsigned q = tw; q < 4; q += tn) {
      const unsigned d   = 64 * q + lane;
      unsigned       run = 0;
      for (unsigned w = 0; w < tn; ++w) {
        const unsigned c  = hist[256 * w + d];
        hist[256 * w + d] = run;
        run += c;
      }
      unsigned inc = run;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = wv::shfl(inc, int(lane) - off);
        if (int(lane) >= off) inc += o;
      }
      dbase[d] = inc - run;  // exclusive inside the quarter
      if (lane == 63) hdr[C::H_TOT + q] = inc;
    }
    teamSync();
    for (unsigned q = tw; q < 4; q += tn) {
      unsigned before = 0;
      for (unsigned p = 0; p < q; ++p) before += hdr[C::H_TOT + p];
      dbase[64 * q + lane] += before;
    }
    teamSync();
  }
  /// one 64-element step: this lane's element `v` with digit `d` (valid: it has one) goes behind the elements of its digit placed so
  /// far -- the lanes of a digit find each other by ballot, keep their order, and the highest of them moves the wave's running offset
  WV_DEV void radixScatter(const bool valid, const unsigned v, const unsigned d, uint16_t* dst, uint32_t* myHist)
  {
    uint64_t peers = wv::ballot(valid);
    for (int bit = 0; bit < 8; ++bit) {
      const bool     on = (d >> bit) & 1u;
      const uint64_t m  = wv::ballot(valid && on);
      peers &= on ? m : ~m;
    }
    unsigned base = 0;
    if (valid) base = dbase[d] + myHist[d];
    wv::sync();
    if (valid) {
      dst[base + unsigned(wv::popc(peers & ((uint64_t(1) << lane) - 1)))] = uint16_t(v);
      if ((peers >> lane) == 1u) myHist[d] += unsigned(wv::popc(peers));  // the highest lane of the digit's group
    }
    wv::sync();
  }

  /// The rest of a locus' slab behind what buildRecords and the speculation list wrote: the records, the three side tables (they lie
  /// back to back in LDS and in the slab: fixed capacities), the pile, and -- thread 0 -- the header and the locus' slab offset.
  WV_DEV void writeSlab(const unsigned locus, const uint64_t off, const LgSlab& SL, const FRec8* nodes, const unsigned nSpec, const unsigned need,
                        const bool acyclic, const unsigned nPseudo, const unsigned nCore)
  {
    uint8_t* slab = G.arena + off;
    FRec8*   gRec = reinterpret_cast<FRec8*>(slab + SL.recs);
    for (unsigned i = tid(); i < nNodes; i += nThreads()) gRec[i] = nodes[i];
    const unsigned  nSib = wv::atomic_load(&hdr[C::H_NSIB]), nSovf = wv::atomic_load(&hdr[C::H_NSOVF]), nPovf = wv::atomic_load(&hdr[C::H_NPOVF]);
    const uint16_t* tsrc = reinterpret_cast<const uint16_t*>(lds + C::OFF_SIB);
    uint16_t*       tdst = reinterpret_cast<uint16_t*>(slab + SL.sib);
    for (unsigned i = tid(); i < C::SIDE_U16; i += nThreads()) tdst[i] = tsrc[i];
    uint32_t* gCodes = reinterpret_cast<uint32_t*>(slab + SL.codes);
    for (unsigned i = tid(); i < codeWords; i += nThreads()) gCodes[i] = codes[i];
    if (tid() == 0) {
      LgHdr h;
      h.nNodes    = nNodes;
      h.nFat      = nFat;
      h.k         = k;
      h.nNormal   = nNormal;
      h.nEligible = nEligible;
      h.nSpec     = nSpec;
      h.nSib      = nSib;
      h.codeWords = codeWords;
      h.W         = W;
      h.need      = need;
      h.nSovf     = nSovf;
      h.nPovf     = nPovf;
      h.acyclic   = acyclic ? 1u : 0u;
      h.nPseudo   = nPseudo;
      h.cyclic    = 0;
      h.nCore     = nCore;
      *reinterpret_cast<LgHdr*>(slab) = h;
      G.slab_off[locus]               = off;
    }
  }
};

/// The body of both graph kernels: persistent workgroups take loci from the queue (P.counter) until `nLoci` are gone.  GRAPH (LdsGraph /
/// LdsGraphL) builds a locus' graph; a locus it does not cover is appended to P.punt_ids (P.punt_count counts them).
template <class GRAPH, int MAXKW>
WV_DEV void lgGraphLoop(const LgArgs& A, const unsigned nLoci)
{
  const AsmParams& P = A.P;
  const LgParams&  G = A.G;
  char*          lds = wv::lds_single();
  uint32_t*      hdr = reinterpret_cast<uint32_t*>(lds + GRAPH::Map::OFF_HDR);
  const unsigned tw  = unsigned(wv::wave_in_wg());
  while (true) {
    if (tw == 0 && wv::lane() == 0) hdr[GRAPH::Map::H_SLOT] = wv::atomic_add(P.counter, 1u);
    wv::sync();
    wv::wg_barrier();
    const unsigned slot = wv::first(wv::atomic_load(&hdr[GRAPH::Map::H_SLOT]));
    if (slot >= nLoci) break;
    const unsigned locus   = P.locus_ids ? P.locus_ids[slot] : slot;
    const bool     arrived = !P.upload_chunks_done || asmWaitUploaded(P, locus);
    bool           ok      = false;
    if (arrived) {
      GRAPH g(P, G, lds);
      ok = g.template run<MAXKW>(locus);
    }
    wv::sync();
    if (tw == 0 && !ok && wv::lane() == 0) P.punt_ids[wv::atomic_add(P.punt_count, 1u)] = locus;
    wv::sync();
    wv::wg_barrier();  // (the slot word is rewritten next)
  }
}

}  // namespace manta_dev
