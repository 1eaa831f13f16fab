// kernels_windows_body.hpp -- the body shared by k_kmer_windows and k_kmer_seeds (kernels_windows.hpp), included once inside
// each of them: the search of one window per lane, count(), the seed emission (KMER_WINDOWS_EMIT) and the profiles.  It is
// text, not a function, so that adding a kernel that shares it leaves the code of the existing ones as it was, instruction
// for instruction.  In scope: PAIR, COUNTS, the kernel's parameters (img, patterns, offsets, k, stride, window_offsets, owners,
// total, out, counts, profiles) and, with KMER_WINDOWS_EMIT, `emit` (SeedEmit).  No include guard on purpose.
// KMER_WINDOWS_POSITION(g), which only k_minimizer_seeds (kernels_minimizers.hpp) defines: where in its read window g of the
// batch begins, in the place of j * stride; `stride` is then not used.
// What follows the search -- outputs, count(), emission, profiles -- is kernels_windows_tail.hpp, included at the end, which
// k_strand_seeds (kernels_strands.hpp) shares.
  __shared__ ulonglong2 stage[TPB2 * 8];
  __shared__ Tables2 t;
  if(threadIdx.x < 2 * MAX_SIGMA) { t.crange[threadIdx.x] = img.crange[threadIdx.x]; }
  t.c2c[threadIdx.x] = img.char2comp[threadIdx.x];
  t.c2c[threadIdx.x + TPB2] = img.char2comp[threadIdx.x + TPB2];
  __syncthreads();

  const u64 first = u64(blockIdx.x) * TPB2;            // < total: the grid covers the windows exactly
  const u32 lane = threadIdx.x & 63;
  ulonglong2* wave_stage = stage + (threadIdx.x & ~63u) * 8;
  const u64 gid = first + threadIdx.x;
  const bool live = gid < total;

  u64 q = ~u64(0), sp = 0, ep = img.n - 1, i = 0;
  const u8* p = patterns;
  bool done = true;
  u64 win_code = 0;                            // packed pattern window (k_find2)
  u32 win_used = ~u32(0), win_bad = 0;
  [[maybe_unused]] u32 force_single = 0;       // PAIR: characters that must be consumed by single steps (replay)

  if(live)
  {
    q = owner_in_wave(owners, window_offsets, total, gid, true);
    const u64 at = window_offsets[q], j = gid - at;
    if(j == 0 && profiles != nullptr) { reinterpret_cast<u64*>(profiles + q)[0] = window_offsets[q + 1] - at; }
    if(img.n > 0)                                              // gcsa.h:99 (k >= 1)
    {
#ifdef KMER_WINDOWS_POSITION
      p = patterns + offsets[q] + KMER_WINDOWS_POSITION(gid);
#else
      p = patterns + offsets[q] + j * stride;
#endif
      const u64 len = k;
      u64 word = 0, word_addr = ~u64(0);                       // pattern bytes from aligned 8-byte words
      auto byte_at = [&](u64 pos) -> u32
      {
        const u64 addr = reinterpret_cast<u64>(p) + pos, aligned = addr & ~u64(7);
        if(aligned != word_addr) { word = *reinterpret_cast<const u64*>(aligned); word_addr = aligned; }
        return u32(word >> ((addr & 7) * 8)) & 0xFF;
      };
      const u32 tk = img.kmer_k;
      bool seeded = false;
      if(tk > 0 && len >= tk)
      {
        u64 tix = 0;
        bool fast = true;
        for(u32 c = 0; c < tk; c++)                            // c-th character from the end
        {
          const u32 comp = t.c2c[byte_at(len - 1 - c)];
          fast = fast && (comp - 1 < 4);
          tix |= u64((comp - 1) & 3) << (2 * c);
        }
        if(fast)
        {
          const u64 entry = img.kmer_table[tix];
          sp = entry & SEED_SP_MASK; ep = sp + (entry >> SEED_SP_BITS) - 1;
          fast = (entry >> SEED_SP_BITS) != SEED_WIDE;         // a wide range is not in the table
        }
        if(fast) { i = len - tk; seeded = true; }
      }
      if(!seeded)
      {
        i = len - 1;
        const u32 comp = t.c2c[byte_at(i)];
        sp = t.crange[2 * comp]; ep = t.crange[2 * comp + 1];  // charRange, gcsa.h:101-102, 150-153
      }
      done = range_empty(sp, ep) || i == 0;                    // gcsa.h:103
    }
  }

  while(true)
  {
    if(!__any(!done)) { break; }
    // The next pattern characters as 2-bit codes, refilled once per 24 consumed characters (k_find2's window: position
    // win_top - 1 - r at bits [2r, 2r + 2) of win_code, bit r of win_bad = "not a fast character").  Adjacent lanes read
    // overlapping bytes; the words are aligned and never lie outside those of the window's own bytes.
    if(!done && win_used > 24)
    {
      win_used = 0; win_code = 0; win_bad = 0;
      const u64 count = (i < 32 ? i : 32), low = reinterpret_cast<u64>(p) + i - count, base = low & ~u64(7);
      u64 w[5];
      const u64 last = (low + count - 1) & ~u64(7);             // never read past the word of the last byte needed
#pragma unroll
      for(u32 c = 0; c < 5; c++) { const u64 a = base + 8 * c; w[c] = *reinterpret_cast<const u64*>(a < last ? a : last); }
      for(u32 r = 0; r < count; r++)
      {
        const u64 at = (low - base) + (count - 1 - r);         // byte offset of position win_top - 1 - r
        u64 word = w[0];
#pragma unroll
        for(u32 c = 1; c < 5; c++) { if((at >> 3) == c) { word = w[c]; } }
        const u32 code = u32(t.c2c[u32(word >> ((at & 7) * 8)) & 0xFF]) - 1;
        win_code |= u64(code & 3) << (2 * r);
        win_bad |= u32(code < 4 ? 0 : 1) << r;
      }
    }
    const bool stepping = !done;
    u32 comp = 0, r_sp = 0, r_ep = 0, idx_sp = 0, idx_ep = 0;
    bool pair = false;
    if(stepping)
    {
      if constexpr(PAIR)
      {
        if(force_single == 0 && i >= 2)
        {
          const u32 r = win_used;                              // window slot of position i - 1; i - 2 is slot r + 1
          pair = ((win_bad >> r) & 3) == 0;                    // both are fast characters
          if(pair)
          {
            const u32 c2 = u32(win_code >> (2 * r)) & 3, c1 = u32(win_code >> (2 * r + 2)) & 3;
            u32 b_sp, b_ep;
            pair_block_of(sp, b_sp, r_sp); pair_block_of(ep + 1, b_ep, r_ep);
            const u32 head = (c1 * 4 + c2) * u32(img.flp_nblocks);
            idx_sp = (head + b_sp) | PAIR_FLAG; idx_ep = (head + b_ep) | PAIR_FLAG;
          }
        }
      }
      if(!pair)
      {
        i--;
        if constexpr(PAIR) { force_single -= (force_single > 0 ? 1 : 0); }
        const u32 r = win_used++;
        if((win_bad >> r) & 1)                                 // rare: the byte itself
        {
          const u64 addr = reinterpret_cast<u64>(p) + i;
          comp = t.c2c[u32(*reinterpret_cast<const u64*>(addr & ~u64(7)) >> ((addr & 7) * 8)) & 0xFF];
        }
        else { comp = 1 + (u32(win_code >> (2 * r)) & 3); }
        u32 b_sp, b_ep;
        flb_block_of(sp, b_sp, r_sp); flb_block_of(ep + 1, b_ep, r_ep);
        idx_sp = comp * u32(img.flb_nblocks) + b_sp; idx_ep = comp * u32(img.flb_nblocks) + b_ep;
      }
    }
    PairEnd p_sp = {0, 0, 0}, p_ep = {0, 0, 0};   // a single step keeps (edge, node) in .raw / .node
    const bool need2 = stepping && idx_ep != idx_sp;
    ulonglong2 blk[8];
    fetch_blocks<PAIR>(img.flb, idx_sp, stepping, wave_stage, lane, img.flp);
    if(stepping)
    {
      read_block(wave_stage, lane, blk);
      if(PAIR && pair)
      {
        p_sp = eval_pair(blk, r_sp, false);
        if(idx_ep == idx_sp) { p_ep = eval_pair(blk, r_ep, true); }
      }
      else
      {
        eval_endpoint(blk, r_sp, 0, p_sp.raw, p_sp.node);
        if(idx_ep == idx_sp) { eval_endpoint(blk, r_ep, 1, p_ep.raw, p_ep.node); }
      }
    }
    if(__any(need2))
    {
      __builtin_amdgcn_wave_barrier();
      fetch_blocks<PAIR>(img.flb, idx_ep, need2, wave_stage, lane, img.flp);
      if(need2)
      {
        read_block(wave_stage, lane, blk);
        if(PAIR && pair) { p_ep = eval_pair(blk, r_ep, true); }
        else { eval_endpoint(blk, r_ep, 1, p_ep.raw, p_ep.node); }
      }
    }
    __builtin_amdgcn_wave_barrier();
    if(stepping)
    {
      if(PAIR && pair)
      {
        u64 a = 0, b = 0;
        const u32 outcome = pair_outcome(p_sp, p_ep, idx_ep == idx_sp, a, b);
        if(outcome == 2) { sp = p_sp.node; ep = p_ep.node; i -= 2; win_used += 2; done = (i == 0); }     // neither step empties
        else if(outcome == 1) { sp = a; ep = b; i -= 2; win_used += 2; done = true; }     // the second step empties, gcsa.h:160
        else { force_single = 2; }                             // replayed as two single steps from the unchanged (sp, ep)
      }
      else
      {
        const u64 a = p_sp.raw, b = p_ep.raw - 1;              // edge space
        if(range_empty(a, b)) { sp = a; ep = b; done = true; } // gcsa.h:160
        else { sp = p_sp.node; ep = p_ep.node; done = (i == 0); }   // gcsa.h:161, 103
      }
    }
  }

#include "kernels_windows_tail.hpp"
