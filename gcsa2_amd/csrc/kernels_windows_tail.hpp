// kernels_windows_tail.hpp -- what a window search does with its lane's final range, included at the end of kernels_windows_body.hpp
// and of k_strand_seeds (kernels_strands.hpp): the per-window outputs, count(), the seed emission (KMER_WINDOWS_EMIT) and the
// profile fold.  Text, not a function, for the reason given in kernels_windows_body.hpp.  In scope: COUNTS, img, live, gid, lane,
// q, sp, ep, k, out, counts, profiles, window_offsets and, with KMER_WINDOWS_EMIT, `emit`; without KMER_WINDOWS_POSITION also
// `stride`.  No include guard on purpose.
  u64 occ = 0;
  if(live)
  {
    if(out != nullptr) { reinterpret_cast<ulonglong2*>(out)[gid] = make_ulonglong2(sp, ep); }
    if constexpr(COUNTS)
    {
      occ = count_range(img, sp, ep);
      if(counts != nullptr) { counts[gid] = occ; }
    }
  }
#if KMER_WINDOWS_EMIT
  {
    const bool hit = live && !range_empty(sp, ep);
    const u64 ballot = __ballot(hit);
    const u32 hits = u32(__popcll(ballot)), rank = u32(__popcll(ballot & ((u64(1) << lane) - 1)));
    u64 base = 0;
    if(lane == 0 && hits > 0) { base = atomicAdd(emit.cursor, (unsigned long long)hits); }
    base = __shfl(base, 0, 64);
    if(lane == 0 && live)                                      // lane 0 lives in every wavefront that has a window
    {
      const u64 wave = gid / 64;
      emit.base[wave] = u32(base); emit.found[wave] = hits; emit.mask[wave] = ballot;
    }
    const u64 at = base + rank;
    if(hit && at < emit.capacity)
    {
      ulonglong2* dst = reinterpret_cast<ulonglong2*>(emit.recs + 4 * at);
#ifdef KMER_WINDOWS_POSITION
      dst[0] = make_ulonglong2(KMER_WINDOWS_POSITION(gid), k);
#else
      dst[0] = make_ulonglong2((gid - window_offsets[q]) * stride, k);
#endif
      dst[1] = make_ulonglong2(sp, ep);
      emit.counts[at] = occ;
    }
  }
#endif
  if(profiles != nullptr)
  {
    const bool nonempty = live && !range_empty(sp, ep);
    u32 found = (nonempty ? 1u : 0u);
    u64 nodes = (nonempty ? ep + 1 - sp : 0);
    // the read of the lane `o` below, read-back of the own one for lanes < o; dead lanes (q = ~0) form the last segment
    const u32 q_lo = u32(q), q_hi = u32(q >> 32);
#pragma unroll
    for(u32 o = 1; o < 64; o <<= 1)
    {
      const u32 below_lo = __shfl_up(q_lo, o, 64), below_hi = __shfl_up(q_hi, o, 64);     // every lane takes part in a shuffle
      const bool same = lane >= o && below_lo == q_lo && below_hi == q_hi;
      const u32 f = __shfl_up(found, o, 64);
      const u64 nd = __shfl_up(nodes, o, 64);
      if(same) { found += f; nodes += nd; }
      if constexpr(COUNTS)
      {
        const u64 oc = __shfl_up(occ, o, 64);
        if(same) { occ += oc; }
      }
    }
    const u32 next_lo = __shfl_down(q_lo, 1, 64), next_hi = __shfl_down(q_hi, 1, 64);
    const bool tail = live && (lane == 63 || next_lo != q_lo || next_hi != q_hi);
    if(tail && found > 0)                                      // empty windows add nothing
    {
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(profiles + q);
      atomicAdd(dst + 1, (unsigned long long)found);
      atomicAdd(dst + 2, (unsigned long long)nodes);
      if constexpr(COUNTS) { atomicAdd(dst + 3, (unsigned long long)occ); }
    }
  }
