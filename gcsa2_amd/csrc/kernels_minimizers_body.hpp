// kernels_minimizers_body.hpp -- the tile walk shared by k_minimizers (kernels_minimizers.hpp) and k_canonical_minimizers
// (kernels_strands.hpp), included once inside each of them and described in front of k_minimizers.  It is text, not a function,
// for the reason given in kernels_windows_body.hpp: the sibling kernel leaves k_minimizers' code as it was.  In scope: PLACE and
// the kernel's parameters (img, patterns, offsets, n_patterns, k, w, hash_seed, sizes, min_offsets, recs).  MINI_CANONICAL: the
// hash of a window is the smaller one of its own and of its reverse complement's (mini_rckey), and a record carries the key and
// the strand as well.  No include guard on purpose.
  __shared__ u8 c2c[256];
  __shared__ u64 table_hash[2 * MINI_TILE];
  __shared__ u32 table_at[2 * MINI_TILE];
  __shared__ u32 marks[4];
  const u32 lane = threadIdx.x;
#pragma unroll
  for(u32 c = 0; c < 256; c += MINI_TPB) { c2c[c + lane] = img.char2comp[c + lane]; }
  __syncthreads();
  const u32 limit = (img.sigma >= 3 ? (img.sigma - 2 < 4 ? u32(img.sigma - 2) : 4u) : 0u);     // codes 0 .. limit - 1
  const u32 need = MINI_TILE + (w - 1) + (k - 1);            // characters of a tile
  const u64 kmask = (u64(1) << k) - 1;                       // k <= 32
  const u64 below = (u64(1) << lane) - 1;
  if(!PLACE && blockIdx.x == 0 && lane == 0) { sizes[n_patterns] = 0; }

  for(u64 q = blockIdx.x; q < n_patterns; q += gridDim.x)
  {
    const u64 begin = offsets[q], len = offsets[q + 1] - begin;
    const u64 W = (len >= k ? len - k + 1 : 0);
    const u64 out = (PLACE ? min_offsets[q] : 0);
    u64 count = 0, carry = 0;
    bool prev_valid = false;                                 // window base - 1
    for(u64 base = 0; base < W; base += MINI_TILE)
    {
      // 1. the tile's characters as five code words and three words of bad bits
      u64 bad[3], word[5];
#pragma unroll
      for(u32 r = 0; r < 3; r++)
      {
        const u32 c = r * 64 + lane;
        const bool there = c < need && base + c < len;
        const u32 code = (there ? u32(c2c[patterns[begin + base + c]]) - 1 : ~u32(0));
        const bool good = code < limit;
        bad[r] = __ballot(!good);
        const u64 plane0 = __ballot(good && (code & 1) != 0), plane1 = __ballot(good && (code & 2) != 0);
        word[2 * r] = mini_spread(__brev(u32(plane0))) | (mini_spread(__brev(u32(plane1))) << 1);
        if(r < 2) { word[2 * r + 1] = mini_spread(__brev(u32(plane0 >> 32))) | (mini_spread(__brev(u32(plane1 >> 32))) << 1); }
      }
      // 2. hash and validity of the lane's window and of its halo window
      const bool upper = lane >= 32;
      const u32 at = lane & 31;
      const u64 key_main = mini_key(upper ? word[1] : word[0], upper ? word[2] : word[1], at, k);
      const u64 key_halo = mini_key(upper ? word[3] : word[2], upper ? word[4] : word[3], at, k);
#if MINI_CANONICAL
      const u64 fwd_main = mini_mix64(key_main ^ hash_seed), rev_main = mini_mix64(mini_rckey(key_main, k) ^ hash_seed);
      const u64 fwd_halo = mini_mix64(key_halo ^ hash_seed), rev_halo = mini_mix64(mini_rckey(key_halo, k) ^ hash_seed);
      const u64 hash_main = (rev_main < fwd_main ? rev_main : fwd_main), hash_halo = (rev_halo < fwd_halo ? rev_halo : fwd_halo);
#else
      const u64 hash_main = mini_mix64(key_main ^ hash_seed), hash_halo = mini_mix64(key_halo ^ hash_seed);
#endif
      const u64 valid_lo = __ballot((mini_bits(bad[0], bad[1], lane) & kmask) == 0);
      const u64 valid_hi = __ballot(lane + 1 < w && (mini_bits(bad[1], bad[2], lane) & kmask) == 0);
      // 3. the span that starts at the lane's window
      const u64 from_here = mini_bits(valid_lo, valid_hi, lane);
      u64 invalid = ~from_here;
      if(w < 64) { invalid |= u64(1) << w; }
      const u32 span = (invalid != 0 ? u32(__ffsll((unsigned long long)invalid)) - 1 : 64u);     // valid windows from here on, at most w
      const bool prev = (lane == 0 ? prev_valid : ((valid_lo >> (lane - 1)) & 1) != 0);
      const bool want = (from_here & 1) != 0 && (span == w || !prev);
      const u32 level = (want ? 31 - u32(__clz(int(span))) : ~u32(0));
      // 4. the sparse table, level by level in place
      __syncthreads();                                       // the previous tile has read its table and marks
      table_hash[lane] = hash_main; table_at[lane] = lane;
      table_hash[MINI_TILE + lane] = hash_halo; table_at[MINI_TILE + lane] = MINI_TILE + lane;
      if(lane < 4) { marks[lane] = 0; }
      __syncthreads();
      u32 best = 0;
      for(u32 j = 0; ; j++)
      {
        const u32 step = u32(1) << j;
        if(level == j)
        {
          const u32 right = lane + span - step;                // < 127: the span ends inside the halo
          const u64 a = table_hash[lane], b = table_hash[right];
          best = (a <= b ? table_at[lane] : table_at[right]);
        }
        if(2 * step > w) { break; }                            // no span needs a higher level
        const u32 hi = MINI_TILE + lane;
        const bool has = hi + step < 2 * MINI_TILE;            // entries without a right half are never asked for
        const u64 x0 = table_hash[lane], y0 = table_hash[lane + step];
        const u32 j0 = table_at[lane + step];
        const u64 x1 = table_hash[hi], y1 = (has ? table_hash[hi + step] : ~u64(0));
        const u32 j1 = (has ? table_at[hi + step] : 0);
        __syncthreads();
        if(y0 < x0) { table_hash[lane] = y0; table_at[lane] = j0; }
        if(has && y1 < x1) { table_hash[hi] = y1; table_at[hi] = j1; }
        __syncthreads();
      }
      // 5. the selected windows: bits 0..63 are final, the rest goes to the next tile
      if(want) { atomicOr(&marks[best >> 5], u32(1) << (best & 31)); }
      __syncthreads();
      const u64 final_bits = (u64(marks[0]) | (u64(marks[1]) << 32)) | carry;
      carry = u64(marks[2]) | (u64(marks[3]) << 32);
      prev_valid = (valid_lo >> 63) != 0;
      if(PLACE && ((final_bits >> lane) & 1) != 0)
      {
        const u64 to = out + count + u64(__popcll(final_bits & below));
        recs[to].position = base + lane; recs[to].hash = hash_main;
#if MINI_CANONICAL
        recs[to].key = key_main; recs[to].strand = (rev_main < fwd_main ? 1 : 0);
#endif
      }
      count += u64(__popcll(final_bits));
    }
    if(!PLACE && lane == 0) { sizes[q] = count; }
  }
