// k_sample_body.inc -- the body of k_sample, of k_sample_norep and of k_sample_weighted (cslicer_hip.hip includes it once
// in each, after a `constexpr bool NOREP`, a `constexpr bool WEIGHTED` and -- where the kernel has no such parameter -- a
// null `constexpr const uint32_t* cum`).  Text, not a function: k_sample stays a plain kernel of that name -- profiles and
// bench.py's live counters look it up as `k_sample` -- and compiles to the code it had before the other kernels existed; an
// inlined template body did not (the compiler ordered three scalar instructions of the prologue differently).
  extern __shared__ __attribute__((aligned(16))) uint32_t s_bh[];  // [nb] bucket histogram
  uint32_t bx, s;
  if (!xcd_block(a, bx, s)) return;
  const uint32_t F = a.fsize[s * (CSL_MAX_LAYERS + 1) + a.layer];
  if (bx * a.tpb * TN >= F) return;
  __shared__ uint32_t s_v[TN];
  __shared__ unsigned long long s_ri[TN];
  __shared__ uint32_t s_rng[TN];
  __shared__ uint32_t s_hb[TN];
  __shared__ uint8_t s_to[TN];  // owner part of the tile's nodes
  __shared__ uint32_t s_wn[NW];
  __shared__ uint32_t s_cnt[5 * CSL_MAX_PARTS];
  __shared__ uint32_t s_ec[TN * CSL_MAX_PARTS];                                 // graph: edges per (node, source part)
  __shared__ uint32_t s_gcnt[CSL_MAX_PARTS + CSL_MAX_PARTS * CSL_MAX_PARTS];    // graph: ECNT[g], PAIR[g][p]
  const uint32_t n = threadIdx.x;
  const uint32_t f = a.fanout, W = a.W;
  const uint32_t P = a.P;
  const uint32_t nb = a.nbk[s];
  for (uint32_t b = n; b < nb; b += TN) s_bh[b] = 0;
  const unsigned long long rbase = a.rngbase[s];
  for (uint32_t sub = 0; sub < a.tpb; sub++) {
    const uint32_t tile = bx * a.tpb + sub;
    if (tile * TN >= F) break;
    const uint32_t i = tile * TN + n;
    // phase 1: stage the tile's nodes, rank the rng consumers
    uint32_t v = 0, need = 0;
    unsigned long long ri = 0;
    if (i < F) {
      v = a.fr_in[s * a.fr_in_stride + i];
      ri = a.ninfo[s * a.fcap + i];
      need = (uint32_t)(ri & DEG_MASK) >= f;
    }
    const unsigned long long bm = __ballot(need);
    __syncthreads();  // previous sub-tile done with the LDS arrays
    if (lane_id() == 0) s_wn[n >> 6] = __popcll(bm);
    if (n < 5 * CSL_MAX_PARTS) s_cnt[n] = 0;
    s_v[n] = v;
    s_ri[n] = ri;
    s_hb[n] = 0;
    s_to[n] = i < F ? (uint8_t)owner(a, v) : 0;
    if (a.graph) {
      for (uint32_t k = n; k < TN * P; k += TN) s_ec[k] = 0;
      if (n < CSL_MAX_PARTS + CSL_MAX_PARTS * CSL_MAX_PARTS) s_gcnt[n] = 0;
    }
    __syncthreads();
    {
      uint32_t r = __popcll(bm & lt_mask());
      for (uint32_t w = 0; w < (n >> 6); w++) r += s_wn[w];
      const uint32_t tb = a.tcnt[((size_t)s * a.nk + K_NEED) * a.tmax + tile];
      s_rng[n] = need ? (tb + r) * f : UNSET;
    }
    __syncthreads();
    // phase 2: candidates, coalesced over c.  Each thread keeps SU candidates in
    // flight: all their rng words are requested, then all their neighbour ids,
    // before any is consumed (the loads are dependent pairs of HBM round trips).
    const uint32_t nodes_here = (F - tile * TN) < (uint32_t)TN ? (F - tile * TN) : (uint32_t)TN;
    const uint32_t ncand = nodes_here * W;
    const size_t cbase = (size_t)s * a.ccap + (size_t)tile * TN * W;
    constexpr int SU = CSL_SU;
    const uint32_t dq = TN / W, dr = TN - dq * W;  // k += TN  =>  node += dq, slot += dr (+carry)
    uint32_t nn = n / W, slot = n - nn * W;
    for (uint32_t k0 = n; k0 < ncand; k0 += TN * SU) {
      uint32_t nnu[SU], slu[SU], vvu[SU], degu[SU], val[SU], rnd[SU];
      unsigned long long addr[SU], rpos[SU];
      bool live[SU], gat[SU], rq[SU];
#pragma unroll
      for (int u = 0; u < SU; u++) {
        live[u] = k0 + u * TN < ncand;
        nnu[u] = nn;
        slu[u] = slot;
        nn += dq;
        slot += dr;
        if (slot >= W) {
          slot -= W;
          nn++;
        }
        val[u] = UNSET;
        gat[u] = false;
        rq[u] = false;
        addr[u] = 0;
        rpos[u] = 0;
        vvu[u] = 0;
        degu[u] = 1;
        rnd[u] = 0;
        if (live[u]) {
          vvu[u] = s_v[nnu[u]];
          if (slu[u] == 0) {
            val[u] = vvu[u];
          } else {
            const unsigned long long r2 = s_ri[nnu[u]];
            const uint32_t deg = (uint32_t)(r2 & DEG_MASK);
            const uint32_t j = slu[u] - 1;
            degu[u] = deg;
            addr[u] = r2 >> DEG_BITS;
            if (deg < f) {
              gat[u] = j < deg;
              addr[u] += j;
            } else {
              gat[u] = true;
              rq[u] = true;
              rpos[u] = rbase + s_rng[nnu[u]] + j;
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < SU; u++) {
        if (rq[u]) {
          if (rpos[u] >= a.gen_lo && rpos[u] < a.gen_hi) {
            rnd[u] = a.ring[rpos[u] & a.ring_mask];
          } else {
            atomicOr(&a.meta[s].error, (uint32_t)CSL_ERR_RNG_WINDOW);
          }
        }
      }
      // csl_set_edge_cdf: word -> edge position through the row's cumulative weights.  x = (r * T) >> 32 lies in [0, T);
      // the pick is the smallest i in [0, deg) with cum[off + i] > x (an upper bound: a zero-weight edge is never picked).
      // The SU row totals are requested together, then the SU searches run in lock-step, one probe of each per trip, the
      // probes of a trip in flight together.  lo <= hi < deg at every step and hi - lo halves: whatever the table holds,
      // every probe and the gather stay inside the row and a search ends within 24 trips (deg < 2^24).
      [[maybe_unused]] uint32_t wlo[SU];
      if constexpr (WEIGHTED) {
        uint32_t tot[SU], whi[SU], wx[SU], wc[SU];
#pragma unroll
        for (int u = 0; u < SU; u++) tot[u] = rq[u] ? cum[addr[u] + (degu[u] - 1u)] : 0u;
        bool more = false;
#pragma unroll
        for (int u = 0; u < SU; u++) {
          wx[u] = __umulhi(rnd[u], tot[u]);
          wlo[u] = (rq[u] && !tot[u]) ? rnd[u] % degu[u] : 0u;  // T == 0: the parent's draw (deg >= fanout >= 1)
          whi[u] = tot[u] ? degu[u] - 1u : wlo[u];
          more |= wlo[u] < whi[u];
        }
        while (more) {
#pragma unroll
          for (int u = 0; u < SU; u++) wc[u] = wlo[u] < whi[u] ? cum[addr[u] + ((wlo[u] + whi[u]) >> 1)] : 0u;
          more = false;
#pragma unroll
          for (int u = 0; u < SU; u++) {
            if (wlo[u] < whi[u]) {
              const uint32_t mid = (wlo[u] + whi[u]) >> 1;
              if (wc[u] > wx[u]) whi[u] = mid;
              else wlo[u] = mid + 1u;
            }
            more |= wlo[u] < whi[u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < SU; u++) {
        // (non-temporal loads here were measured 5 % slower: picks of one row share lines)
        if constexpr (WEIGHTED) {
          if (gat[u]) val[u] = a.indices[addr[u] + wlo[u]];
        } else if constexpr (NOREP) {
          if (gat[u])
            val[u] = a.indices[addr[u] + (rq[u] ? floyd_pick(a, s, rpos[u] - (slu[u] - 1u), slu[u] - 1u, degu[u] - f, rnd[u]) : 0u)];
        } else {
          if (gat[u]) val[u] = a.indices[addr[u] + (rq[u] ? rnd[u] % degu[u] : 0u)];
        }
      }
#pragma unroll
      for (int u = 0; u < SU; u++) {
        if (live[u]) {
          // The flag byte every candidate gets here is what k_bucket would find in the common case: a self entry
          // new to the frontier, an edge candidate the first occurrence of its node (in the frontier and among its
          // slice's in-nodes) and not a frontier node itself.  k_bucket then only stores the exceptions (a fifth of
          // the entries) instead of one scattered byte per first occurrence (most entries): its evaluate phase was
          // bound by exactly those stores.  bit0 new-frontier, bit1 first-in-node, bits 2-4 owner part.
          uint32_t fl = 0;
          if (slu[u] == 0) {
            atomicAdd(&s_bh[bucket_of(val[u], nb)], 1u);
            fl = (a.graph ? 3u : 1u) | ((uint32_t)s_to[nnu[u]] << 2);
          } else if (val[u] != UNSET) {
            if (val[u] == vvu[u]) {
              // a sampled self loop only re-adds the self edge (slicer.cpp:33-35,
              // bipartite.h:34): it is neither an edge nor new to the frontier
              if (a.candk) a.candk[cbase + k0 + u * TN] = val[u];  // (the raw stream keeps it)
              val[u] = UNSET;
            } else {
              const uint32_t og = owner(a, val[u]);
              atomicOr(&s_hb[nnu[u]], 1u << og);
              if (a.graph) atomicAdd(&s_ec[nnu[u] * P + og], 1u);
              atomicAdd(&s_bh[bucket_of(val[u], nb)], 1u);
              fl = 3u | (og << 2);
              // graph mode: an edge's source position is its own position unless k_bucket finds an earlier one
              if (a.graph) a.srcpos[cbase + k0 + u * TN] = tile * TN * W + k0 + u * TN;
            }
          }
          a.cand[cbase + k0 + u * TN] = val[u];
          a.cflag[cbase + k0 + u * TN] = (uint8_t)fl;  // k_bucket corrects the exceptions
          if (a.candk && (val[u] != UNSET || slu[u] == 0 || !gat[u])) a.candk[cbase + k0 + u * TN] = val[u];
        }
      }
    }
    __syncthreads();
    // phase 3: per-node list memberships (bipartite.h:33-66 push conditions)
    uint32_t hb = 0, to = 0;
    const bool act = i < F;
    if (act) {
      hb = s_hb[n];
      to = s_to[n];
      if (!a.graph) a.firstpos[s * a.fcap + i] = UNSET;  // k_bucket stores it for nodes that are sampled as a neighbour too
      // graph mode: a node is always an out node of its own slice
      if (a.graph) hb |= 1u << to;
      a.hasedge[s * a.fcap + i] = hb;
    }
    if (a.graph) {
      for (uint32_t g = 0; g < P; g++) {
        const uint32_t ec = act ? s_ec[n * P + g] : 0u;  // <= fanout <= 255
        if (act) a.ecnt[(s * a.fcap + i) * P + g] = (uint8_t)ec;
        uint32_t x = ec;
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
        if (lane_id() == 0 && x) atomicAdd(&s_gcnt[g], x);
        const bool hasg = act && ((hb >> g) & 1u) && to != g;
        for (uint32_t p = 0; p < P; p++) {
          const uint32_t c_pair = __popcll(__ballot(hasg && to == p));
          if (lane_id() == 0 && c_pair) atomicAdd(&s_gcnt[CSL_MAX_PARTS + g * CSL_MAX_PARTS + p], c_pair);
        }
      }
    }
    for (uint32_t g = 0; g < P; g++) {
      const bool own = act && to == g;
      const bool has = act && ((hb >> g) & 1u);
      const uint32_t c_out = __popcll(__ballot(has));
      const uint32_t c_owned = __popcll(__ballot(own && has));
      const uint32_t c_self = __popcll(__ballot(own));
      const uint32_t c_to = __popcll(__ballot(own && (hb & ~(1u << g)) != 0));
      const uint32_t c_from = __popcll(__ballot(has && !own));
      if (lane_id() == 0) {
        if (c_out) atomicAdd(&s_cnt[0 * CSL_MAX_PARTS + g], c_out);
        if (c_owned) atomicAdd(&s_cnt[1 * CSL_MAX_PARTS + g], c_owned);
        if (c_self) atomicAdd(&s_cnt[2 * CSL_MAX_PARTS + g], c_self);
        if (c_to) atomicAdd(&s_cnt[3 * CSL_MAX_PARTS + g], c_to);
        if (c_from) atomicAdd(&s_cnt[4 * CSL_MAX_PARTS + g], c_from);
      }
    }
    __syncthreads();
    if (n < 5 * P) {
      const uint32_t kind5 = n / P, g = n - kind5 * P;
      a.tcnt[((size_t)s * a.nk + (K_OUT(P, 0) + kind5 * P + g)) * a.tmax + tile] = s_cnt[kind5 * CSL_MAX_PARTS + g];
    }
    if (a.graph) {
      if (n < P) a.tcnt[((size_t)s * a.nk + K_ECNT(P, n)) * a.tmax + tile] = s_gcnt[n];
      if (n < P * P) {
        const uint32_t g = n / P, p = n - g * P;
        a.tcnt[((size_t)s * a.nk + K_PAIR(P, g, p)) * a.tmax + tile] = s_gcnt[CSL_MAX_PARTS + g * CSL_MAX_PARTS + p];
      }
    }
  }
  __syncthreads();
  uint32_t* gcnt = a.bcnt + (size_t)s * (a.nbmax + 1);
  for (uint32_t b = n; b < nb; b += TN) {
    const uint32_t c = s_bh[b];
    if (c) atomicAdd(&gcnt[b], c);
  }
