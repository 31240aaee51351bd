// How the persistent waves of a K1 launch share its work items (ks_rank.hpp).
//
// Every wave of a launch is resident from the start (the grid is num_cus x blocks per CU), and the SIMD's issue arbiter
// favours its oldest wave: with one equal, strided share per wave the oldest wave of a SIMD ends long before the youngest,
// and the launch finishes with one to three waves per SIMD instead of four (profiles/k1_wave_balance.txt).  So only a part
// of a wave's share is fixed; the rest of the items is handed out in small chunks to whichever wave runs out first:
//   * rounds  — wave w takes items w + k * waves, k < rounds, exactly as the strided walk does (no atomic);
//   * chunks  — items [first, items), first = rounds * waves, are cut into chunks of `chunk` consecutive items; chunk c holds
//               items first + c * chunk .. + chunk - 1 (those below `items`).  Chunk w belongs to wave w (no atomic either);
//               chunk waves + t goes to the wave that draws ticket t from the launch's counter (one returning atomic increment,
//               counter = 0 when the launch starts).
// A wave is done when it holds an item >= items: tickets only grow, so every later chunk of it would lie beyond the end too.
// The launcher, the kernel and the host-side check (nmod_item_claim_plan) all take the arithmetic from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmod {

// The fixed part is 3/8 of the equal share: the oldest wave of a SIMD ends its equal share at ~0.4 of the launch (measured:
// profiles/k1_wave_balance.txt), and a fixed part beyond that would leave it idle again.  A chunk is at most four items (one
// 200 v 200 item is ~12 us of a wave: the ragged end of a launch stays near 1 % of a 281-item share) and one item for short
// shares; one atomic per chunk and wave, issued one chunk ahead of its use.
constexpr int kClaimFixedNum = 3, kClaimFixedDen = 8;
constexpr int kClaimChunkMax = 4;
constexpr int kClaimItemsPerChunkStep = 32;      // chunk = share / 32, within 1 .. kClaimChunkMax

template <typename I>
struct ItemClaimPlanT {
  I rounds;            // strided rounds of every wave
  I first;             // first item that is handed out by chunk
  int32_t chunk;       // items per chunk
  int32_t dynamic;     // 1: chunks beyond the waves' own exist (tickets are drawn), 0: the launch needs no atomic
};
using ItemClaimPlan = ItemClaimPlanT<int64_t>;

// strided_only (NMOD_FLAG_K1_STATIC_ITEMS): the strided walk for every item, nothing is claimed.  I: int64_t on the host,
// uint32_t in the kernels (a launch has fewer than 2^31 items; the divisions are 32-bit there) — the same arithmetic.
template <typename I>
__host__ __device__ inline ItemClaimPlanT<I> item_claim_plan(I items, I waves, bool strided_only) {
  ItemClaimPlanT<I> p;
  if (waves < 1) waves = 1;
  if (strided_only) {
    p.rounds = (items + waves - 1) / waves; p.first = items; p.chunk = 1; p.dynamic = 0;
    return p;
  }
  const I share = items / waves;
  p.rounds = share / kClaimFixedDen * kClaimFixedNum + share % kClaimFixedDen * kClaimFixedNum / kClaimFixedDen;   // share * 3 / 8
  p.first = p.rounds * waves;
  const I c = share / kClaimItemsPerChunkStep;
  p.chunk = (int32_t)(c < 1 ? 1 : (c > kClaimChunkMax ? kClaimChunkMax : c));
  p.dynamic = (items - p.first > waves * (I)p.chunk) ? 1 : 0;
  return p;
}
// first item of chunk c (chunk w: wave w's own; chunk waves + t: ticket t)
template <typename I>
__host__ __device__ inline I item_claim_chunk_first(const ItemClaimPlanT<I>& p, I c) { return p.first + c * (I)p.chunk; }

// The walk of one wave; every member but `ticket` is wave-uniform.  begin() / next() may issue the claim of the chunk AFTER the
// one they enter — one lane's returning atomic, so callers place them where no vector load is outstanding whose wait the
// compiler counts — and collect() takes its result once a vmcnt(0) has passed (the same item: the claim is always a chunk ahead).
// Items are 32-bit here: a launch has fewer than 2^31 of them, and a claim past the end overshoots by less than
// 3 * waves * chunk + chunk (a wave stops drawing at its first chunk beyond the end, one more is in flight by then).
struct ItemWalk {
  uint32_t step, left, pend, base, chunk;          // base: first item of chunk `waves`, the one ticket 0 stands for
  bool dynamic, outstanding;
  unsigned* counter;
  unsigned ticket;

  __device__ __forceinline__ uint32_t enter_pending(int lane) {
    const uint32_t it = pend;
    step = 1u; left = chunk - 1u;
    pend = 0xffffffffu;                            // (no further chunk unless a ticket says so)
    if (dynamic) {
      // (atomicInc with the largest bound is "add one"; the compiler turns a wave-uniform atomicAdd into a reduction whose
      // result it broadcasts at once, behind a vmcnt(0) of its own — the wait this claim is issued early to avoid)
      if (lane == 0) ticket = atomicInc(counter, 0xffffffffu);
      outstanding = true;
    }
    return it;
  }
  __device__ __forceinline__ uint32_t begin(const ItemClaimPlanT<uint32_t>& p, uint32_t wave, uint32_t waves, unsigned* ctr, int lane) {
    chunk = (uint32_t)p.chunk; dynamic = p.dynamic != 0; outstanding = false; counter = ctr; ticket = 0u;
    base = item_claim_chunk_first(p, waves);
    pend = item_claim_chunk_first(p, wave);
    if (p.rounds > 0u) { step = waves; left = p.rounds - 1u; return wave; }
    return enter_pending(lane);
  }
  __device__ __forceinline__ uint32_t next(uint32_t it, int lane) {
    if (left > 0u) { --left; return it + step; }
    return enter_pending(lane);
  }
  __device__ __forceinline__ void collect() {
    if (outstanding) {
      pend = base + (uint32_t)__builtin_amdgcn_readfirstlane((int)ticket) * chunk;
      outstanding = false;
    }
  }
};

}  // namespace nmod
