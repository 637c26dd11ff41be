// keytab.h -- the device half of the 64-bit key table that vertex clustering, the smoothing's edge list, the mesh weld and the
// cloud's voxel subsample (kernels_cloudglobal.hip) share ("The key table").  An open-addressing table of
// `mask + 1` words (a power of two), filled with 0xFF by the host (kt_reserve, api_host.h) before the call's first insert, probed linearly.  A table holds keys and nothing else: what
// a user keeps beside a key (a leader, an output index) lives in an array of its own, indexed by the slot these functions return,
// and its obligations (H2 of the user's file) stay with the user.
//
// Proof obligations of the table.  They are what keeps a broken table from hanging the device, and they are kept HERE, by the
// statements named on the right, for every user at once:
//   H1  a key word changes once, EMPTY -> key, by the   the only store to keys[] after the fill is the atomicCAS(EMPTY, key) of
//       CAS that writes it.                             kt_claim; a CAS that fails returns the key somebody else wrote.  So a key
//                                                       a thread has seen in a slot stays there, and every probe sequence a thread
//                                                       has walked stays valid.
//   H3  load <= 0.5, so probing ends.                   the host sizes every table with kt_slots(max_keys): a power of two
//                                                       >= 2 * max_keys, and a user inserts at most max_keys distinct keys (it says
//                                                       in its header what bounds them), so an EMPTY slot or the own key lies ahead.
//                                                       Both loops are ALSO bounded by the capacity: a table that is full, or was
//                                                       never filled, costs one walk over it and gives KT_NONE.
//   H5  no thread waits for another thread's store.     no flags, no polls, no spin loops: a failed CAS is answered by looking at the
//                                                       value it returned and probing on.
// A key must differ from KT_EMPTY; every user's keys have bit 63 clear.
#pragma once
#include "compact.h"

namespace tl3d {

typedef unsigned long long u64;

constexpr u64 KT_EMPTY = ~0ull;                          // the fill: no key equals it
constexpr u64 KT_NONE = ~0ull;                           // no slot (a slot is <= mask < 2^63)

// the finaliser of MurmurHash3
__device__ __forceinline__ u64 kt_mix(u64 x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// The slot that holds `key`, claiming the first EMPTY slot of its probe sequence when the key is not there yet; won: this
// thread's CAS wrote the key (exactly one thread per key wins).  KT_NONE only when the bounded loop runs out (H3: never).
__device__ __forceinline__ u64 kt_claim(u64 *keys, u64 mask, u64 key, bool &won) {
    won = false;
    u64 h = kt_mix(key) & mask;
    for (u64 probe = 0; probe <= mask; ++probe) {                           // (H3: ends long before the bound)
        u64 cur = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == KT_EMPTY) {
            cur = atomicCAS(keys + h, KT_EMPTY, key);                       // H1
            if (cur == KT_EMPTY) {
                won = true;
                cur = key;
            }
        }
        if (cur == key) return h;
        h = (h + 1) & mask;                                                 // H5: somebody else's key; on to the next slot
    }
    return KT_NONE;
}

// The slot that holds `key` in a table no launch writes any more; KT_NONE when the probe sequence reaches EMPTY first
__device__ __forceinline__ u64 kt_find(const u64 *__restrict__ keys, u64 mask, u64 key) {
    u64 h = kt_mix(key) & mask, found = KT_NONE;
    for (u64 probe = 0; probe <= mask; ++probe) {                           // (H3)
        const u64 cur = keys[h];
        if (cur == key) found = h;
        if (cur == key || cur == KT_EMPTY) break;
        h = (h + 1) & mask;
    }
    return found;
}

// *word += the lanes of the wave that `flag`: one add, by the first of them.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_count(bool flag, u64 *word) {
    const u64 m = __ballot(flag);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(word, (u64)__popcll(m));
}

}  // namespace tl3d
