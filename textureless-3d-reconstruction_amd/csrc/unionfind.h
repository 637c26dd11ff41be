// unionfind.h -- the lock-free union-find on a `parent` array that the mesh components (kernels_meshcc.hip) and the planar regions
// of a cloud (kernels_planes.hip) share: ONE copy of find / unite and of the obligations every user of them keeps.  A user's own
// kernels are the "init" (parent[v] = v, a kernel of its own), the "hook" (the unites) and the "flatten" (parent -> labels) of the table.
//
// Proof obligations of the union-find (hook and flatten).  Each line is kept by every statement that touches `parent`:
//   I1  parent[v] <= v, always.                         init writes v; hook CASes a root r from r to a value < r; halving and flatten
//                                                       atomicMin an ancestor, which is <= the old value.
//   I2  parent words change only through agent-scope    atomicCAS / atomicMin on global memory (device scope); no plain store after
//       atomics.                                        init, and init is a kernel of its own.
//   I3  every value parent[v] ever held is an ancestor  hooks only add edges root -> other tree; halving replaces a parent by an
//       of v from then on, and in v's final component.  ancestor.  So a stale read (another CU's older value) names a real ancestor.
//   I4  every loop descends a strictly decreasing       find: next = parent[cur] < cur or stop.  unite: a failed CAS on root hi
//       chain or retries a CAS with the value the       returns the fresh parent[hi] < hi, and the walk goes on from there, so
//       failed CAS returned.                            max(ra, rb) falls strictly per retry.  Stale reads cost steps, never more.
//   I5  no thread waits for another thread's store.     no flags, no polls, no spin loops; a CAS that fails is answered by walking on.
//   I6  the smaller root always wins.                   the smallest index m of a component has parent[m] = m for ever (I1 + I3), so
//                                                       when every triangle's unites are done the one root left is m.
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

__device__ __forceinline__ unsigned cc_load(const unsigned *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of v as far as this thread can see, halving the path on the way (I1-I4)
__device__ __forceinline__ unsigned cc_find(unsigned *parent, unsigned v) {
    unsigned cur = v, p = cc_load(parent + cur);
    while (p < cur) {
        const unsigned gp = cc_load(parent + p);
        if (gp < p) atomicMin(parent + cur, gp);
        cur = p;
        p = gp;
    }
    return cur;
}

__device__ __forceinline__ void cc_unite(unsigned *parent, unsigned a, unsigned b) {
    unsigned ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        const unsigned hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const unsigned old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;                   // hi was a root and now hangs under lo
        ra = cc_find(parent, old);               // old < hi: somebody hooked hi first; go on from its new parent
        rb = lo;
    }
}

}  // namespace tl3d
