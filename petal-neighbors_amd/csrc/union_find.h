// union_find.h -- the lock-free union-find over parent[] shared by components.hip (DBSCAN) and mst.hip (Boruvka).
//
// Every hook links the larger of two roots under the smaller, so parent[x] <= x always, the forest has no cycle, and a
// finished component's root is its lowest member whatever order the unions ran in.
//
// Visibility.  The L2s of the eight XCDs are not coherent for plain loads: a workgroup that re-read parent[] with plain
// loads could spin on a stale "I am a root" and never see its CAS succeed.  Inside a kernel that unites or flattens, EVERY
// read of parent[] is a relaxed agent-scope atomic load (sc1: served by the coherent level), every write an agent-scope
// atomic store or CAS.  Arrays written by earlier launches only are read plainly.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pn {

__device__ __forceinline__ uint32_t uf_load(const uint32_t *parent, uint32_t i) {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// path halving: x's parent is replaced by its grandparent on the way up.  Only a non-root is written (p != x), a non-root
// never becomes a root again and is never the target of a hook, and the value stored is an ancestor of x: racing stores
// leave some ancestor in place, never a wrong tree.
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    uint32_t p = uf_load(parent, x);
    while (p != x) {
        const uint32_t g = uf_load(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}
// unites the sets of a and b; ra = a root a was last seen under (a hint: the common case, equal roots, costs one find).
// A failed CAS means parent[hi] has been lowered by another hook, so the next round starts from a strictly smaller root
// of that side: at most hi + 1 rounds.  Returns the root both are under now.
__device__ __forceinline__ uint32_t uf_unite(uint32_t *parent, uint32_t ra, uint32_t b) {
    uint32_t rb = uf_find(parent, b);
    ra = uf_find(parent, ra);
    while (ra != rb) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        uint32_t expect = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        ra = uf_find(parent, hi);
        rb = uf_find(parent, lo);
    }
    return ra;
}

}  // namespace pn
