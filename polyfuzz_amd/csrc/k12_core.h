// K12's union-find: the connected components of "similarity >= t", kept as a forest in one int32 array while the hits are found
// (k12_components.hip), in the style of ECL-CC (Jaiganesh & Burtscher, HPDC 2018): lock-free hooking of the larger root under the
// smaller by compare-and-swap, path halving in the finds.  Plain C++ over a small trait of atomic operations, so that the HIP
// kernels (agent-scope __hip_atomic_*) and a host program with racing threads (tests/k12_core_host.cpp, __atomic_*) run the SAME
// logic.
//
// parent[x] starts as x.  Ops is a type with three static functions on one int32 word, all of them atomic and relaxed:
//   int32_t load(const int32_t *p);   void store(int32_t *p, int32_t v);   int32_t cas(int32_t *p, int32_t expected, int32_t desired)
// (cas returns the value it found: `expected` iff it stored).
//
// Invariants, at every moment and under every interleaving of the atomics:
//   (1) parent[x] <= x, and parent[x] == x exactly while x is a root.  Only two kinds of store exist: the hook, a CAS that replaces
//       the x of a root by a smaller position, and the halving store, which writes a value read from parent[p] != p of some p < x
//       into a NON-root x.  A non-root never becomes a root again (no store writes x into parent[x]), so a halving store never
//       lands on a root and a hook never lands on a non-root: the CAS expects x itself.
//   (2) every value ever stored in parent[x] is a member of x's tree -- an ancestor of x when it was read -- and trees only merge
//       (a hook joins two), they never split.  So a value read a while ago, however stale, still names a member of x's tree
//       that is smaller than x.
//   (3) by (1) every chain of parents falls strictly until it meets a root: there is no cycle and uf_find ends.
// What this buys: correctness does not rest on freshness.  A find that reads an old parent walks a longer way to a position that
// WAS a root; if it no longer is one, the hook's CAS -- decided at the memory, where the atomics of all workgroups meet -- fails,
// and the loop goes round from the two positions it holds, which are still members of the two trees.  A failed CAS means another
// hook succeeded on that word, so the number of roots fell: the system makes progress whenever any lane retries.  No lane waits
// for another, there is no flag, lock or barrier between workgroups, and no fence: a parent is never used as evidence that some
// OTHER word has been written.
// When every uf_unite has returned, u and v of each call are in one tree (they were when it returned, and trees never split), each
// tree is inside one component (a hook only ever joins the trees of a hit's two ends), and by (1) a tree's root is its smallest
// member.  Hence the root of a component is its smallest position, whatever the order of the atomics: the labels are
// deterministic.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define K12_HD __host__ __device__ inline
#else
#define K12_HD inline
#endif

namespace pfz {

// the root x's tree had when the walk got there; halves the path behind it
template <class Ops> K12_HD int32_t uf_find(int32_t *parent, int32_t x)
{
    int32_t p = Ops::load(parent + x);
    while (p != x) {
        const int32_t g = Ops::load(parent + p);
        if (g == p) return p;
        Ops::store(parent + x, g);      // x is not a root; g < p < x is a member of its tree
        x = g;
        p = Ops::load(parent + x);
    }
    return x;
}

// u and v end in one tree.  Returns the number of CAS attempts that failed (a work count; 0 almost always).
template <class Ops> K12_HD int uf_unite(int32_t *parent, int32_t u, int32_t v)
{
    int failed = 0;
    for (;;) {
        u = uf_find<Ops>(parent, u);
        v = uf_find<Ops>(parent, v);
        if (u == v) return failed;
        const int32_t lo = u < v ? u : v, hi = u < v ? v : u;
        if (Ops::cas(parent + hi, hi, lo) == hi) return failed;
        ++failed;                       // hi was hooked by another lane meanwhile: go on from the two positions in hand
        u = lo;
        v = hi;
    }
}

// the same walk without a store, for a forest that no longer changes (k12_flatten, behind the kernel boundary)
template <class Ops> K12_HD int32_t uf_root(const int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = Ops::load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

#if defined(__HIPCC__)
// parent as the kernels that hook touch it (K12's walk, K14's tile epilogue): relaxed, agent scope, nothing else
struct UfDeviceOps {
    __device__ static int32_t load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static void store(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static int32_t cas(int32_t *p, int32_t expected, int32_t desired)
    {
        __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
};

// the finished forest, behind the kernel boundary: plain loads
struct UfPlainOps {
    __device__ static int32_t load(const int32_t *p) { return *p; }
};
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
// the host's atomics: what tests/k12_core_host.cpp races its threads through
struct UfHostOps {
    static int32_t load(const int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static void store(int32_t *p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
    static int32_t cas(int32_t *p, int32_t expected, int32_t desired)
    {
        __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expected;
    }
};
#endif

}  // namespace pfz
