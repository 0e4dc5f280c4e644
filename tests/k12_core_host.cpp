// polyfuzz_amd/csrc/k12_core.h -- K12's lock-free union-find (uf_find with path halving, uf_unite hooking the larger root under
// the smaller by compare-and-swap) -- compiled for the host over the host trait (UfHostOps: relaxed __atomic_*) and held to the
// definition: when every uf_unite has returned, the root of every node is the SMALLEST node of its connected component, and at
// every moment parent[x] <= x.
//   k12_host_exhaustive: every graph on 1 .. max_nodes nodes (every subset of the n (n - 1) / 2 edges), its edges united in
//     several orders -- ascending, descending, each edge's ends swapped, and seeded shuffles --, single-threaded; the invariant
//     is checked after EVERY unite.
//   k12_host_race: a seeded random graph whose edges `threads` host threads unite at the same time (each its own interleaved
//     share; every thread checks the invariant on the words it has just touched), then the whole array.  hot > 0: every second
//     edge has one end among the first `hot` nodes, so that the hooks of all threads meet on a few roots.
// report: [0] (graph, order) combinations / edges done, [1] parent[x] > x seen, [2] nodes whose root is not the smallest node of
// their component, [3] compare-and-swap attempts that failed (the race is real where this is > 0), [4] components.
// tests/test_components_cpu.py asserts [1] == [2] == 0.
// With -DK12_HOST_MAIN: a stand-alone program (for a sanitizer run) that runs both and exits 1 on a violation.
#include <stddef.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>

#include "../polyfuzz_amd/csrc/k12_core.h"

using namespace pfz;

typedef std::pair<int32_t, int32_t> Edge;

// the definition: the smallest node of every node's component, by relabelling until nothing moves
static std::vector<int32_t> smallest_of_component(int n, const std::vector<Edge> &edges)
{
    std::vector<int32_t> lab((size_t)n);
    for (int i = 0; i < n; ++i) lab[(size_t)i] = i;
    for (bool moved = true; moved;) {
        moved = false;
        for (const Edge &e : edges) {
            const int32_t m = std::min(lab[(size_t)e.first], lab[(size_t)e.second]);
            if (lab[(size_t)e.first] != m || lab[(size_t)e.second] != m) {
                lab[(size_t)e.first] = lab[(size_t)e.second] = m;
                moved = true;
            }
        }
    }
    return lab;
}

static uint64_t next_random(uint64_t &s)      // splitmix64
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int64_t count_above(const std::vector<int32_t> &parent)
{
    int64_t bad = 0;
    for (size_t x = 0; x < parent.size(); ++x) bad += UfHostOps::load(&parent[x]) > (int32_t)x;
    return bad;
}

extern "C" {

int k12_host_exhaustive(int max_nodes, int n_shuffles, int64_t *report)
{
    for (int k = 0; k < 5; ++k) report[k] = 0;
    uint64_t seed = 12;
    for (int n = 1; n <= max_nodes; ++n) {
        std::vector<Edge> all;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) all.push_back(Edge(i, j));
        for (uint32_t subset = 0; subset < (1u << all.size()); ++subset) {
            std::vector<Edge> edges;
            for (size_t e = 0; e < all.size(); ++e)
                if (subset >> e & 1) edges.push_back(all[e]);
            const std::vector<int32_t> want = smallest_of_component(n, edges);
            for (int order = 0; order < 3 + n_shuffles; ++order) {
                std::vector<Edge> es = edges;
                if (order == 1) std::reverse(es.begin(), es.end());
                if (order == 2)
                    for (Edge &e : es) std::swap(e.first, e.second);
                if (order >= 3)
                    for (size_t i = es.size(); i > 1; --i) {
                        std::swap(es[i - 1], es[(size_t)(next_random(seed) % i)]);
                        if (next_random(seed) & 1) std::swap(es[i - 1].first, es[i - 1].second);
                    }
                std::vector<int32_t> parent((size_t)n);
                for (int i = 0; i < n; ++i) parent[(size_t)i] = i;
                for (const Edge &e : es) {
                    report[3] += uf_unite<UfHostOps>(parent.data(), e.first, e.second);
                    report[1] += count_above(parent);
                }
                for (int i = 0; i < n; ++i) {
                    report[2] += uf_find<UfHostOps>(parent.data(), i) != want[(size_t)i];
                    report[2] += uf_root<UfHostOps>(parent.data(), i) != want[(size_t)i];
                }
                report[1] += count_above(parent);
                ++report[0];
            }
        }
    }
    return 0;
}

// out_label: NULL or int32[n], the roots as the racing threads left them
int k12_host_race(int n, int64_t n_edges, int threads, int hot, uint64_t seed, int64_t *report, int32_t *out_label)
{
    for (int k = 0; k < 5; ++k) report[k] = 0;
    std::vector<Edge> edges((size_t)n_edges);
    int64_t at = 0;
    for (Edge &e : edges) {
        e.first = (int32_t)(next_random(seed) % (uint64_t)(hot > 0 && (at++ & 1) ? hot : n));
        e.second = (int32_t)(next_random(seed) % (uint64_t)n);      // (a loop u == u is a legal call: nothing happens)
    }
    std::vector<int32_t> parent((size_t)n);
    for (int i = 0; i < n; ++i) parent[(size_t)i] = i;
    std::atomic<int64_t> above(0), failed(0);
    std::atomic<int> ready(0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.push_back(std::thread([&, t]() {
            ready.fetch_add(1);
            while (ready.load() < threads) {}                       // start together (the test's own rendezvous, not the union-find's)
            int64_t my_above = 0, my_failed = 0;
            for (size_t e = (size_t)t; e < edges.size(); e += (size_t)threads) {
                my_failed += uf_unite<UfHostOps>(parent.data(), edges[e].first, edges[e].second);
                my_above += UfHostOps::load(&parent[(size_t)edges[e].first]) > edges[e].first;
                my_above += UfHostOps::load(&parent[(size_t)edges[e].second]) > edges[e].second;
            }
            above += my_above;
            failed += my_failed;
        }));
    for (std::thread &th : pool) th.join();
    const std::vector<int32_t> want = smallest_of_component(n, edges);
    report[0] = n_edges;
    report[1] = above.load() + count_above(parent);
    report[3] = failed.load();
    for (int i = 0; i < n; ++i) {
        const int32_t r = uf_root<UfHostOps>(parent.data(), i);
        report[2] += r != want[(size_t)i];
        report[4] += r == i;
        if (out_label) out_label[i] = r;
    }
    return 0;
}

}  // extern "C"

#ifdef K12_HOST_MAIN
#include <stdio.h>
int main()
{
    int64_t r[5];
    k12_host_exhaustive(5, 4, r);
    printf("exhaustive: %lld orders, above %lld, wrong %lld\n", (long long)r[0], (long long)r[1], (long long)r[2]);
    int bad = r[1] != 0 || r[2] != 0;
    for (int64_t m : {500, 2000, 20000, 200000}) {
        k12_host_race(2000, m, 8, m > 20000 ? 4 : 0, (uint64_t)m, r, nullptr);
        printf("race %lld edges: above %lld, wrong %lld, failed CAS %lld, components %lld\n", (long long)m, (long long)r[1], (long long)r[2],
               (long long)r[3], (long long)r[4]);
        bad |= r[1] != 0 || r[2] != 0;
    }
    return bad;
}
#endif
