// polyfuzz_amd/csrc/k6_core.h -- the per-element decisions of K6's two kernels -- compiled for the host and driven the way
// k_linkage_top1 drives them: phase by phase, every phase a sequential loop over the rows, a round of a loop reading what the
// previous round left (the kernel's barriers make its rounds such Jacobi rounds; the pointer jumping is run from a copy, the
// slowest order the kernel's unordered reads can take).  The two-level founding scan runs over `threads` slices as the kernel's
// runs over 1024, so that a small graph can have several rows per slice.  Both loops carry the caps of k6_core.h
// (link_round_cap, link_jump_cap): a rule that does not settle ends there with a status and is counted, it does not spin.
//   k6_host_link: one top-1 result through the phases -> cluster, key, info[4] as the kernel leaves them.  rule 0: link_active of
//     k6_core.h;  rule 1: the activity rule as it stood before self-pointing rows were served (fin[x] > x), kept here only to
//     show that the caps catch it.
//   k6_host_exhaustive: every assignment g_i in {-1, 0 .. n-1} for n = 1 .. max_n ((n + 1)^n graphs, self-pointing rows
//     included) against the SEQUENTIAL walk (greedy_walk below: reference linkage.py:28-45 on ids, cluster 0 falsy) -- never
//     against the phases.  report: [0] graphs, [1] graphs whose cluster differs, [2] whose mapped strings sorted by key differ
//     from the walk's insertion order or whose unmapped strings have a key, [3] that ran into the fixpoint cap, [4] into the
//     jumping cap, [5] the most fixpoint rounds minus (n + 1) over all graphs (<= 0), [6] the most jumping rounds minus
//     link_jump_cap(n) (<= 0), [7] graphs whose info[2] is not the walk's number of foundings.
//   k6_host_kept / k6_host_bin / k6_host_fixed: kept_row, pr_bin and pr_scale + pr_fixed over arrays, for numpy to judge.
// With -DK6_HOST_MAIN: a stand-alone program (for a sanitizer run) that runs the exhaustive check and exits 1 on a violation.
#include <stddef.h>
#include <algorithm>
#include <vector>

#include "../polyfuzz_amd/csrc/k6_core.h"

using namespace pfz;

// the definition: the reference's walk over the kept rows in order.  cluster[x] = -1 while unmapped; order = dict insertion order.
static int greedy_walk(int n, const std::vector<int> &rows, const int32_t *g, int stride, std::vector<int32_t> &cluster,
                       std::vector<int32_t> &order)
{
    cluster.assign((size_t)n, -1);
    order.clear();
    int nxt = 0;
    for (int a : rows) {
        const int b = g[(size_t)a * stride];
        if (cluster[a] > 0) continue;
        if (cluster[b] <= 0) {
            if (cluster[b] < 0) order.push_back(b);
            cluster[b] = nxt;
            if (cluster[a] < 0) order.push_back(a);
            cluster[a] = nxt++;
        } else {
            if (cluster[a] < 0) order.push_back(a);
            cluster[a] = cluster[b];
        }
    }
    return nxt;
}

constexpr int kHostRootRewritten = 3;      // (this program's own finding, not a status of the kernel)

struct Rounds {
    int fixpoint, jumps;
};

static int link_phases(int n, const int32_t *idx, const float *val, int stride, double thr, int threads, int rule, int32_t *cluster,
                       int32_t *key, int32_t *info, Rounds *rounds_out)
{
    std::vector<int32_t> state((size_t)n), fin((size_t)n), ptr((size_t)n), scan((size_t)n), part((size_t)threads);
    rounds_out->fixpoint = rounds_out->jumps = 0;
    int t0 = kLinkInf;
    for (int i = 0; i < n; ++i) {
        const bool f = kept_row(idx[(size_t)i * stride], val[(size_t)i * stride], n, thr);
        state[i] = f ? 1 : 0;
        cluster[i] = key[i] = -1;
        if (f) t0 = std::min(t0, i);
    }
    info[0] = -1, info[1] = info[2] = 0, info[3] = kLinkDone;
    if (t0 == kLinkInf) return kLinkDone;
    for (int i = 0; i < n; ++i) state[i] = link_initial_state(state[i] != 0, i, t0);
    int rounds = 0;
    for (;;) {
        for (int i = 0; i < n; ++i) fin[i] = kLinkInf;
        for (int s = 0; s < n; ++s)
            if (state[s] & 1) {
                int32_t &f = fin[(size_t)idx[(size_t)s * stride]];
                f = std::min(f, s);
            }
        bool changed = false;
        for (int x = 0; x < n; ++x) {       // (state[x] is read and written by x's owner only: in place is the kernel's order)
            const int st = state[x];
            const int nst = rule == 0 ? link_active(st, fin[x], x) : ((st & 2) ? (2 | (fin[x] > x ? 1 : 0)) : st);
            if (nst != st) state[x] = nst, changed = true;
        }
        ++rounds;
        rounds_out->fixpoint = rounds;
        if (!changed) break;
        if (rounds >= link_round_cap(n)) {
            info[0] = t0, info[1] = rounds, info[3] = kLinkFixpointOverrun;
            return kLinkFixpointOverrun;
        }
    }
    const int per = (n + threads - 1) / threads;
    for (int t = 0; t < threads; ++t) {
        const int lo = std::min(n, t * per), hi = std::min(n, lo + per);
        int mine = 0;
        for (int s = lo; s < hi; ++s) {
            const int st = state[s];
            const int g = (st & 1) ? idx[(size_t)s * stride] : s;
            const int founding = (st & 1) && link_founding(s, g, fin[g], state[g]);
            scan[s] = founding;
            mine += founding;
            ptr[s] = link_pointer(st, s, g);
        }
        part[t] = mine;
    }
    int run = 0;
    for (int t = 0; t < threads; ++t) {
        const int c = part[t];
        part[t] = run;
        run += c;
    }
    info[2] = run + 1;
    for (int t = 0; t < threads; ++t) {
        const int lo = std::min(n, t * per), hi = std::min(n, lo + per);
        int r = part[t];
        for (int s = lo; s < hi; ++s) {
            const int f = scan[s];
            scan[s] = r;
            r += f;
        }
    }
    for (int x = 0; x < n; ++x)
        if (link_founded(x, fin[x], state[x])) {
            cluster[x] = 1 + scan[fin[x]];
            key[x] = 2 * fin[x];
        }
    int jumps = 0;
    for (;;) {
        const std::vector<int32_t> before = ptr;
        bool changed = false;
        for (int x = 0; x < n; ++x) {
            const int p = before[x], pp = before[p];
            if (pp != p) ptr[x] = pp, changed = true;
        }
        ++jumps;
        rounds_out->jumps = jumps;
        if (!changed) break;
        if (jumps >= link_jump_cap(n)) {
            info[0] = t0, info[1] = rounds, info[3] = kLinkJumpOverrun;
            return kLinkJumpOverrun;
        }
    }
    {
        const std::vector<int32_t> before(cluster, cluster + n);
        for (int x = 0; x < n; ++x)
            if (state[x] & 1) {
                cluster[x] = before[ptr[x]];
                key[x] = 2 * x + 1;
            }
        // the kernel reads cluster[ptr[x]] while other threads write cluster[...]: that is only sound if no root changes here
        for (int x = 0; x < n; ++x)
            if ((state[x] & 1) && cluster[ptr[x]] != before[ptr[x]]) return kHostRootRewritten;
    }
    link_patch_cluster0(t0, idx[(size_t)t0 * stride], cluster, key);
    info[0] = t0, info[1] = rounds, info[3] = kLinkDone;
    return kLinkDone;
}

extern "C" {

int k6_host_link(int n, const int32_t *idx, const float *val, int stride, double thr, int threads, int rule, int32_t *cluster,
                 int32_t *key, int32_t *info4)
{
    Rounds r;
    return link_phases(n, idx, val, stride, thr, threads, rule, cluster, key, info4, &r);
}

int k6_host_exhaustive(int max_n, int threads, int rule, int64_t *report)
{
    for (int k = 0; k < 8; ++k) report[k] = 0;
    report[5] = report[6] = -(1 << 30);
    std::vector<int32_t> want_cluster, want_order, got_order;
    for (int n = 1; n <= max_n; ++n) {
        std::vector<int32_t> g((size_t)n, -1), cluster((size_t)n), key((size_t)n);
        const std::vector<float> val((size_t)n, 0.5f);
        for (;;) {
            std::vector<int> rows;
            for (int i = 0; i < n; ++i)
                if (g[i] >= 0) rows.push_back(i);
            const int founded = greedy_walk(n, rows, g.data(), 1, want_cluster, want_order);
            int32_t info[4];
            Rounds r;
            const int status = link_phases(n, g.data(), val.data(), 1, 0.3, threads, rule, cluster.data(), key.data(), info, &r);
            ++report[0];
            report[5] = std::max<int64_t>(report[5], r.fixpoint - (n + 1));
            report[6] = std::max<int64_t>(report[6], r.jumps - link_jump_cap(n));
            if (status == kLinkFixpointOverrun) ++report[3];
            else if (status == kLinkJumpOverrun) ++report[4];
            else if (status != kLinkDone) ++report[1];
            else {
                report[1] += cluster != want_cluster;
                got_order.clear();
                bool stray = false;
                for (int x = 0; x < n; ++x) {
                    if (cluster[x] >= 0) got_order.push_back(x);
                    else stray |= key[x] != -1;
                }
                std::stable_sort(got_order.begin(), got_order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
                report[2] += stray || got_order != want_order;
                report[7] += info[2] != founded || info[0] != (rows.empty() ? -1 : rows[0]);
            }
            int i = 0;                                  // the next assignment, g as a number in base n + 1
            while (i < n && g[i] == n - 1) g[i++] = -1;
            if (i == n) break;
            ++g[i];
        }
    }
    return 0;
}

void k6_host_kept(const int32_t *g, const float *v, int64_t m, int32_t n, double thr, uint8_t *out)
{
    for (int64_t i = 0; i < m; ++i) out[i] = kept_row(g[i], v[i], n, thr) ? 1 : 0;
}

void k6_host_bin(const double *thr, int32_t n_thr, const double *v, int64_t m, int32_t *out)
{
    for (int64_t i = 0; i < m; ++i) out[i] = pr_bin(thr, n_thr, v[i]);
}

// out_fixed[i] = the signed fixed-point word of v[i] under the scale of (n, max_abs); returns the scale
double k6_host_fixed(const double *v, int64_t m, int64_t n, double max_abs, int64_t *out_fixed)
{
    const double scale = pr_scale(n, max_abs);
    for (int64_t i = 0; i < m; ++i) out_fixed[i] = (int64_t)pr_fixed(v[i], scale);
    return scale;
}

}  // extern "C"

#ifdef K6_HOST_MAIN
#include <stdio.h>
int main()
{
    int64_t r[8];
    int bad = 0;
    for (int threads : {1024, 4}) {
        k6_host_exhaustive(6, threads, 0, r);
        printf("slices %d: %lld graphs, cluster %lld, order %lld, fixpoint cap %lld, jump cap %lld, info %lld\n", threads, (long long)r[0],
               (long long)r[1], (long long)r[2], (long long)r[3], (long long)r[4], (long long)r[7]);
        bad |= r[1] || r[2] || r[3] || r[4] || r[7] || r[5] > 0 || r[6] > 0;
    }
    k6_host_exhaustive(6, 1024, 1, r);
    printf("the rule before self-pointing rows were served: %lld of %lld graphs run into the fixpoint cap\n", (long long)r[3], (long long)r[0]);
    return bad;
}
#endif
