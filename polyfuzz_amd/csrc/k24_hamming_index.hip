// K24 -- a second route to K23's results for SMALL distances: pfz_hamming_join_indexed / pfz_hamming_components_indexed.  K23 computes
// every pair of codes; at hmax = 3 on 64-bit fingerprints nearly all of that work is thrown away.  The block index of k24_core.h
// (cut the d bits into hmax + 1 blocks: two codes within hmax agree completely on at least one) computes only the pairs that
// share a block's bits, and the filter is exact: the result is K23's, bit for bit.
//
//   k24_keys     a thread per (row, block): the block's key into uint32[n][m] (the hit rule reads them again), and for a to-row the
//                64-bit sort key block << 56 | key << 24 | position
//   sort         ONE sort_codes_u64 over the m n_to sort keys: block b's keys are the positions [b n_to, (b + 1) n_to), every bucket
//                one run, ordered by position inside it
//   k24_ranges   a thread per probe (from-row i, block b): the run of its partners by two binary searches inside block b's segment
//                (self-join: from position i + 1 on), the run's number of work items (k17_core.h) and, summed per wave into one
//                64-bit device word, its length -- the call's `checks`
//   scan         exclusive_scan_i32 over the probes' ITEM counts (not the run lengths: `checks` may pass 2^31 where the items, a
//                64th of them, do not), then k24_items writes the (from-row, slice) items
//   k24_probe    a wave per item, a lane per partner: XOR / popcount over the whole row in 16-byte pieces, left as soon as h > hmax;
//                on h <= hmax the first-block rule on the stored keys; the hits leave as K23's do -- one reservation per wave that
//                holds a hit, key = row << 32 | col with h beside it while there is room, or united in K12's forest
//
// The route (PFZ_HAMMING_INDEX_AUTO) is decided behind the sort and the scan, where `checks` is known: the index runs iff
// checks * kK24AutoRatio <= all pairs, otherwise K23's tile program runs inside the same call (hamming_join_run /
// hamming_comp_run of k23_hamming_join.hip).
#include "k24_core.h"
#include "k23_core.h"

namespace pfz {

// the call's device words, a 256-byte line apart as k23_core.h explains
enum { kK24Hits = 0, kK24Checks = kK23Line, kK24Roots = 2 * kK23Line, kK24Words = 3 * kK23Line };

struct K24Args {
    const uint8_t *A, *B;            // the rows of the from- and the to-codes, `pitch` bytes each (whole 16-byte pieces, zero padded)
    uint32_t *ka, *kb;               // [n][m] block keys (self-join: the same array)
    uint64_t *skeys;                 // [m n_b] sort keys; behind the sort: ascending
    int32_t *run_lo, *run_hi;        // [n_a m] every probe's run [lo, hi) of the sorted keys
    int32_t *item_ptr;               // [n_a m + 1] items per probe, scanned in place
    PairItem *items;                 // .row = the FROM-ROW; the block is the sorted keys' own top byte
    int64_t n_a, n_b, n_items;
    int32_t d, m, pitch, hmax, self;
    uint64_t *keys;                  // join sink
    int32_t *dist;
    unsigned long long capacity;
    int32_t *parent;                 // unite sink
    unsigned long long *state;
};

__global__ __launch_bounds__(256) void k24_keys(const uint8_t *__restrict__ rows, int64_t n, int32_t d, int32_t m, int32_t pitch,
                                                uint32_t *__restrict__ keys, uint64_t *__restrict__ skeys)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n * m) return;
    const int64_t r = c / m;
    const int32_t b = (int32_t)(c - r * m);
    const uint32_t key = k24_block_key(rows + r * pitch, k24_block_lo(d, m, b), k24_block_lo(d, m, b + 1));
    keys[c] = key;
    if (skeys) skeys[c] = k24_sort_key(b, key, (int32_t)r);
}

__global__ __launch_bounds__(256) void k24_ranges(K24Args P)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int len = 0;
    if (c < P.n_a * P.m) {
        const int64_t i = c / P.m;
        const int32_t b = (int32_t)(c - i * P.m);
        int64_t p0, p1;
        k24_probe_run(P.skeys, P.n_b, b, P.ka[c], (int32_t)i, P.self != 0, &p0, &p1);
        P.run_lo[c] = (int32_t)p0;
        P.run_hi[c] = (int32_t)p1;
        len = (int)(p1 - p0);
        P.item_ptr[c] = pair_item_count(len, kPairSlice);
    }
    // (a run is shorter than 2^24 and a wave has 64 of them: the sum fits)
    const int all = __shfl(wave_scan_i32(len, lane), 63, 64);
    if (lane == 0 && all) atomicAdd(P.state + kK24Checks, (unsigned long long)all);
}

__global__ __launch_bounds__(256) void k24_items(K24Args P)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= P.n_a * P.m) return;
    const int32_t first = P.item_ptr[c], n = P.item_ptr[c + 1] - first, row = (int32_t)(c / P.m);
    for (int32_t k = 0; k < n; ++k) P.items[first + k] = pair_item_slice(row, P.run_lo[c], P.run_hi[c], k, kPairSlice);
}

template <DenseSink kSink>
__device__ __forceinline__ void k24_probe_body(const K24Args &P)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 4;
    const int pieces = P.pitch / 16, hmax = P.hmax, m = P.m;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < P.n_items; it += stride) {      // (uniform in a wave)
        const PairItem item = P.items[it];
        const int32_t i = item.row;
        const uint4 *a = reinterpret_cast<const uint4 *>(P.A + (int64_t)i * P.pitch);
        for (int64_t q = item.p0; q < item.p1; q += 64) {      // (one round with the measured slice of 64)
            const int64_t p = q + lane;
            bool hit = false;
            int32_t j = 0, h = 0;
            if (p < item.p1) {
                const uint64_t s = P.skeys[p];
                j = k24_sort_key_pos(s);
                const uint4 *bb = reinterpret_cast<const uint4 *>(P.B + (int64_t)j * P.pitch);
                for (int k = 0; k < pieces && h <= hmax; ++k) {
                    const uint4 x = a[k], y = bb[k];
                    h += __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
                }
                hit = h <= hmax && k24_first_block(P.ka + (int64_t)i * m, P.kb + (int64_t)j * m, k24_sort_key_block(s));
            }
            const unsigned long long held = __ballot(hit);
            if (!held) continue;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(P.state + kK24Hits, (unsigned long long)__popcll(held));
            if (kSink == kSinkUnite) {
                if (hit) uf_unite<UfDeviceOps>(P.parent, i, j);
                continue;
            }
            base = __shfl(base, 0, 64);
            const unsigned long long pos = base + (unsigned long long)__popcll(held & ((1ull << lane) - 1));
            if (hit && pos < P.capacity) {
                P.keys[pos] = (uint64_t)(uint32_t)i << 32 | (uint64_t)(uint32_t)j;
                P.dist[pos] = h;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k24_probe_join(K24Args P) { k24_probe_body<kSinkJoin>(P); }
__global__ __launch_bounds__(256) void k24_probe_comp(K24Args P) { k24_probe_body<kSinkUnite>(P); }

static int hamming_operand(const char *who, const char *side, const pfz_dense *m)
{
    PFZ_REQUIRE(m->dtype == PFZ_DENSE_B1, "%s: the %s are %s; the Hamming threshold kernels take binary operands only (pfz_dense_upload1)", who,
                side, dense_dtype_name(m->dtype));
    if (m->n >= ((int64_t)1 << 31)) {
        set_error("%s: %lld rows exceed the 32-bit positions", who, (long long)m->n);
        return PFZ_ERR_UNSUPPORTED;
    }
    return PFZ_OK;
}

// why a call has no block index (NULL: it has one)
static const char *k24_refusal(int64_t d, int64_t hmax, int64_t n_from, int64_t n_to, char *buf, size_t room)
{
    const int64_t m = hmax + 1;
    if (m > d) snprintf(buf, room, "max_distance %lld leaves no bit for each of its %lld blocks (%lld bits)", (long long)hmax, (long long)m, (long long)d);
    else if (m > kK24MaxBlocks) snprintf(buf, room, "max_distance %lld needs %lld blocks, the limit is %d", (long long)hmax, (long long)m, kK24MaxBlocks);
    else if (!k24_indexable(d, hmax)) snprintf(buf, room, "%lld bits at max_distance %lld have no block index", (long long)d, (long long)hmax);
    else if (n_from >= kK24MaxRows || n_to >= kK24MaxRows) snprintf(buf, room, "a list of 2^24 rows or more (%lld, %lld)", (long long)n_from, (long long)n_to);
    else if (!k24_rows_indexable(n_from, n_to, m)) snprintf(buf, room, "%lld blocks times %lld rows reach 2^31 sort keys", (long long)m, (long long)std::max(n_from, n_to));
    else return nullptr;
    return buf;
}

struct K24Run {
    DevBuf ka, kb, raw, skeys, run_lo, run_hi, item_ptr, items, state;
    K24Args P = {};
    int64_t checks = 0, n_items = 0;
};

static inline unsigned k24_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// keys, sort, ranges and scan; behind it the host knows `checks` and the number of items.  *too_many: the items pass 2^31
static int k24_index(pfz_ctx *ctx, const pfz_dense *F, const pfz_dense *T, bool self, int64_t hmax, K24Run *w, bool *too_many)
{
    K24Args &P = w->P;
    P.A = (const uint8_t *)F->x;
    P.B = (const uint8_t *)T->x;
    P.n_a = F->n;
    P.n_b = T->n;
    P.d = (int32_t)F->dim;
    P.m = (int32_t)(hmax + 1);
    P.pitch = (int32_t)(F->ld / 8);
    P.hmax = (int32_t)hmax;
    P.self = self ? 1 : 0;
    const int64_t n_keys = P.n_b * P.m, n_probes = P.n_a * P.m;
    PFZ_TRY(w->kb.alloc(ctx, (size_t)n_keys * sizeof(uint32_t)));
    PFZ_TRY(w->raw.alloc(ctx, (size_t)n_keys * sizeof(uint64_t)));
    PFZ_TRY(w->skeys.alloc(ctx, (size_t)sort_codes_capacity(n_keys) * sizeof(uint64_t)));
    PFZ_TRY(w->run_lo.alloc(ctx, (size_t)n_probes * sizeof(int32_t)));
    PFZ_TRY(w->run_hi.alloc(ctx, (size_t)n_probes * sizeof(int32_t)));
    PFZ_TRY(w->item_ptr.alloc(ctx, (size_t)(n_probes + 1) * sizeof(int32_t)));
    PFZ_TRY(w->state.alloc(ctx, kK24Words * sizeof(unsigned long long)));
    PFZ_HIP(hipMemsetAsync(w->state.p, 0, kK24Words * sizeof(unsigned long long), ctx->stream));
    P.kb = w->kb.as<uint32_t>();
    P.ka = P.kb;
    P.skeys = w->skeys.as<uint64_t>();
    P.run_lo = w->run_lo.as<int32_t>();
    P.run_hi = w->run_hi.as<int32_t>();
    P.item_ptr = w->item_ptr.as<int32_t>();
    P.state = w->state.as<unsigned long long>();
    {
        ProfScope ps(ctx, "k24_keys");
        hipLaunchKernelGGL(k24_keys, dim3(k24_blocks(n_keys)), dim3(256), 0, ctx->stream, P.B, P.n_b, P.d, P.m, P.pitch, P.kb, w->raw.as<uint64_t>());
        PFZ_HIP(hipGetLastError());
        if (!self) {
            PFZ_TRY(w->ka.alloc(ctx, (size_t)n_probes * sizeof(uint32_t)));
            P.ka = w->ka.as<uint32_t>();
            hipLaunchKernelGGL(k24_keys, dim3(k24_blocks(n_probes)), dim3(256), 0, ctx->stream, P.A, P.n_a, P.d, P.m, P.pitch, P.ka, (uint64_t *)nullptr);
            PFZ_HIP(hipGetLastError());
        }
    }
    {
        ProfScope ps(ctx, "k24_sort");
        PFZ_TRY(sort_codes_u64(ctx, w->raw.as<uint64_t>(), P.skeys, n_keys));
    }
    unsigned long long state[kK24Words];
    {
        ProfScope ps(ctx, "k24_ranges");
        hipLaunchKernelGGL(k24_ranges, dim3(k24_blocks(n_probes)), dim3(256), 0, ctx->stream, P);
        PFZ_HIP(hipGetLastError());
        PFZ_TRY(exclusive_scan_i32(ctx, P.item_ptr, n_probes));
        PFZ_TRY(copy_d2h(ctx, state, w->state.p, sizeof(state)));      // (waits)
    }
    w->raw.reset();
    w->checks = (int64_t)state[kK24Checks];
    // every probe's last item may be short, the others are full (pair_item_bound): below 2^31, or the scan's words have wrapped
    *too_many = pair_item_bound(n_probes, w->checks, kPairSlice) >= ((int64_t)1 << 31);
    if (*too_many) return PFZ_OK;
    int32_t n_items = 0;
    PFZ_TRY(copy_d2h(ctx, &n_items, P.item_ptr + n_probes, sizeof(n_items)));
    w->n_items = P.n_items = n_items;
    return PFZ_OK;
}

// the items and the probe launch (enqueued)
static int k24_probe(pfz_ctx *ctx, K24Run *w, bool unite)
{
    K24Args &P = w->P;
    if (P.n_items == 0) return PFZ_OK;
    PFZ_TRY(w->items.alloc(ctx, (size_t)P.n_items * sizeof(PairItem)));
    P.items = w->items.as<PairItem>();
    hipLaunchKernelGGL(k24_items, dim3(k24_blocks(P.n_a * P.m)), dim3(256), 0, ctx->stream, P);
    PFZ_HIP(hipGetLastError());
    // four waves a workgroup, the items dealt round robin over at most 32 waves per compute unit's worth of workgroups
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((P.n_items + 3) / 4, (int64_t)ctx->prop.multiProcessorCount * 32));
    if (unite) hipLaunchKernelGGL(k24_probe_comp, dim3((unsigned)grid), dim3(256), 0, ctx->stream, P);
    else hipLaunchKernelGGL(k24_probe_join, dim3((unsigned)grid), dim3(256), 0, ctx->stream, P);
    PFZ_HIP(hipGetLastError());
    return PFZ_OK;
}

// all pairs of a call, saturated
static int64_t k24_all_pairs(int64_t n_from, int64_t n_to, bool self) { return self ? n_from * (n_from - 1) / 2 : n_from * n_to; }

static void k24_counters(int64_t *out, int64_t d, int64_t hmax, int64_t checks, int64_t items, int64_t route)
{
    if (!out) return;
    const bool plan = k24_indexable(d, hmax);
    out[0] = plan ? hmax + 1 : 0;
    out[1] = plan ? k24_block_min(d, hmax + 1) : 0;
    out[2] = checks;
    out[3] = items;
    out[4] = route;
}

// *route = 1: the index runs; 0: the tiles do (AUTO).  BLOCKS without an index: PFZ_ERR_UNSUPPORTED with the reason
static int k24_route(const char *who, pfz_ctx *ctx, const pfz_dense *F, const pfz_dense *T, bool self, int64_t hmax, int32_t mode, K24Run *w,
                     int *route)
{
    char buf[160];
    const char *why = k24_refusal(F->dim, hmax, F->n, T->n, buf, sizeof(buf));
    if (!why) {
        bool too_many = false;
        PFZ_TRY(k24_index(ctx, F, T, self, hmax, w, &too_many));
        if (too_many) {
            snprintf(buf, sizeof(buf), "%lld candidate checks need 2^31 work items or more", (long long)w->checks);
            why = buf;
        }
    }
    *route = 0;
    if (why) {
        if (mode == PFZ_HAMMING_INDEX_AUTO) return PFZ_OK;
        set_error("%s: no block index: %s", who, why);
        return PFZ_ERR_UNSUPPORTED;
    }
    // checks * R <= all pairs, without the product: checks <= all / R
    *route = mode == PFZ_HAMMING_INDEX_BLOCKS || w->checks <= k24_all_pairs(F->n, T->n, self) / kK24AutoRatio ? 1 : 0;
    return PFZ_OK;
}

static int hamming_join_indexed_run(pfz_ctx *ctx, const pfz_dense *F, const pfz_dense *T, bool self, int64_t hmax, int32_t mode, int64_t capacity,
                                    int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, int64_t *out_total, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_total = 0;
    k24_counters(out_counters, 0, -1, 0, 0, 0);
    const int64_t n_from = F->n;
    if (n_from == 0 || T->n == 0) {
        for (int64_t r = 0; r <= n_from; ++r) out_row_ptr[r] = 0;
        return PFZ_OK;
    }
    K24Run w;
    int route = 0;
    PFZ_TRY(k24_route("pfz_hamming_join_indexed", ctx, F, T, self, hmax, mode, &w, &route));
    k24_counters(out_counters, F->dim, hmax, w.checks, w.n_items, route);
    if (route == 0) {
        w = K24Run();      // (the index's blocks go back before the tiles ask for theirs)
        return hamming_join_run(ctx, F, T, self, hmax, capacity, out_row_ptr, out_idx, out_dist, out_total, nullptr);
    }
    DevBuf d_keys, d_vals;
    PFZ_TRY(d_keys.alloc(ctx, (size_t)capacity * sizeof(uint64_t)));
    PFZ_TRY(d_vals.alloc(ctx, (size_t)capacity * sizeof(int32_t)));
    w.P.keys = d_keys.as<uint64_t>();
    w.P.dist = d_vals.as<int32_t>();
    w.P.capacity = (unsigned long long)capacity;
    unsigned long long state[kK24Words];
    {
        ProfScope ps(ctx, "k24_probe");
        PFZ_TRY(k24_probe(ctx, &w, false));
        PFZ_TRY(copy_d2h(ctx, state, w.state.p, sizeof(state)));      // (waits for the kernels)
    }
    const int64_t total = (int64_t)state[kK24Hits];
    *out_total = total;
    if (total > capacity) return PFZ_OK;       // the caller's buffers stay as they are: it repeats the call with room for `total`
    return join_sort_unpack(ctx, "k24_sort_unpack", d_keys.as<uint64_t>(), d_vals.as<uint32_t>(), total, n_from, out_row_ptr, out_idx,
                            reinterpret_cast<float *>(out_dist));
}

static int hamming_comp_indexed_run(pfz_ctx *ctx, const pfz_dense *V, int64_t hmax, int32_t mode, int32_t *out_label, int64_t *out_pairs,
                                    int64_t *out_components, int64_t *out_counters)
{
    PFZ_HIP(hipSetDevice(ctx->device));
    *out_pairs = *out_components = 0;
    k24_counters(out_counters, 0, -1, 0, 0, 0);
    const int64_t n = V->n;
    if (n == 0) return PFZ_OK;
    K24Run w;
    int route = 0;
    PFZ_TRY(k24_route("pfz_hamming_components_indexed", ctx, V, V, true, hmax, mode, &w, &route));
    k24_counters(out_counters, V->dim, hmax, w.checks, w.n_items, route);
    if (route == 0) {
        w = K24Run();
        return hamming_comp_run(ctx, V, hmax, out_label, out_pairs, out_components, nullptr);
    }
    ForestRun forest;
    PFZ_TRY(forest.alloc(ctx, n));
    w.P.parent = forest.parent.as<int32_t>();
    {
        ProfScope ps(ctx, "k24_components");
        PFZ_TRY(forest.begin(ctx));
        PFZ_TRY(k24_probe(ctx, &w, true));
        PFZ_TRY(forest.flatten(ctx, w.P.state + kK24Roots));
    }
    unsigned long long state[kK24Words];
    PFZ_TRY(copy_d2h(ctx, state, w.state.p, sizeof(state)));
    PFZ_TRY(forest.download(ctx, out_label));
    *out_pairs = (int64_t)state[kK24Hits];
    *out_components = (int64_t)state[kK24Roots];
    return PFZ_OK;
}

}  // namespace pfz

using namespace pfz;

extern "C" {

int pfz_hamming_join_indexed(pfz_ctx *ctx, const pfz_dense *from, const pfz_dense *to, int64_t max_distance, int32_t mode, int64_t capacity,
                             int64_t *out_row_ptr, int32_t *out_idx, int32_t *out_dist, int64_t *out_total, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && from, "pfz_hamming_join_indexed: NULL argument");
    PFZ_REQUIRE(mode == PFZ_HAMMING_INDEX_BLOCKS || mode == PFZ_HAMMING_INDEX_AUTO, "pfz_hamming_join_indexed: mode %d is neither BLOCKS nor AUTO", (int)mode);
    PFZ_REQUIRE(capacity >= 0, "pfz_hamming_join_indexed: capacity %lld < 0", (long long)capacity);
    PFZ_REQUIRE(out_row_ptr && out_total, "pfz_hamming_join_indexed: NULL out_row_ptr / out_total");
    PFZ_REQUIRE(capacity == 0 || (out_idx && out_dist), "pfz_hamming_join_indexed: NULL output with capacity %lld", (long long)capacity);
    const bool self = to == nullptr || to == from;
    const pfz_dense *T = self ? from : to;
    PFZ_TRY(hamming_operand("pfz_hamming_join_indexed", "from-codes", from));
    PFZ_TRY(hamming_operand("pfz_hamming_join_indexed", "to-codes", T));
    PFZ_REQUIRE(from->dim == T->dim, "pfz_hamming_join_indexed: from-codes have %lld bits, to-codes %lld", (long long)from->dim, (long long)T->dim);
    PFZ_REQUIRE(max_distance >= 0 && max_distance <= from->dim, "pfz_hamming_join_indexed: max_distance %lld is outside [0, %lld]",
                (long long)max_distance, (long long)from->dim);
    return hamming_join_indexed_run(ctx, from, T, self, max_distance, mode, capacity, out_row_ptr, out_idx, out_dist, out_total, out_counters);
}

int pfz_hamming_components_indexed(pfz_ctx *ctx, const pfz_dense *codes, int64_t max_distance, int32_t mode, int32_t *out_label,
                                   int64_t *out_pairs, int64_t *out_components, int64_t *out_counters)
{
    PFZ_REQUIRE(ctx && codes, "pfz_hamming_components_indexed: NULL argument");
    PFZ_REQUIRE(mode == PFZ_HAMMING_INDEX_BLOCKS || mode == PFZ_HAMMING_INDEX_AUTO, "pfz_hamming_components_indexed: mode %d is neither BLOCKS nor AUTO", (int)mode);
    PFZ_REQUIRE(out_pairs && out_components, "pfz_hamming_components_indexed: NULL out_pairs / out_components");
    PFZ_REQUIRE(codes->n == 0 || out_label, "pfz_hamming_components_indexed: NULL out_label");
    PFZ_TRY(hamming_operand("pfz_hamming_components_indexed", "codes", codes));
    PFZ_REQUIRE(max_distance >= 0 && max_distance <= codes->dim, "pfz_hamming_components_indexed: max_distance %lld is outside [0, %lld]",
                (long long)max_distance, (long long)codes->dim);
    return hamming_comp_indexed_run(ctx, codes, max_distance, mode, out_label, out_pairs, out_components, out_counters);
}

int pfz_hamming_index_plan(int64_t dim_bits, int64_t max_distance, int64_t *out)
{
    PFZ_REQUIRE(out, "pfz_hamming_index_plan: NULL out");
    PFZ_REQUIRE(dim_bits >= 1 && dim_bits < ((int64_t)1 << 24), "pfz_hamming_index_plan: %lld bits are outside [1, 2^24)", (long long)dim_bits);
    PFZ_REQUIRE(max_distance >= 0 && max_distance <= dim_bits, "pfz_hamming_index_plan: max_distance %lld is outside [0, %lld]",
                (long long)max_distance, (long long)dim_bits);
    char buf[160];
    const char *why = k24_refusal(dim_bits, max_distance, 0, 0, buf, sizeof(buf));
    if (why) {
        set_error("pfz_hamming_index_plan: no block index: %s", why);
        return PFZ_ERR_UNSUPPORTED;
    }
    const int64_t m = max_distance + 1;
    out[0] = m;
    out[1] = k24_block_min(dim_bits, m);
    out[2] = k24_block_max(dim_bits, m);
    out[3] = kK24AutoRatio;
    return PFZ_OK;
}

}  // extern "C"
