// rls_nearest_rebuild.hpp -- the rebuild of librls_nearest_rebuild.so (include/rlshaders_amd_nearest_rebuild.h): the tree the
// host builder (rls_nearest_bvh.hpp, nearest_build) makes from a moved mesh, made level by level from three presorted lists
// -- each step written once as a host + device function of one element, the whole algorithm as host loops over them
// (rebuild_host), and (under hipcc) the kernels around the same functions.  tests/native/nearest_rebuild_host_check.cpp compiles
// this file for the CPU and holds rebuild_host to nearest_build: links and leaf order exactly, boxes by value.
//
// WHY THE SHAPE IS GIVEN.  The builder splits a range of n triangles into ceil(n / 2) and floor(n / 2) and allocates children
// in pairs, depth first; a leaf holds its range.  So a node's `first`, its leaf count, its place in the node array and the
// range [begin, begin + count) of records below it are functions of (nt, leaf) alone.  A moved mesh changes the split AXIS of
// an inner node, WHICH TRIANGLE sits in which record, and the BOXES -- nothing else.  The rebuild therefore allocates and
// relinks nothing: it chooses the axes top-down and permutes the triangle ids, then runs the refit's kernels
// (rls_nearest_refit.hpp, included, not copied): records from the vertices, boxes bottom-up.
//
// THE ALGORITHM.  Per triangle the builder's lo / hi (nearest_minf / nearest_maxf in its operand order; a PARKED triangle --
// refit_finite fails on one of nine coordinates -- has lo = hi = 0) and key_c = the order key of lo_c + hi_c.
//   1. list_c, c = 0, 1, 2: the ids ordered by (key_c, id) -- a stable LSD radix sort of the 32-bit keys from id order, eight
//      passes of 4-bit digits; the tie-break by id is the sort's stability.
//   2. Top-down, a level a round.  INVARIANT: inside a node's range every list_c holds the node's triangles ordered by
//      (key_c, id).  It holds at the root by 1.  For an inner node: the axis by the builder's rule from the list ends (below);
//      mid = begin + (count + 1) / 2; the left set is list_axis[begin, mid) -- the builder's nth_element under the same total
//      order puts exactly these there; a flag a triangle id marks it; each list_c's range is partitioned STABLY by the flag
//      (an exclusive scan of the flags in list order, minus its value at `begin`), which restores the invariant for both
//      children.  node_at[k], the node position k is in (the root at first), moves to first + (k >= mid); a leaf's stay.
//   3. One lane a leaf sorts its <= 8 ids ascending (the builder's std::sort) into the records' prim.
//   4. refit_records_kernel, then the refit's level kernels, bottom-up.
//
// THE AXIS FROM THE LIST ENDS.  The builder folds cmin_c / cmax_c over a node's triangles by nearest_minf / nearest_maxf; the
// rebuild reads lo + hi of list_c[begin] and list_c[end - 1], the smallest and largest key.  The key order is the order of
// the values except that it puts -0 below +0, where the fold keeps whichever zero it met first: the two agree by VALUE, and a
// zero may differ in sign.  lo and hi are finite (or the triangle is parked), so a sum is finite or an infinity, never a NaN.
// ext_c = cmax_c - cmin_c: with a nonzero operand -0 and +0 give the same float; with two zeros the difference is a zero of
// either sign, and `>` reads -0 and +0 alike, on either side, now and when it is the ext a later axis is compared with.  An
// inf - inf is NaN under both, and a NaN on either side of `>` is false under both.  So the axis is the builder's.
//
// Only compares, copies, one float add a key and one subtract an extent, each a single IEEE operation: the CPU and the device
// agree whatever the flags.
#ifndef RLS_NEAREST_REBUILD_HPP
#define RLS_NEAREST_REBUILD_HPP

#include <stdint.h>

#include <utility>
#include <vector>

#include "rls_nearest_refit.hpp"

#define RLS_REBUILD_HD RLS_REFIT_HD
#if defined(__HIPCC__)
#define RLS_REBUILD_UNROLL _Pragma("unroll")
#else
#define RLS_REBUILD_UNROLL
#endif

constexpr int kRebuildDigitBits = 4, kRebuildDigits = 1 << kRebuildDigitBits, kRebuildPasses = 32 / kRebuildDigitBits;
constexpr int kRebuildTile = 256;                  // the sort's and the scan's tile: one element a lane of a workgroup
constexpr int kRebuildMaxLeaf = 8;

// nearest_order_key (rls_nearest_bvh.hpp) for host and device, and its inverse
RLS_REBUILD_HD uint32_t rebuild_order_key(float f)
{
    uint32_t b;
    __builtin_memcpy(&b, &f, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
RLS_REBUILD_HD float rebuild_key_value(uint32_t key)
{
    const uint32_t b = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
    float f;
    __builtin_memcpy(&f, &b, sizeof f);
    return f;
}

// the three centroid keys of a triangle from the moved vertices, as nearest_build computes them; parked: the origin's
RLS_REBUILD_HD void rebuild_keys(const float *V, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t (&key)[3])
{
    const float *a = V + 3 * (int64_t)i0, *b = V + 3 * (int64_t)i1, *c = V + 3 * (int64_t)i2;
    bool finite = true;
    for (int k = 0; k < 3; k++) finite = finite && refit_finite(a[k]) && refit_finite(b[k]) && refit_finite(c[k]);
    for (int k = 0; k < 3; k++) {
        const float lo = finite ? nearest_minf(nearest_minf(a[k], b[k]), c[k]) : 0.0f;
        const float hi = finite ? nearest_maxf(nearest_maxf(a[k], b[k]), c[k]) : 0.0f;
        key[k] = rebuild_order_key(lo + hi);
    }
}

// the builder's axis rule over the keys at a node's list ends (the argument is at the top of this file)
RLS_REBUILD_HD int rebuild_axis(const uint32_t (&kmin)[3], const uint32_t (&kmax)[3])
{
    int axis = 0;
    float ext = rebuild_key_value(kmax[0]) - rebuild_key_value(kmin[0]);
    for (int c = 1; c < 3; c++) {
        const float e = rebuild_key_value(kmax[c]) - rebuild_key_value(kmin[c]);
        if (e > ext) { ext = e; axis = c; }
    }
    return axis;
}

// the record range below a node: a function of (nt, leaf) alone
struct RebuildRange { uint32_t begin, count; };

// What an update works on.  The three lists are one array [3 * nt], list c at c * nt, and so are the keys (indexed by
// triangle id) and the scan.
struct RebuildWork {
    NearestNode *nodes;
    NearestTri *tris;
    const uint32_t *index;            // [nt * 3]: the scene's vertex indices
    const float *vertices;            // [nv * 3]: the moved mesh
    const RebuildRange *range;        // [nodes]
    uint32_t *key;                    // [3 * nt]
    uint32_t *list, *other;           // [3 * nt] each: the lists, and where a sort pass or a partition writes them
    uint32_t *scan;                   // [3 * nt]: the exclusive scan of the flags in list order
    uint32_t *node_at;                // [nt]
    uint8_t *flag;                    // [nt], by triangle id: in the left half of its node's split
    uint32_t nt, leaf;
};

// step 0, one triangle: its keys, its place in the three lists in id order, the root over its position
RLS_REBUILD_HD void rebuild_init(const RebuildWork &w, uint32_t i)
{
    const uint32_t *ix = w.index + 3 * (int64_t)i;
    uint32_t key[3];
    rebuild_keys(w.vertices, ix[0], ix[1], ix[2], key);
    for (uint32_t c = 0; c < 3; c++) {
        w.key[c * w.nt + i] = key[c];
        w.list[c * w.nt + i] = i;
    }
    w.node_at[i] = 0u;
}

// step 1, one element of list c in one pass: its digit
RLS_REBUILD_HD uint32_t rebuild_digit(const RebuildWork &w, uint32_t c, uint32_t k, int shift)
{
    return (w.key[c * w.nt + w.list[c * w.nt + k]] >> shift) & (uint32_t)(kRebuildDigits - 1);
}

// step 2, one position: where its node is inner, the node's axis from the list ends, and the flag of the triangle that stands
// at this position of the axis' list; the range's first position stores the axis
RLS_REBUILD_HD void rebuild_mark(const RebuildWork &w, uint32_t k)
{
    const uint32_t n = w.node_at[k];
    const RebuildRange r = w.range[n];
    if (r.count <= w.leaf) return;
    uint32_t kmin[3], kmax[3];
    for (uint32_t c = 0; c < 3; c++) {
        kmin[c] = w.key[c * w.nt + w.list[c * w.nt + r.begin]];
        kmax[c] = w.key[c * w.nt + w.list[c * w.nt + r.begin + r.count - 1u]];
    }
    const uint32_t axis = (uint32_t)rebuild_axis(kmin, kmax);
    const uint32_t mid = r.begin + (r.count + 1u) / 2u;
    w.flag[w.list[axis * w.nt + k]] = k < mid ? 1 : 0;
    if (k == r.begin) w.nodes[n].meta = axis << kNearestAxisShift;
}

// step 2, one position after the scan: the stable partition of the three lists, and the position's node one level down
RLS_REBUILD_HD void rebuild_partition(const RebuildWork &w, uint32_t k)
{
    const uint32_t n = w.node_at[k];
    const RebuildRange r = w.range[n];
    if (r.count <= w.leaf) {
        for (uint32_t c = 0; c < 3; c++) w.other[c * w.nt + k] = w.list[c * w.nt + k];
        return;
    }
    const uint32_t mid = r.begin + (r.count + 1u) / 2u;
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t id = w.list[c * w.nt + k];
        const uint32_t left = w.scan[c * w.nt + k] - w.scan[c * w.nt + r.begin];       // flagged ones ahead of k in the range
        const uint32_t to = w.flag[id] ? r.begin + left : mid + ((k - r.begin) - left);
        // inside [begin, begin + count) by the invariant; the compare keeps a working set that another stream's update
        // wrote into meanwhile (the caller's to order) from sending a write outside the lists
        if (to < w.nt) w.other[c * w.nt + to] = id;
    }
    w.node_at[k] = w.nodes[n].first + (k >= mid ? 1u : 0u);
}

// step 3, one node: a leaf's ids ascending into its records (every list holds the leaf's triangles in its range: list 0's)
RLS_REBUILD_HD void rebuild_leaf(const RebuildWork &w, uint32_t n)
{
    const RebuildRange r = w.range[n];
    if (r.count > w.leaf) return;
    uint32_t id[kRebuildMaxLeaf];
    RLS_REBUILD_UNROLL
    for (uint32_t j = 0; j < (uint32_t)kRebuildMaxLeaf; j++) id[j] = j < r.count ? w.list[r.begin + j] : 0xFFFFFFFFu;
    RLS_REBUILD_UNROLL
    for (int pass = 0; pass < kRebuildMaxLeaf - 1; pass++) {
        RLS_REBUILD_UNROLL
        for (int j = 0; j < kRebuildMaxLeaf - 1 - pass; j++) {
            const uint32_t a = id[j], b = id[j + 1];
            id[j] = a < b ? a : b;
            id[j + 1] = a < b ? b : a;
        }
    }
    RLS_REBUILD_UNROLL
    for (uint32_t j = 0; j < (uint32_t)kRebuildMaxLeaf; j++)
        if (j < r.count) w.tris[r.begin + j].prim = id[j];
}

// The ranges of a tree that is there, from its links, and whether they are the shape above: the root over [0, nt), an inner
// node (more than `leaf` records) split at begin + (count + 1) / 2, a leaf's first == its begin and its count == its range's.
// -> false for any other tree.
inline bool rebuild_shape(const NearestNode *nodes, int64_t node_count, int64_t nt, int leaf, std::vector<RebuildRange> &range)
{
    range.assign((size_t)(node_count > 0 ? node_count : 0), RebuildRange{0u, 0u});
    if (node_count <= 0) return node_count == 0 && nt == 0;
    if (nt <= 0 || leaf < 1 || leaf > kRebuildMaxLeaf) return false;
    std::vector<uint8_t> seen((size_t)node_count, 0);
    std::vector<std::pair<uint32_t, RebuildRange>> stack;
    stack.push_back({0u, RebuildRange{0u, (uint32_t)nt}});
    int64_t met = 0;
    while (!stack.empty()) {
        const uint32_t n = stack.back().first;
        const RebuildRange r = stack.back().second;
        stack.pop_back();
        if ((int64_t)n >= node_count || seen[n]) return false;
        seen[n] = 1;
        met++;
        range[n] = r;
        const uint32_t count = nodes[n].meta & kNearestCountMask;
        if (r.count <= (uint32_t)leaf) {
            if (count != r.count || nodes[n].first != r.begin) return false;
            continue;
        }
        if (count != 0u) return false;
        const uint32_t left = (r.count + 1u) / 2u;
        stack.push_back({nodes[n].first + 1u, RebuildRange{r.begin + left, r.count - left}});
        stack.push_back({nodes[n].first, RebuildRange{r.begin, left}});
    }
    return met == node_count;
}

// The whole rebuild on the host, for the CPU check: the steps above as loops over the one-element functions, then refit_host.
// nodes / tris: a tree of the shape (rebuild_shape's range, refit_levels' list and level count); -> the triangles parked.
inline int64_t rebuild_host(NearestNode *nodes, NearestTri *tris, int64_t nt, int leaf, const uint32_t *index, const float *V,
                            const std::vector<RebuildRange> &range, const std::vector<uint32_t> &level_list, int levels)
{
    if (nt <= 0) return 0;
    const size_t n = (size_t)nt;
    std::vector<uint32_t> key(3 * n), list(3 * n), other(3 * n), scan(3 * n), node_at(n);
    std::vector<uint8_t> flag(n, 0);
    RebuildWork w = {};
    w.nodes = nodes; w.tris = tris; w.index = index; w.vertices = V; w.range = range.data();
    w.key = key.data(); w.list = list.data(); w.other = other.data(); w.scan = scan.data(); w.node_at = node_at.data();
    w.flag = flag.data(); w.nt = (uint32_t)nt; w.leaf = (uint32_t)leaf;
    for (uint32_t i = 0; i < w.nt; i++) rebuild_init(w, i);
    for (int pass = 0; pass < kRebuildPasses; pass++) {               // 1: a stable counting sort a digit, a list at a time
        const int shift = pass * kRebuildDigitBits;
        for (uint32_t c = 0; c < 3; c++) {
            uint32_t at[kRebuildDigits + 1] = {};
            for (uint32_t k = 0; k < w.nt; k++) at[rebuild_digit(w, c, k, shift) + 1]++;
            for (int d = 0; d < kRebuildDigits; d++) at[d + 1] += at[d];
            for (uint32_t k = 0; k < w.nt; k++) w.other[c * w.nt + at[rebuild_digit(w, c, k, shift)]++] = w.list[c * w.nt + k];
        }
        std::swap(w.list, w.other);
    }
    for (int level = 1; level < levels; level++) {                     // 2: the deepest level holds leaves alone
        for (uint32_t k = 0; k < w.nt; k++) rebuild_mark(w, k);
        uint32_t sum = 0;
        for (size_t j = 0; j < 3 * n; j++) { w.scan[j] = sum; sum += w.flag[w.list[j]]; }
        for (uint32_t k = 0; k < w.nt; k++) rebuild_partition(w, k);
        std::swap(w.list, w.other);
    }
    for (size_t node = 0; node < range.size(); node++) rebuild_leaf(w, (uint32_t)node);      // 3
    return refit_host(nodes, tris, nt, index, V, level_list);          // 4
}

#if defined(__HIPCC__)
// ---- the kernels: rlsh::grid_for grids over tile loops.  No workgroup waits on another: a scan is three launches (a sum a
// tile, one workgroup over the sums, the tiles again), and every destination is a function of the inputs alone. -----------------
static_assert(kRebuildTile == rlsh::kBlock && rlsh::kBlock % 64 == 0, "one element a lane");
constexpr int kRebuildWaves = kRebuildTile / 64;

struct RebuildIO {
    RebuildWork w;
    int64_t count, tiles;             // the elements and tiles of this launch
};

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_init_kernel(RebuildIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t i = tile * kRebuildTile + threadIdx.x;
        if (i < a.count) rebuild_init(a.w, (uint32_t)i);
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_mark_kernel(RebuildIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * kRebuildTile + threadIdx.x;
        if (k < a.count) rebuild_mark(a.w, (uint32_t)k);
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_partition_kernel(RebuildIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * kRebuildTile + threadIdx.x;
        if (k < a.count) rebuild_partition(a.w, (uint32_t)k);
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_leaf_kernel(RebuildIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t n = tile * kRebuildTile + threadIdx.x;
        if (n < a.count) rebuild_leaf(a.w, (uint32_t)n);
    }
}

// The exclusive scan of one value a lane over the workgroup, and the workgroup's total.  Every lane of the workgroup calls it
// (two barriers; wave_sum is free again on return).
__device__ __forceinline__ uint32_t rebuild_block_scan(uint32_t v, uint32_t *wave_sum, uint32_t &total)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inclusive = v;
    RLS_REBUILD_UNROLL
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inclusive, d, 64);
        if (lane >= (unsigned)d) inclusive += up;
    }
    if (lane == 63u) wave_sum[wave] = inclusive;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    RLS_REBUILD_UNROLL
    for (unsigned x = 0; x < (unsigned)kRebuildWaves; x++) {
        const uint32_t s = wave_sum[x];
        before += x < wave ? s : 0u;
        total += s;
    }
    __syncthreads();
    return before + inclusive - v;
}

// A scan over `count` values, in three launches.  The values: in[j], or with `via` the flag of the triangle at list position j.
struct RebuildScanIO {
    const uint32_t *in;
    const uint32_t *via;              // NULL-able: the lists
    const uint8_t *flag;
    uint32_t *out;                    // may be `in`: a lane reads its own element ahead of writing it
    uint32_t *sums;                   // [tiles]
    int64_t count, tiles;
};

__device__ __forceinline__ uint32_t rebuild_scan_value(const RebuildScanIO &a, int64_t j)
{
    if (j >= a.count) return 0u;
    return a.via ? (uint32_t)a.flag[a.via[j]] : a.in[j];
}

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_scan_reduce_kernel(RebuildScanIO a)
{
    __shared__ uint32_t wave_sum[kRebuildWaves];
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        uint32_t total;
        (void)rebuild_block_scan(rebuild_scan_value(a, tile * kRebuildTile + threadIdx.x), wave_sum, total);
        if (threadIdx.x == 0) a.sums[tile] = total;
    }
}

// ONE workgroup: the tiles' sums scanned in place, a run of kRebuildTile at a time with the carry in a register
__global__ __launch_bounds__(rlsh::kBlock) void rebuild_scan_sums_kernel(RebuildScanIO a)
{
    __shared__ uint32_t wave_sum[kRebuildWaves];
    uint32_t carry = 0;
    for (int64_t base = 0; base < a.tiles; base += kRebuildTile) {
        const int64_t j = base + threadIdx.x;
        uint32_t total;
        const uint32_t ahead = rebuild_block_scan(j < a.tiles ? a.sums[j] : 0u, wave_sum, total);
        if (j < a.tiles) a.sums[j] = carry + ahead;
        carry += total;
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_scan_apply_kernel(RebuildScanIO a)
{
    __shared__ uint32_t wave_sum[kRebuildWaves];
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t j = tile * kRebuildTile + threadIdx.x;
        uint32_t total;
        const uint32_t ahead = rebuild_block_scan(rebuild_scan_value(a, j), wave_sum, total);
        if (j < a.count) a.out[j] = a.sums[tile] + ahead;
    }
}

// One pass of the radix sort over the three lists at once: list c has `tpa` tiles of its own (the last one short), tile t of
// the launch is tile t % tpa of list t / tpa.  counts [3][digits][tpa], list-major then digit-major, so that ONE exclusive
// scan over the whole array is every (list, digit, tile)'s first destination in the [3 * nt] array of lists.
struct RebuildSortIO {
    RebuildWork w;
    uint32_t *counts;
    int shift;
    int64_t tpa, tiles;               // tiles = 3 * tpa
};

// A lane's digit ranked in its wavefront: one ballot a bit of the digit and one of the lanes inside the list; the lanes that
// hold digit d are those that agree with d in every bit.  -> the lanes below this one with the same digit; lane d < 16 gets
// the wavefront's count of digit d in `count`.  A lane past the list's end (valid false) matches nothing.
__device__ __forceinline__ uint32_t rebuild_wave_rank(uint32_t digit, bool valid, uint32_t &count)
{
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t inside = __builtin_amdgcn_ballot_w64(valid);
    uint64_t same = inside, of_lane = inside;
    RLS_REBUILD_UNROLL
    for (int b = 0; b < kRebuildDigitBits; b++) {
        const uint64_t set = __builtin_amdgcn_ballot_w64(valid && ((digit >> b) & 1u));
        same &= ((digit >> b) & 1u) ? set : ~set;
        of_lane &= ((lane >> b) & 1u) ? set : ~set;
    }
    count = (uint32_t)__popcll(of_lane);
    return (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(rlsh::kBlock) void rebuild_sort_count_kernel(RebuildSortIO a)
{
    __shared__ uint32_t wave_count[kRebuildWaves][kRebuildDigits];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t c = (uint32_t)(tile / a.tpa);
        const int64_t t = tile - (int64_t)c * a.tpa, k = t * kRebuildTile + threadIdx.x;
        const bool valid = k < (int64_t)a.w.nt;
        const uint32_t digit = valid ? rebuild_digit(a.w, c, (uint32_t)k, a.shift) : 0u;
        uint32_t count;
        (void)rebuild_wave_rank(digit, valid, count);
        if (lane < (unsigned)kRebuildDigits) wave_count[wave][lane] = count;
        __syncthreads();
        if (threadIdx.x < (unsigned)kRebuildDigits) {
            uint32_t sum = 0;
            for (int x = 0; x < kRebuildWaves; x++) sum += wave_count[x][threadIdx.x];
            a.counts[((int64_t)c * kRebuildDigits + threadIdx.x) * a.tpa + t] = sum;
        }
        __syncthreads();
    }
}

// counts: scanned.  An element goes to its (list, digit, tile)'s first destination + the same digits in the wavefronts
// before its own + those below it in its own: the order within a digit is the order it came in, so the pass is stable.
__global__ __launch_bounds__(rlsh::kBlock) void rebuild_sort_scatter_kernel(RebuildSortIO a)
{
    __shared__ uint32_t wave_count[kRebuildWaves][kRebuildDigits];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t c = (uint32_t)(tile / a.tpa);
        const int64_t t = tile - (int64_t)c * a.tpa, k = t * kRebuildTile + threadIdx.x;
        const bool valid = k < (int64_t)a.w.nt;
        const uint32_t digit = valid ? rebuild_digit(a.w, c, (uint32_t)k, a.shift) : 0u;
        uint32_t count;
        const uint32_t rank = rebuild_wave_rank(digit, valid, count);
        if (lane < (unsigned)kRebuildDigits) wave_count[wave][lane] = count;
        __syncthreads();
        if (valid) {
            uint32_t before = 0;
            for (unsigned x = 0; x < (unsigned)kRebuildWaves; x++) before += x < wave ? wave_count[x][digit] : 0u;
            const uint32_t to = a.counts[((int64_t)c * kRebuildDigits + digit) * a.tpa + t] + before + rank;
            if (to < 3u * a.w.nt) a.w.other[to] = a.w.list[c * a.w.nt + (uint32_t)k];     // (inside by construction; as in rebuild_partition)
        }
        __syncthreads();
    }
}
#endif // __HIPCC__

#endif
