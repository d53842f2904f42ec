// rls_trace_route.hpp -- routing a queue's hits to the nodes (part of trace.hip, included there inside its anonymous namespace,
// after rls_trace_opacity.hpp): the stable partition of the rays by the node bin they hit (rls_trace_route_hits) and the movers
// between ray order and a bin's dense batch (rls_trace_route_gather / _scatter / _fill).  Pure data movement: mode-free, in the
// EXACT unit like state_advance_kernel.
//
// The partition is a counting sort over at most 17 keys (bins + the misses), three steps on the context's stream:
//   1. route_count_kernel: per tile of kRouteTile rays the count of every key, bin-major: counts[key * tiles + tile].
//   2. the queues' scan (trace_scan_{block,totals,add}_kernel) over those (bins + 1) * tiles counts: one exclusive scan of a
//      bin-major matrix gives every (key, tile) pair its first position in `order`; the value at (key, tile 0) is offsets[key].
//   3. route_place_kernel: the tile's keys again, each ray ranked among the tile's rays of its key, order[base + rank] = ray.
// Every position is a function of the inputs alone: the ranks come from wavefront ballots (v_mbcnt below the lane) and running
// counts, no atomic anywhere.
//
// A tile is four runs of kRouteTile / 4 consecutive rays, one per wavefront, walked in rounds of 64: ray order within the tile is
// (wavefront, round, lane).  A wavefront ranks its rays key by key: for each of the call's bins + 1 keys one ballot per round,
// the rays of the key ranked by the lanes below them (v_mbcnt) and the key's running count, a scalar; lane b of every
// wavefront ends up with the wavefront's count of key b.  The work grows with the call's bin count, not with the keys present.
//
// The stores of `order` are direct: within a round the lanes of one key write consecutive words, and the next round of the same
// wavefront continues each run, so a key with share s of the rays gets 256 s bytes per round -- whole cache lines from s = 1/2,
// and the L2 merges the partial lines of consecutive rounds.  Staging the tile's runs through LDS would make every run one
// store of up to 8 KiB at the price of another barrier, 8 KiB of LDS and an LDS round trip per ray.  Measured, the place kernel
// takes what the count kernel takes plus what a copy of the stored bytes takes, and neither is bound by memory: the staging
// had nothing to win and was not built ("Routing hits to the nodes").

#if !RLS_FAST
constexpr int kRouteKeys = RLS_ROUTE_MAX_BINS + 1;                 // the bins and the misses
constexpr int kRouteWaves = rlsh::kBlock / 64;
constexpr int kRoutePer = 8;                                       // rounds of 64 rays per wavefront and tile
constexpr int kRouteTile = rlsh::kBlock * kRoutePer;
static_assert(kRouteKeys <= 64, "lane L of a wavefront carries the count of key L");
static_assert(kRouteTile == kScanTile, "the partition tile is the scan tile");

struct RouteIO {
    const uint8_t *bin;
    int64_t *counts;             // [(bins + 1) * tiles + 1]: step 1 writes, step 2 scans in place, step 3 reads
    int64_t *offsets;            // [bins + 2]
    uint32_t *order, *slot;      // slot NULL-able
    int64_t rays, tiles;
    int bins;
};
struct RouteMoveIO {
    rls_route_planes p;
    const uint32_t *index;
    int64_t m;
};
struct RouteFillIO {
    float *dst[RLS_ROUTE_MAX_W32];
    float value[RLS_ROUTE_MAX_W32];
    const uint32_t *index;
    int64_t m;
    int n_planes;
};

// the kernel's argument struct where it lies, in the kernarg segment: a plane pointer picked by a loop counter is then one
// scalar load at a uniform offset, where indexing the by-value copy would move the whole struct to scratch memory first
// (reload_args, rls_internal.hpp, reads the same segment for the pointwise kernels).  IO must be the kernel's only parameter.
#if defined(__HIP_DEVICE_COMPILE__)
#define RLS_ROUTE_KERNARG(IO, a) ((const __attribute__((address_space(4))) IO *)__builtin_amdgcn_kernarg_segment_ptr())
#define RLS_ROUTE_GLOBAL(T, p) ((__attribute__((address_space(1))) T *)(p))
#else
#define RLS_ROUTE_KERNARG(IO, a) (&(a))
#define RLS_ROUTE_GLOBAL(T, p) ((T *)(p))
#endif

// A wavefront's kRoutePer rounds, key by key: the outer loop runs over the call's keys (uniform: every lane takes every
// ballot), the inner over the rounds with the key's running count in a scalar, so no iteration waits on another's ballot.
// rank[u]: the rank of round u's ray among the wavefront's rays of its key -- the earlier rounds' and this round's lower lanes
// (RANK false: not formed).  Returns, in lane b <= bins, the wavefront's count of key b.  key[u] < 0: no ray.
template <bool RANK>
__device__ __forceinline__ int route_wave(const int (&key)[kRoutePer], int (&rank)[kRoutePer], int bins, int lane)
{
    int run = 0;
    for (int b = 0; b <= bins; b++) {
        int before = 0;
#pragma unroll
        for (int u = 0; u < kRoutePer; u++) {
            const bool mine = key[u] == b;
            const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
            if (RANK && mine)
                rank[u] = before + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            before += __builtin_popcountll(m);
        }
        if (lane == b) run = before;
    }
    return run;
}

// the key of ray k: its bin, or `bins` for every other value
__device__ __forceinline__ int route_key(const uint8_t *bin, int64_t k, int bins)
{
    const int b = bin[k];
    return b < bins ? b : bins;
}

__global__ __launch_bounds__(rlsh::kBlock) void route_count_kernel(RouteIO a)
{
    __shared__ int wtot[kRouteWaves][kRouteKeys];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k0 = tile * kRouteTile + (int64_t)wave * (kRouteTile / kRouteWaves) + lane;
        int key[kRoutePer], rank[kRoutePer];
#pragma unroll
        for (int u = 0; u < kRoutePer; u++) key[u] = k0 + u * 64 < a.rays ? route_key(a.bin, k0 + u * 64, a.bins) : -1;
        const int run = route_wave<false>(key, rank, a.bins, lane);
        __syncthreads();                                         // the previous tile's sums are read
        if (lane < kRouteKeys) wtot[wave][lane] = run;
        __syncthreads();
        if ((int)threadIdx.x <= a.bins) {
            int64_t c = 0;
#pragma unroll
            for (int w = 0; w < kRouteWaves; w++) c += wtot[w][threadIdx.x];
            a.counts[(int64_t)threadIdx.x * a.tiles + tile] = c;
        }
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void route_place_kernel(RouteIO a)
{
    __shared__ int wtot[kRouteWaves][kRouteKeys];
    __shared__ int64_t wbase[kRouteWaves][kRouteKeys];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    // offsets: the scanned count at (key, tile 0); the grand total behind the last key.  No ray: all 0, nothing scanned.
    if (blockIdx.x == 0 && (int)threadIdx.x <= a.bins + 1)
        a.offsets[threadIdx.x] = a.rays == 0 ? 0 : (int)threadIdx.x <= a.bins ? a.counts[(int64_t)threadIdx.x * a.tiles] : a.rays;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k0 = tile * kRouteTile + (int64_t)wave * (kRouteTile / kRouteWaves) + lane;
        int key[kRoutePer], rank[kRoutePer];
#pragma unroll
        for (int u = 0; u < kRoutePer; u++) key[u] = k0 + u * 64 < a.rays ? route_key(a.bin, k0 + u * 64, a.bins) : -1;
        const int run = route_wave<true>(key, rank, a.bins, lane);
        __syncthreads();                                         // the previous tile's bases are read
        if (lane < kRouteKeys) wtot[wave][lane] = run;
        __syncthreads();
        if (lane <= a.bins) {
            int64_t base = a.counts[(int64_t)lane * a.tiles + tile];
            for (int w = 0; w < wave; w++) base += wtot[w][lane];
            wbase[wave][lane] = base;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kRoutePer; u++) {
            if (key[u] < 0) continue;
            const int64_t at = wbase[wave][key[u]] + rank[u];
            const int64_t k = k0 + u * 64;
            a.order[at] = (uint32_t)k;
            if (a.slot) a.slot[k] = (uint32_t)at;
        }
    }
}

// The movers: one element per lane, its index in a register, the planes one after another -- four loads in flight, then their
// four stores.  The planes move as bits: no float instruction touches a word.
// GATHER: dst[j] = src[index[j]]; else dst[index[j]] = src[j].
template <class T, bool GATHER, class S, class D>
__device__ __forceinline__ void route_move_planes(S src, D dst, int n, int64_t j, int64_t k)
{
    const int64_t from = GATHER ? k : j, to = GATHER ? j : k;
    int p = 0;
    for (; p + 4 <= n; p += 4) {
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = RLS_ROUTE_GLOBAL(const T, src[p + u])[from];
#pragma unroll
        for (int u = 0; u < 4; u++) RLS_ROUTE_GLOBAL(T, dst[p + u])[to] = v[u];
    }
    for (; p < n; p++) RLS_ROUTE_GLOBAL(T, dst[p])[to] = RLS_ROUTE_GLOBAL(const T, src[p])[from];
}

template <bool GATHER>
__device__ __forceinline__ void route_move(const RouteMoveIO &a)
{
    const auto ka = RLS_ROUTE_KERNARG(RouteMoveIO, a);
    const int64_t m = ka->m;
    const int nw = ka->p.n_w32, nb = ka->p.n_u8;
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t k = RLS_ROUTE_GLOBAL(const uint32_t, ka->index)[j];
        route_move_planes<uint32_t, GATHER>(ka->p.src_w32, ka->p.dst_w32, nw, j, k);
        route_move_planes<uint8_t, GATHER>(ka->p.src_u8, ka->p.dst_u8, nb, j, k);
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void route_gather_kernel(RouteMoveIO a) { route_move<true>(a); }
__global__ __launch_bounds__(rlsh::kBlock) void route_scatter_kernel(RouteMoveIO a) { route_move<false>(a); }

__global__ __launch_bounds__(rlsh::kBlock) void route_fill_kernel(RouteFillIO a)
{
    const auto ka = RLS_ROUTE_KERNARG(RouteFillIO, a);
    const int64_t m = ka->m;
    const int n = ka->n_planes;
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t k = RLS_ROUTE_GLOBAL(const uint32_t, ka->index)[j];
        for (int p = 0; p < n; p++) RLS_ROUTE_GLOBAL(float, ka->dst[p])[k] = ka->value[p];
    }
}
#endif
