// rls_walk_list.hpp -- what the probe walk (walk.hip) and the shadow rays' walk (csrc_shadow_walk/shadow_walk.hip) share, written
// once: both step an active list (rls_walk_rays, include/rlshaders_amd_walk.h) by the same scheme -- a decision per entry, the
// tiles' survivors counted, the trace library's scan over the counts, a stable placement -- and differ in the decision and in
// what an entry carries.  Included by both inside their anonymous namespaces, after csrc_trace/rls_trace_queue.hpp (the scan)
// and before their own kernels' header: each library compiles its own copy into its own code object, and the walks' kernels
// come out the same machine code as when each file stated these pieces itself (rlshaders_amd/codeid.py, kernel_digests).
//
// Here: the tile of a list and its survivor count (device); the scratch's carve, the checks of a ray count, a context and a
// list, the scan and placement launches, the read of a list's count (host).  A check's message names the entry point that
// refused (fn).  What names a library's own struct or function -- check_walk, the queue and found checks -- is in that library.

// A tile is kBlock entries, one per lane.
constexpr int kWalkTile = rlsh::kBlock;
constexpr int kWalkWaves = rlsh::kBlock / 64;

// the survivors of this workgroup's tile, from one ballot a wavefront; whole workgroup.  below: those on the lanes and
// wavefronts before this lane.
__device__ __forceinline__ int tile_count(int (&wtot)[kWalkWaves], bool survives, int &below)
{
    const int wave = (int)(threadIdx.x >> 6);
    const uint64_t m = __builtin_amdgcn_ballot_w64(survives);
    below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    __syncthreads();                                             // the previous tile's sums are read
    if ((threadIdx.x & 63u) == 0) wtot[wave] = __builtin_popcountll(m);
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWalkWaves; w++) {
        if (w < wave) below += wtot[w];
        total += wtot[w];
    }
    return total;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t walk_tiles(int64_t entries) { return std::max<int64_t>((entries + kWalkTile - 1) / kWalkTile, 1); }
inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

// The parts of a scratch in order, each 256-byte aligned; over a NULL base only `off`, the size, means anything.
struct Carve {
    char *base;
    size_t off;
    template <class T> T *take(int64_t count)
    {
        T *at = (T *)(base + off);
        off += align256((size_t)count * sizeof(T));
        return at;
    }
};

// ---- the argument checks, each written once; fn: the entry point its message names ---------------------------------------------
rls_status check_rays(const char *fn, int64_t rays)
{
    RLS_REQUIRE_IN(fn, rays >= 0, "rays < 0");
    RLS_REQUIRE_IN(fn, rays <= (int64_t)UINT32_MAX, "rays > 2^32 - 1 (the list's ray index is 32-bit)");
    return RLS_OK;
}
rls_status check_ctx(const char *fn, const rls_context *ctx)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    return RLS_OK;
}
// a list: its count always, its planes where it can hold an entry of the walk (in: the list a step reads, else the one written)
rls_status check_list(const char *fn, const rls_walk_rays *l, int64_t rays, bool in)
{
    RLS_REQUIRE_IN(fn, l != nullptr, in ? "in is NULL" : "out is NULL");
    RLS_REQUIRE_IN(fn, l->count != nullptr, in ? "in.count is NULL" : "out.count is NULL");
    RLS_REQUIRE_IN(fn, l->capacity >= rays, in ? "in.capacity < walk.rays" : "out.capacity < walk.rays");
    RLS_REQUIRE_IN(fn, rays == 0 || (l->ray != nullptr && rlsh::has3(l->origin) && rlsh::has3(l->dir) && l->maxdist != nullptr &&
                                     l->trials != nullptr),
                   in ? "in.ray, in.origin, in.dir, in.maxdist or in.trials plane is NULL"
                      : "out.ray, out.origin, out.dir, out.maxdist or out.trials plane is NULL");
    return RLS_OK;
}
// the two lists of a step, each checked already
rls_status check_in_is_not_out(const char *fn, const rls_walk_rays *in, const rls_walk_rays *out, int64_t rays)
{
    RLS_REQUIRE_IN(fn, in->count != out->count && (rays == 0 || (in->ray != out->ray && in->maxdist != out->maxdist)),
                   "out is in: a step reads one list and writes the other");
    return RLS_OK;
}
// the entries a step walks at most: no more than rays, which the scratch is sized by
inline int64_t step_bound(int64_t bound, int64_t rays) { return bound < 0 || bound > rays ? rays : bound; }

// steps 2 and 3 of a begin or a step: the tile counts scanned (the grand total to the output list's count), the survivors placed
// by the walk's own kernel.  IO: WalkIO or ShadowWalkIO (out, bound, tiles, counts).
template <class IO>
rls_status scan_and_place(rls_context *ctx, const IO &io, int64_t *totals, void (*place_kernel)(IO), const char *fn)
{
    rls_status s;
    const int64_t st = scan_tiles(io.tiles);
    hipLaunchKernelGGL(trace_scan_block_kernel, dim3((unsigned)st), dim3(rlsh::kBlock), 0, ctx->stream, io.counts, io.tiles, totals);
    if ((s = rlsh::check_launch("trace_scan_block_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_totals_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, totals, st, io.out.count);
    if ((s = rlsh::check_launch("trace_scan_totals_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_add_kernel, rlsh::grid_for(ctx, io.tiles), dim3(rlsh::kBlock), 0, ctx->stream, io.counts, io.tiles,
                       (const int64_t *)totals);
    if ((s = rlsh::check_launch("trace_scan_add_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(place_kernel, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

// a list's count read to the host: the one call of a walk that synchronises
rls_status list_active(const char *fn, rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count)
{
    if (rls_status s = check_ctx(fn, ctx)) return s;
    RLS_REQUIRE_IN(fn, rays != nullptr && rays->count != nullptr, "rays or rays.count is NULL");
    RLS_REQUIRE_IN(fn, host_count != nullptr, "host_count is NULL");
    RLS_HIP_TRY(hipSetDevice(ctx->device));
    RLS_HIP_TRY(hipMemcpyAsync(host_count, rays->count, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    RLS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RLS_OK;
}
