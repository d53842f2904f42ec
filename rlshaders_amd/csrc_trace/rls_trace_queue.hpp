// rls_trace_queue.hpp -- what every compacted queue shares (part of trace.hip, included there inside its anonymous namespace):
// steps 2 and 3 of an emit and the resolves.
//   2. trace_scan_{block,totals,add}_kernel: offsets[0, n) scanned in place (exclusive), offsets[n] = the ray count.  A
//      multi-kernel scan (tiles, then the tile sums in one workgroup, then the add-back): no workgroup waits on another.
//   3. trace_compact_kernel / shadow_compact_kernel: per tile of points, the kept records move from their staging slots to
//      offsets[i] + rank, transposed through LDS (staging rows in, the tile's contiguous queue range out).
// Both are the same for every closure.  Every position is a function of the inputs: no atomics anywhere.
//
// Resolve (trace_resolve_kernel): per point the sequential sum over its rays in queue order; the products
// radiance x weight of a tile of rays are formed with coalesced loads into LDS, then each lane adds its point's ones.  The
// glossy resolve serves the rlGgx glossy and both rlDisney queues.  shadow_resolve_kernel: the same for a light loop's queue.
// Their tile walks (ray_sums, ray_sums_about_reference, shadow_sums) are the node resolves' too.

#if !RLS_FAST
// exclusive scan of offsets[0, n): each workgroup one tile, its sum to totals[tile]
__global__ __launch_bounds__(rlsh::kBlock) void trace_scan_block_kernel(int64_t *v, int64_t n, int64_t *totals)
{
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    const int64_t count = n - base < kScanTile ? n - base : kScanTile;
    const int64_t total = scan_tile(v + base, count, 0);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the tile sums, tile by tile with a carry; the grand total is the ray count, offsets[n]
__global__ __launch_bounds__(rlsh::kBlock) void trace_scan_totals_kernel(int64_t *totals, int64_t tiles, int64_t *ray_count)
{
    int64_t carry = 0;
    for (int64_t b = 0; b < tiles; b += kScanTile) {
        const int64_t count = tiles - b < kScanTile ? tiles - b : kScanTile;
        carry += scan_tile(totals + b, count, carry);
    }
    if (threadIdx.x == 0) *ray_count = carry;
}

__global__ __launch_bounds__(rlsh::kBlock) void trace_scan_add_kernel(int64_t *v, int64_t n, const int64_t *totals)
{
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * rlsh::kBlock)
        v[j] += totals[j / kScanTile];
}
#endif
// (What follows, down to the node resolves, is templates and inline device functions: the mode-free kernels among them are
// instantiated by the EXACT unit's host code alone; rlSkin's node resolve, built per math mode, uses the walks in both units.)

// A tile of P consecutive points (P * spp <= kCompactSlots): sample (i, s) moves from staging slot s * n + i to queue position
// offsets[i] + rank.  Through LDS, one plane at a time, so that both sides are coalesced: the staging is read in rows (one
// sample of P consecutive points), the tile's rays are one contiguous range of the queue and are written in order.
template <int NW>
__global__ __launch_bounds__(rlsh::kBlock) void trace_compact_kernel(TraceCompactIO a)
{
    constexpr int kPer = kCompactSlots / rlsh::kBlock;         // slots per thread: their loads are issued together
    __shared__ float buf[kCompactSlots];         // one plane of the tile's rays, in queue order
    __shared__ int64_t off[kCompactMaxPoints + 1];
    const rls_ray_queue &q = a.q;
    const int P = a.tile_points;
    const int64_t tiles = (a.n + P - 1) / P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        const int slots = pc * a.spp;
        __syncthreads();                                         // the previous tile is written out
        for (int p = threadIdx.x; p <= pc; p += rlsh::kBlock) off[p] = a.offsets[p0 + p];
        __syncthreads();
        const int64_t base = off[0];
        const int rays = (int)(off[pc] - base);
        // slot t = threadIdx.x + u * kBlock = s * pc + p: its staging index and position in the tile's range (-1: dropped)
        int64_t src_at[kPer];
        uint16_t tag[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int t = (int)threadIdx.x + u * rlsh::kBlock, s = t / pc, p = t - s * pc;
            src_at[u] = staging_slot(s, a.n, p0) + p;
            tag[u] = t < slots ? a.tag[src_at[u]] : kDropped;
        }
        int pos[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int t = (int)threadIdx.x + u * rlsh::kBlock, s = t / pc, p = t - s * pc;
            pos[u] = tag[u] == kDropped ? -1 : (int)(off[p] - base) + tag_rank(tag[u]);
        }
        for (int plane = 0; plane < 3 + NW; plane++) {
            const float *src = plane < 3 ? a.sdir[plane] : a.sw[plane - 3];
            float *out = plane == 0 ? q.dir.x : plane == 1 ? q.dir.y : plane == 2 ? q.dir.z
                       : plane == 3 ? q.weight.r : plane == 4 ? q.weight.g : q.weight.b;
            float v[kPer];
#pragma unroll
            for (int u = 0; u < kPer; u++) v[u] = pos[u] >= 0 ? src[src_at[u]] : 0.0f;
#pragma unroll
            for (int u = 0; u < kPer; u++) if (pos[u] >= 0) buf[pos[u]] = v[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                const int k = (int)threadIdx.x + u * rlsh::kBlock;
                if (k < rays) out[base + k] = buf[k];
            }
            __syncthreads();
        }
        if (q.point || q.sample || q.kind) {
            uint32_t *ib = (uint32_t *)buf;
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                const int t = (int)threadIdx.x + u * rlsh::kBlock, s = t / pc, p = t - s * pc;
                if (pos[u] >= 0) ib[pos[u]] = (uint32_t)p | (uint32_t)s << 8 | (uint32_t)tag_kind(tag[u]) << 16;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                const int k = (int)threadIdx.x + u * rlsh::kBlock;
                if (k >= rays) continue;
                const uint32_t v = ib[k];
                if (q.point) q.point[base + k] = (uint32_t)(p0 + (v & 0xFF));
                if (q.sample) q.sample[base + k] = (uint8_t)(v >> 8);
                if (NW == 1 && q.kind) q.kind[base + k] = (uint8_t)(v >> 16);
            }
        }
    }
}

// per point the sum over its rays [offsets[i], offsets[i+1]) in queue order.  A workgroup takes kBlock consecutive points,
// i.e. one contiguous range of rays, in tiles of kResolveTile rays: coalesced loads form the products L x weight in LDS,
// then lane i adds those of its own rays, in order (kResolveTile: rls_trace_device.hpp).
// The tile walk over one ray queue for the workgroup's points p0 .. p0 + kBlock - 1 (trace_resolve_kernel and the node
// resolves): acc = the sum over this lane's point's rays of L x weight, in queue order.  Whole workgroup; the walk opens
// with a barrier, so prod may hold an earlier walk's products.  NW: the weight's planes.
template <int NW>
__device__ __forceinline__ void ray_sums(float (*prod)[kResolveTile], const TraceResolveIO &a, int64_t p0, int64_t n,
                                         float (&acc)[3])
{
    const int64_t i = p0 + threadIdx.x;
    const bool live = i < n;
    const int64_t pend = n - p0 < rlsh::kBlock ? n : p0 + rlsh::kBlock;
    const int64_t r0 = a.offsets[p0], r1 = a.offsets[pend];
    const int64_t lo = live ? a.offsets[i] : 0, hi = live ? a.offsets[i + 1] : 0;
    float aR = 0.0f, aG = 0.0f, aB = 0.0f;
    for (int64_t t0 = r0; t0 < r1; t0 += kResolveTile) {
        const int tn = r1 - t0 < kResolveTile ? (int)(r1 - t0) : kResolveTile;
        __syncthreads();                                     // the previous tile's products are consumed
        for (int k = threadIdx.x; k < tn; k += rlsh::kBlock) {
            const int64_t q = t0 + k;
            if (NW == 3) {
                prod[0][k] = a.L.r[q] * a.w[0][q]; prod[1][k] = a.L.g[q] * a.w[1][q]; prod[2][k] = a.L.b[q] * a.w[2][q];
            } else {
                const float wq = a.w[0][q];
                prod[0][k] = a.L.r[q] * wq; prod[1][k] = a.L.g[q] * wq; prod[2][k] = a.L.b[q] * wq;
            }
        }
        __syncthreads();
        const int64_t b = lo > t0 ? lo : t0, e = hi < t0 + tn ? hi : t0 + tn;
        for (int64_t q = b; q < e; q++) {
            aR += prod[0][q - t0]; aG += prod[1][q - t0]; aB += prod[2][q - t0];
        }
    }
    acc[0] = aR; acc[1] = aG; acc[2] = aB;
}

template <int NW>
__global__ __launch_bounds__(rlsh::kBlock) void trace_resolve_kernel(TraceResolveIO a)
{
    __shared__ float prod[3][kResolveTile];
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float acc[3];
        ray_sums<NW>(prod, a, p0, a.n, acc);
        if (i < a.n) {
            if (NW == 1) { acc[0] *= a.scale; acc[1] *= a.scale; acc[2] *= a.scale; }
            a.out.r[i] = acc[0]; a.out.g[i] = acc[1]; a.out.b[i] = acc[2];
        }
    }
}

// The node resolves' walk over one ray queue: the sum over this lane's point's rays of L x weight, x inv, formed about a
// reference radiance so that a UNIFORM radiance gives the analytic call's bits.  Per channel, with Lref = the radiance of
// smallest magnitude among the point's rays (the first such in queue order; a property of the set of rays, not of their order):
//     A = sum w (in queue order: the analytic loop's sum),  B = sum (L - Lref) w,   S = (A inv) Lref + B inv
// In exact arithmetic S = inv sum L w.  Where every ray of the point carries the same radiance env, every term of B is
// exactly 0 -- also where a weight is infinite: a term whose L - Lref is 0 is skipped, which changes no finite sum (B is never
// -0) -- and S = (A inv) env: what ggx_shade_kernel / disney_shade_kernel form from their sum and env (csrc/shade.hip), for
// env = 1 and for any other.  Rounding: with k rays, |S - inv sum L w| <= (k + 3) 2^-24 inv (|Lref| sum |w| +
// sum |L - Lref| |w|); |Lref| <= |L| on every ray, so that is at most 3 (k + 3) 2^-24 inv sum |L| |w| (2 for radiances of one
// sign): a bound relative to the sum of the terms' magnitudes, as the plain sum's, whatever single ray is bright.
// Lref is found in a pass of its own over the lane's rays in global memory (they are read again, coalesced, by the tiles).
// The radiance and the weight of a tile go to LDS side by side (coalesced loads), lane i multiplies.
// planes: 3 + NW rows.  A point without rays: S = 0.
template <int NW>
__device__ __forceinline__ void ray_sums_about_reference(float (*planes)[kResolveTile], const TraceResolveIO &a, int64_t p0,
                                                         int64_t n, float inv, float (&S)[3])
{
    const int64_t i = p0 + threadIdx.x;
    const bool live = i < n;
    const int64_t pend = n - p0 < rlsh::kBlock ? n : p0 + rlsh::kBlock;
    const int64_t r0 = a.offsets[p0], r1 = a.offsets[pend];
    const int64_t lo = live ? a.offsets[i] : 0, hi = live ? a.offsets[i + 1] : 0;
    float ref[3] = { 0.0f, 0.0f, 0.0f };
    if (hi > lo) { ref[0] = a.L.r[lo]; ref[1] = a.L.g[lo]; ref[2] = a.L.b[lo]; }
    for (int64_t q = lo + 1; q < hi; q++) {
        const float v[3] = { a.L.r[q], a.L.g[q], a.L.b[q] };
#pragma unroll
        for (int c = 0; c < 3; c++) if (absf(v[c]) < absf(ref[c])) ref[c] = v[c];
    }
    float A[3] = { 0.0f, 0.0f, 0.0f }, B[3] = { 0.0f, 0.0f, 0.0f };
    for (int64_t t0 = r0; t0 < r1; t0 += kResolveTile) {
        const int tn = r1 - t0 < kResolveTile ? (int)(r1 - t0) : kResolveTile;
        __syncthreads();                                     // the previous tile is consumed
        for (int k = threadIdx.x; k < tn; k += rlsh::kBlock) {
            const int64_t q = t0 + k;
            planes[0][k] = a.L.r[q]; planes[1][k] = a.L.g[q]; planes[2][k] = a.L.b[q];
#pragma unroll
            for (int c = 0; c < NW; c++) planes[3 + c][k] = a.w[c][q];
        }
        __syncthreads();
        const int64_t b = lo > t0 ? lo : t0, e = hi < t0 + tn ? hi : t0 + tn;
        for (int64_t q = b; q < e; q++) {
            const int k = (int)(q - t0);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float w = planes[3 + (NW == 3 ? c : 0)][k];
                if (NW == 3 || c == 0) A[c] += w;
                // (a ray AT the reference adds nothing, whatever its weight: 0 x inf would be NaN where the analytic sum is inf.
                // That is all the skip guarantees -- the uniform radiance of the contract; under a non-uniform radiance an infinite
                // weight may still meet Lref = 0 in (A inv) Lref and give NaN where the plain sum is inf)
                const float d = planes[c][k] - ref[c];
                B[c] += d == 0.0f ? 0.0f : d * w;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) S[c] = (A[NW == 3 ? c : 0] * inv) * ref[c] + B[c] * inv;
}

// trace_compact_kernel for the light loops' queue: a tile of P consecutive points with a.slots slots each (P * slots <=
// kShadowMaxSlots; one point at the limits of 8 lights x 3 segments x 256 samples).  Slot t = sp * pc + p of the tile is slot sp
// of its point p: the staging is read in rows, the tile's rays are one contiguous range of the queue.  The positions are kept
// in LDS (a thread has up to 24 slots), the planes go through buf one at a time.  NWD: the planes of weight_diffuse.
// Limits of this shape: a staging row is pc points wide, so with many slots per point (tile_points = 6144 / slots: 64 at 2
// lights x 16 samples, 1 at the maximum) the tag and plane reads are short runs n words apart rather than full cache lines, and
// every plane's pass walks all the tile's slots (through pos), kept or not.
// HITS: the queue over rlSss's hit list (rls_trace_hits.hpp): no weight_specular planes, staged or queued, and a point without
// rays -- every entry past the list's end -- has no tags staged: its slots read as dropped.
template <int NWD, bool HITS>
__device__ __forceinline__ void shadow_compact_tiles(const ShadowCompactIO &a)
{
    __shared__ float buf[kShadowMaxSlots];           // one plane of the tile's rays, in queue order
    __shared__ int16_t pos[kShadowMaxSlots];         // slot -> its ray's place in the tile's range, -1: dropped
    static_assert(kShadowMaxSlots <= 32767, "pos holds a slot's place in 16 bits");
    static_assert(kCompactMaxPoints <= 256 && kMaxSpp <= 256, "ib packs the point's index in the tile and the sample in 8 bits each");
    static_assert(kShadowMaxSlots <= 0x10000, "the tag's rank is 16 bits");
    __shared__ int64_t off[kCompactMaxPoints + 1];
    const rls_shadow_queue &q = a.q;
    const int P = a.tile_points;
    const int64_t tiles = (a.n + P - 1) / P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        const int slots = pc * a.slots;
        __syncthreads();                                         // the previous tile is written out
        for (int p = threadIdx.x; p <= pc; p += rlsh::kBlock) off[p] = a.offsets[p0 + p];
        __syncthreads();
        const int64_t base = off[0];
        const int rays = (int)(off[pc] - base);
        if (HITS && rays == 0) continue;
        // (sp, p) of this thread's slots t = threadIdx.x, + kBlock, ...: advanced without a division per slot
        const int sp0 = (int)threadIdx.x / pc, pp0 = (int)threadIdx.x - sp0 * pc;
        const int dsp = rlsh::kBlock / pc, dp = rlsh::kBlock - dsp * pc;
        uint32_t *ib = (uint32_t *)buf;
        for (int t = threadIdx.x, sp = sp0, p = pp0; t < slots; t += rlsh::kBlock) {
            const uint32_t tag = HITS && off[p + 1] == off[p] ? kShadowDropped : a.tag[staging_slot(sp, a.n, p0 + p)];
            int at = -1;
            if (tag != kShadowDropped) {
                at = (int)(off[p] - base) + (int)(tag & 0xFFFFu);
                ib[at] = (uint32_t)p | (uint32_t)(sp % a.spp) << 8 | (tag >> 16) << 16;
            }
            pos[t] = (int16_t)at;
            sp += dsp; p += dp;
            if (p >= pc) { p -= pc; sp++; }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < rays; k += rlsh::kBlock) {
            const uint32_t v = ib[k];
            q.kind[base + k] = (uint8_t)(v >> 16);
            if (q.point) q.point[base + k] = (uint32_t)(p0 + (v & 0xFF));
            if (q.sample) q.sample[base + k] = (uint8_t)(v >> 8);
        }
        for (int plane = 0; plane < 7 + NWD; plane++) {
            if (HITS && plane >= 4 && plane < 7) continue;
            const float *src = a.src[plane];
            float *out = plane == 0 ? q.dir.x : plane == 1 ? q.dir.y : plane == 2 ? q.dir.z : plane == 3 ? q.maxdist
                       : plane == 4 ? q.weight_specular.r : plane == 5 ? q.weight_specular.g : plane == 6 ? q.weight_specular.b
                       : plane == 7 ? q.weight_diffuse.r : plane == 8 ? q.weight_diffuse.g : q.weight_diffuse.b;
            __syncthreads();                                     // buf's previous contents are written out
            for (int t = threadIdx.x, sp = sp0, p = pp0; t < slots; t += rlsh::kBlock) {
                const int at = pos[t];
                if (at >= 0) buf[at] = src[staging_slot(sp, a.n, p0 + p)];
                sp += dsp; p += dp;
                if (p >= pc) { p -= pc; sp++; }
            }
            __syncthreads();
            for (int k = threadIdx.x; k < rays; k += rlsh::kBlock) out[base + k] = buf[k];
        }
    }
}

template <int NWD>
__global__ __launch_bounds__(rlsh::kBlock) void shadow_compact_kernel(ShadowCompactIO a)
{
    shadow_compact_tiles<NWD, false>(a);
}
#if !RLS_FAST
__global__ __launch_bounds__(rlsh::kBlock) void hits_compact_kernel(ShadowCompactIO a)
{
    shadow_compact_tiles<1, true>(a);
}
#endif

// The light loops' sums with the traced visibility.  Like trace_resolve_kernel a workgroup takes kBlock consecutive points, one
// contiguous range of rays, in tiles: coalesced loads form visibility x weight of both lobes in LDS, then lane i walks its own
// point's rays in queue order -- lights ascending -- and keeps the analytic loop's four sums per light (light or BSDF strategy x
// lobe), closing a light with s = light_sum + bsdf_sum, t = (radiance * s) * inv, the first light assigning
// (ggx_direct_loops / disney_direct_loops, rls_loops.hpp).  A light without rays is closed too: it adds radiance * 0 * inv.
// NWD = 1 (rlGgx): weight_diffuse is one plane, and the tail diffuse *= KdColor * Kd, specular *= Ks follows (src/rlGgx.cpp:304-305).
// (kShadowTile: rls_trace_device.hpp)

// the lights' radiance into LDS, once per workgroup (the walk below indexes it by a per-lane light)
__device__ __forceinline__ void stage_radiance(float (*rad)[3], const ShadowResolveIO &a)
{
    if (threadIdx.x < RLS_MAX_LIGHTS * 3) rad[threadIdx.x / 3][threadIdx.x % 3] = a.rad[threadIdx.x / 3][threadIdx.x % 3];
    __syncthreads();
}

// The tile walk over the light loops' queue for the workgroup's points p0 .. p0 + kBlock - 1 (shadow_resolve_kernel and the
// node resolves): oS / oD = the point's specular / diffuse sum over the lights, before rlGgx's tail.  Whole workgroup; opens
// with a barrier like ray_sums.
// SPEC = false: a queue without weight_specular planes (the hit list's): oS is +0.
template <int NWD, bool SPEC = true>
__device__ __forceinline__ void shadow_sums(float (*prod)[kShadowTile], uint8_t *kinds, const float (*rad)[3],
                                            const ShadowResolveIO &a, int64_t p0, float (&oS)[3], float (&oD)[3])
{
    // NWD = 0: a lobe of rlSkin (ggx_light_loops, rls_loops.hpp): no diffuse term, and ONE sum per light that takes the rays of
    // both strategies in queue order; the lights' terms are added to +0
    constexpr bool GGX = NWD == 1, ONE = NWD == 0;
    const int64_t i = p0 + threadIdx.x;
    const bool live = i < a.n;
    const int64_t pend = a.n - p0 < rlsh::kBlock ? a.n : p0 + rlsh::kBlock;
    const int64_t r0 = a.offsets[p0], r1 = a.offsets[pend];
    const int64_t lo = live ? a.offsets[i] : 0, hi = live ? a.offsets[i + 1] : 0;
    float lS[3] = { 0.0f, 0.0f, 0.0f }, lD[3] = { 0.0f, 0.0f, 0.0f }, bS[3] = { 0.0f, 0.0f, 0.0f }, bD[3] = { 0.0f, 0.0f, 0.0f };
    for (int c = 0; c < 3; c++) { oS[c] = 0.0f; oD[c] = 0.0f; }
    int l = 0;
    auto close_light = [&]() {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            // (ONE: bS stays +0, and a sum that starts at +0 is never -0: lS + bS is lS)
            const float tS = rad[l][c] * (lS[c] + bS[c]) * a.inv, tD = rad[l][c] * (lD[c] + bD[c]) * a.inv;
            oS[c] = l == 0 && !ONE ? tS : oS[c] + tS;
            oD[c] = l == 0 ? tD : oD[c] + tD;
            lS[c] = 0.0f; lD[c] = 0.0f; bS[c] = 0.0f; bD[c] = 0.0f;
        }
        l++;
    };
    for (int64_t t0 = r0; t0 < r1; t0 += kShadowTile) {
        const int tn = r1 - t0 < kShadowTile ? (int)(r1 - t0) : kShadowTile;
        __syncthreads();                                     // the previous tile's products are consumed
        for (int k = threadIdx.x; k < tn; k += rlsh::kBlock) {
            const int64_t r = t0 + k;
            const float vr = a.vis.r[r], vg = a.vis.g[r], vb = a.vis.b[r];
            if (SPEC) { prod[0][k] = vr * a.ws[0][r]; prod[1][k] = vg * a.ws[1][r]; prod[2][k] = vb * a.ws[2][r]; }
            if (GGX) {
                const float wd = a.wd[0][r];
                prod[3][k] = vr * wd; prod[4][k] = vg * wd; prod[5][k] = vb * wd;
            } else if (!ONE) {
                prod[3][k] = vr * a.wd[0][r]; prod[4][k] = vg * a.wd[1][r]; prod[5][k] = vb * a.wd[2][r];
            }
            kinds[k] = a.kind[r];
        }
        __syncthreads();
        const int64_t b = lo > t0 ? lo : t0, e = hi < t0 + tn ? hi : t0 + tn;
        for (int64_t r = b; r < e; r++) {
            const int k = (int)(r - t0), kind = kinds[k];
            const int lk = (kind & RLS_SHADOW_LIGHT_MASK) < a.nl ? (kind & RLS_SHADOW_LIGHT_MASK) : a.nl - 1;
            while (l < lk) close_light();
            if (ONE) {
                lS[0] += prod[0][k]; lS[1] += prod[1][k]; lS[2] += prod[2][k];
            } else if (kind & RLS_SHADOW_BSDF) {
                if (SPEC && (kind & RLS_SHADOW_SPECULAR)) { bS[0] += prod[0][k]; bS[1] += prod[1][k]; bS[2] += prod[2][k]; }
                if (kind & RLS_SHADOW_DIFFUSE) { bD[0] += prod[3][k]; bD[1] += prod[4][k]; bD[2] += prod[5][k]; }
            } else {
                if (SPEC && (kind & RLS_SHADOW_SPECULAR)) { lS[0] += prod[0][k]; lS[1] += prod[1][k]; lS[2] += prod[2][k]; }
                if (kind & RLS_SHADOW_DIFFUSE) { lD[0] += prod[3][k]; lD[1] += prod[4][k]; lD[2] += prod[5][k]; }
            }
        }
    }
    if (live) {
        while (l < a.nl) close_light();
    }
}

// rlGgx's node parameters at point i, as ggx_shade_kernel forms them (src/rlGgx.cpp:279, 308)
struct GgxTail { float ks, d[3], t[3]; };
__device__ __forceinline__ GgxTail ggx_tail(const rls_material_index &materials, const rls_ggx_shader &sh, int64_t i, bool kt)
{
    GgxTail r = {};
    const PIndex<int64_t> pk = pindex(materials, i);
    const float kd = ldp(sh.Kd, pk);
    r.ks = ldp(sh.Ks, pk);
    ldrgb(sh.KdColor, pk, r.d[0], r.d[1], r.d[2]);
    r.d[0] *= kd; r.d[1] *= kd; r.d[2] *= kd;                // diffuseColor, src/rlGgx.cpp:279
    if (kt) {
        const float k = ldp(sh.Kt, pk);
        ldrgb(sh.KtColor, pk, r.t[0], r.t[1], r.t[2]);
        r.t[0] *= k; r.t[1] *= k; r.t[2] *= k;               // ktColor, :308
    }
    return r;
}

template <int NWD>
__global__ __launch_bounds__(rlsh::kBlock) void shadow_resolve_kernel(ShadowResolveIO a)
{
    constexpr bool GGX = NWD == 1;
    __shared__ float prod[6][kShadowTile];           // visibility x weight_specular, visibility x weight_diffuse
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    stage_radiance(rad, a);
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float oS[3], oD[3];
        shadow_sums<NWD>(prod, kinds, rad, a, p0, oS, oD);
        if (i < a.n) {
            if (GGX) {
                const GgxTail t = ggx_tail(a.materials, a.sh, i, false);
                strgb(a.ds, i, oS[0] * t.ks, oS[1] * t.ks, oS[2] * t.ks);
                strgb(a.dd, i, oD[0] * t.d[0], oD[1] * t.d[1], oD[2] * t.d[2]);
            } else {
                strgb(a.ds, i, oS[0], oS[1], oS[2]);
                strgb(a.dd, i, oD[0], oD[1], oD[2]);
            }
        }
    }
}
